#!/usr/bin/env python3
"""Timing of the contour tracer (gsdf_hip_contour2 / gsdf_hip_slice3; kernels_contour.h) on the GPU, the numbers of DESIGN.md
section 8: the `text` scene's outline on a lattice of about 4096^2 nodes, and 256 slices of npt-flange at diagonal / 1600.

For each case and kernel form (interpreter / per-tree): the device time of the two stages from the handle's statistics (ms_eval: the
lattice positions and the program's Evaluate; ms_trace: everything behind it), evaluations per second of the evaluation stage, and the
host clock around the blocking call (allocation, the waits between the stages and the read-back included), median of --reps calls after
one warm-up. Beside them the yardstick: gsdf_hip_eval2_dev / gsdf_hip_eval3_dev alone over the same lattice positions, resident on
the device, in calls of the tracer's default chunk size. One JSON line per measurement.

    python tools/contour_bench.py [--cases text,npt-flange] [--reps 3]
"""
import argparse
import importlib.util
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CHUNK = 1 << 24  # gsdf_hip.h: GSDF_CONTOUR_DEFAULT_MAX_NODES


def _example():
    spec = importlib.util.spec_from_file_location("render_svg", os.path.join(ROOT, "examples", "render_svg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def median(v):
    return sorted(v)[len(v) // 2]


def eval_alone_ms(sdf, st, res, z, reps):
    """The program's Evaluate over the tracer's lattice positions (x0 + i res, y0 + j res, z[k]), already on the device."""
    import torch
    bb = sdf.Bounds()
    xs = (float(bb[0]) - res) + torch.arange(st.nx, dtype=torch.float32, device="cuda") * res
    ys = (float(bb[1]) - res) + torch.arange(st.ny, dtype=torch.float32, device="cuda") * res
    gy, gx = torch.meshgrid(ys, xs, indexing="ij")
    if z is None:
        pos = torch.stack([gx, gy], -1).reshape(-1, 2).contiguous()
    else:
        zz = torch.tensor(z, dtype=torch.float32, device="cuda")
        pos = torch.stack([gx.expand(len(z), -1, -1), gy.expand(len(z), -1, -1), zz[:, None, None].expand(-1, st.ny, st.nx)], -1).reshape(-1, 3).contiguous()
    dim = pos.shape[1]
    n = pos.shape[0]
    per = max(1, CHUNK // (st.nx * st.ny)) * st.nx * st.ny
    dist = torch.empty(n, dtype=torch.float32, device="cuda")

    def run():
        for a in range(0, n, per):
            m = min(per, n - a)
            sdf.evaluate_dev(pos.data_ptr() + a * dim * 4, dim * 4, dist.data_ptr() + a * 4, m)
        torch.cuda.synchronize()

    run()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        run()
        out.append((time.perf_counter() - t0) * 1e3)
    return median(out), n


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cases", default="text,npt-flange")
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args(argv)
    try:
        import torch  # noqa: F401  (initialised before the library's runtime: tests/conftest.py explains why)
        torch.cuda.init()
    except Exception:
        pass
    import numpy as np
    from gsdf_amd import hip

    hip.init(0)
    ex = _example()
    for case in args.cases.split(","):
        shape = ex.scene(case)
        is3d = case in ex.SCENES_3D
        make = hip.SDF3HIP if is3d else hip.SDF2HIP
        handles = {"interpreter": make(shape), "per-tree": make(shape).specialize()}
        bb = handles["interpreter"].Bounds()
        if is3d:
            res = ex.spacing(bb, True, 1600.0)
            z = hip.layer_heights(bb, float(bb[5] - bb[2]) / 256)
        else:
            res = np.float32(math.sqrt(float(bb[3] - bb[0]) * float(bb[4] - bb[1]) / 4096.0 ** 2))
            z = None
        for form, sdf in handles.items():
            ex.trace(hip, sdf, res, z)  # warm-up (per-tree: loads the module)
            ev, tr, wall = [], [], []
            for _ in range(args.reps):
                t0 = time.perf_counter()
                c = ex.trace(hip, sdf, res, z)
                wall.append((time.perf_counter() - t0) * 1e3)
                st = c.stats
                ev.append(st.ms_eval)
                tr.append(st.ms_trace)
            alone, n = eval_alone_ms(sdf, st, float(res), None if z is None else z.tolist(), args.reps)
            print(json.dumps({"case": case, "form": form, "res": float(res), "nx": st.nx, "ny": st.ny, "layers": st.n_layers, "nodes": int(st.evals),
                              "loops": int(st.n_loops), "verts": int(st.n_verts), "rank_rounds": st.rank_rounds, "ms_eval": round(median(ev), 3),
                              "ms_trace": round(median(tr), 3), "ms_wall": round(median(wall), 2), "evals_per_s_eval_stage": st.evals / (median(ev) * 1e-3),
                              "ms_eval_dev_alone": round(alone, 3), "evals_per_s_alone": n / (alone * 1e-3), "reps": args.reps}), flush=True)
            del c
    return 0


if __name__ == "__main__":
    sys.exit(main())
