#!/usr/bin/env python3
"""Device time of gsdf_hip_indexed_project (project_kernel) beside gsdf_hip_indexed_normals (normals_kernel) on the same vertices,
program and kernel form: one JSON line per scene and form (profiles/project_bench.jsonl).

    python tools/project_bench.py [--reps 7] [--warmup 2]

npt-flange at resdiv 400 simplified at 4 res, bolt at resdiv 200 (welded, not simplified); interpreter and per-tree kernels.
Two kinds of time, never mixed in one ratio:
  project_ms, deviation_ms        the kernel's own time (HIP events around the launch, gsdf_project_stats.ms_device)
  project_wall_ms, normals_wall_ms  the host clock around the blocking call (launch, kernel, synchronisation, the counters' copy):
                                   like for like between the two calls, and what `wall_ratio` compares
The two KERNELS' device times side by side come from a profiler run of this tool (rocprofv3 --kernel-trace --stats), a run of its own.
`lane_occupancy_min` is a lower bound of the share of lane-evaluations that counted: a vertex with s accepted steps pays at most
s + 1 centre evaluations and s + 1 gradients, and a wave pays for its own slowest lane, which is at most the mesh's slowest
(steps_max): evaluations / (64 x waves x 7 x (steps_max + 1)). Median of the repetitions after the warm-up."""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args(argv)
    import numpy as np
    from gsdf_amd import hip
    from scaffold.builder import Builder

    hip.init(0)
    for scene, resdiv, cell_res in (("npt-flange", 400, 4.0), ("bolt", 200, 0.0)):
        shape = Builder().Scene(scene)
        res = np.float32(float(shape.Diagonal()) / resdiv)
        for form in ("interpreter", "specialised"):
            sdf = hip.SDF3HIP(shape)
            if form == "specialised":
                sdf.specialize()
            mesh = hip.OctreeHIP(sdf, res, payload=hip.PAYLOAD_RECORDS)
            ix = mesh.weld()
            max_move = res
            if cell_res:
                ix, _ = ix.simplify(np.float32(cell_res) * res, tuple(np.float32(o) - np.float32(0.5) * res for o in mesh.stats.origin[:]))
                max_move = np.float32(cell_res) * res
            o = dict(step=res / np.float32(4), tol=res / np.float32(1024), max_move=max_move, max_iters=8)
            ms_p, ms_n, ms_d, ms_pw = [], [], [], []
            for k in range(args.warmup + args.reps):
                tp = time.perf_counter()
                _, st = ix.project(sdf, dry=True, **o)
                tp = time.perf_counter() - tp
                dv = ix.deviation(sdf, o["tol"])
                t0 = time.perf_counter()
                ix.normals(sdf, o["step"])
                t1 = time.perf_counter()
                if k >= args.warmup:
                    ms_p.append(st.ms_device)
                    ms_d.append(dv.ms_device)
                    ms_n.append((t1 - t0) * 1e3)
                    ms_pw.append(tp * 1e3)
            out, st = ix.project(sdf, **o)
            med_p, med_n, med_d, med_pw = statistics.median(ms_p), statistics.median(ms_n), statistics.median(ms_d), statistics.median(ms_pw)
            line = {"scene": scene, "resdiv": resdiv, "cell_res": cell_res, "form": form, "kernel": sdf.info()["kernels"]["project"], "n_verts": ix.n_verts,
                    "n_tris": ix.n_tris, "counts": {n: int(st.count[k]) for k, n in enumerate(hip.PROJECT_STATUS)}, "evals": int(st.evals),
                    "steps_max": int(st.steps_max), "max_abs_before": float(st.max_abs_before), "max_abs_after": float(st.max_abs_after), "res": float(res),
                    "over_tol_before": int(st.over_tol_before), "over_tol_after": int(st.over_tol_after), "project_ms": med_p,
                    "project_evals_per_s": st.evals / (med_p * 1e-3), "deviation_ms": med_d, "deviation_evals_per_s": ix.n_verts / (med_d * 1e-3),
                    "project_wall_ms": med_pw, "project_evals_per_s_wall": st.evals / (med_pw * 1e-3),
                    "normals_wall_ms": med_n, "normals_evals": 6 * ix.n_verts, "normals_evals_per_s_wall": 6 * ix.n_verts / (med_n * 1e-3),
                    "wall_ratio": (st.evals / med_pw) / (6 * ix.n_verts / med_n),
                    "lane_occupancy_min": st.evals / (64.0 * 7.0 * ((ix.n_verts + 63) // 64) * (int(st.steps_max) + 1)),
                    "volume_before": ix.report().volume, "volume_after": out.report().volume, "misoriented_after": int(out.report().misoriented_edges),
                    "reps": args.reps, "warmup": args.warmup}
            print(json.dumps(line), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
