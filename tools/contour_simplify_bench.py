#!/usr/bin/env python3
"""Timing of the loops' simplification and measures (gsdf_hip_contour_simplify / gsdf_hip_contour_measures;
kernels_contour_simplify.h) on the GPU, the numbers of DESIGN.md section 8: the `text` scene's outline on the lattice of
tools/contour_bench.py (about 4096^2 nodes), beside that handle's own ms_trace, and a synthetic circle of 200 000 vertices at 16 levels.

For each case: the device time (HIP events; the host's waits between the passes left out) of a simplification at tol = res / 8 (the
circle: 0.75 and 600 at radius 1000), one pass and three, and of the measures, median of --reps calls after one warm-up; the vertices
before and after, max_dev, the largest span level. One JSON line per measurement.

    python tools/contour_simplify_bench.py [--reps 3]
"""
import argparse
import importlib.util
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _example():
    spec = importlib.util.spec_from_file_location("render_svg", os.path.join(ROOT, "examples", "render_svg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def median(v):
    return sorted(v)[len(v) // 2]


def run(hip, name, c, tol, levels, passes, reps, extra):
    c.simplify(tol, levels, passes, dry=True)  # warm-up
    c.measures()
    ms, ms_dry, ms_meas = [], [], []
    for _ in range(reps):
        out, st = c.simplify(tol, levels, passes)
        ms.append(st.ms_device)
        ms_dry.append(c.simplify(tol, levels, passes, dry=True)[1].ms_device)
        c.measures()
        ms_meas.append(hip.ContourHIP.measures_ms())
    print(json.dumps(dict(extra, case=name, tol=float(tol), levels=levels, passes=passes, loops=c.n_loops, verts_in=int(st.n_verts_in), verts_out=int(st.n_verts_out),
                          loops_changed=int(st.loops_changed), max_dev=st.max_dev, max_level=st.max_level, ms_simplify=round(median(ms), 4),
                          ms_simplify_dry=round(median(ms_dry), 4), ms_measures=round(median(ms_meas), 4), reps=reps)), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
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
    sdf = hip.SDF2HIP(ex.scene("text")).specialize()
    bb = sdf.Bounds()
    res = np.float32(math.sqrt(float(bb[3] - bb[0]) * float(bb[4] - bb[1]) / 4096.0 ** 2))
    ex.trace(hip, sdf, res)  # warm-up (loads the per-tree module)
    traces = [ex.trace(hip, sdf, res) for _ in range(args.reps)]
    c = traces[-1]
    extra = {"res": float(res), "ms_trace": round(median([t.stats.ms_trace for t in traces]), 3), "ms_eval": round(median([t.stats.ms_eval for t in traces]), 3)}
    for passes in (1, 3):
        run(hip, "text", c, np.float32(res / np.float32(8)), 8, passes, args.reps, extra)
    n = 200_000
    th = np.arange(n, dtype=np.float64) * (2 * math.pi / n)
    circle = hip.ContourHIP.from_arrays(np.stack([1000 * np.cos(th), 1000 * np.sin(th)], 1).astype(np.float32), [0, n])
    for tol in (0.75, 600.0):
        run(hip, "circle", circle, np.float32(tol), 16, 1, args.reps, {})
    return 0


if __name__ == "__main__":
    sys.exit(main())
