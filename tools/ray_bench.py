#!/usr/bin/env python3
"""Timing of rays (gsdf_hip_raycast3; kernels_ray.h) against the UI's view (gsdf_hip_render3; kernels_view.h) on the GPU, and of the
wall thickness of a welded mesh (gsdf_hip_indexed_thickness).

The primary rays of examples/view_part.py's frame -- 1920 x 1080, aa = 1, generated on the host from tests/viewref.py's statements
-- go through gsdf_hip_raycast3 with tol 1e-4, min_step 0, refine 0: both kernels then run the same one-point lockstep loop, the
view's four normal taps per hit aside. Per frame: the rays' ms_device (HIP events around ray_kernel) and evals, and the view's
blocking frame on the host clock (its outputs stay on the device: allocation + kernel + the counter's read-back) with its evals;
`--frames` of each, alternated, so the spread of each is on record. The view's KERNEL time: run this under
`rocprofv3 --kernel-trace --stats` in a run of its own and read view_kernel and ray_kernel off the statistics.
The rays go in twice: in the image's row-major order (a wave is 64 pixels of one row), and in view_kernel's own order (8 x 8 screen
tiles, one per wave). A wave pays every trip for its slowest lane, so beside the evaluations each line has `wave_trips`: the sum
over the waves of the most evaluations of any of their lanes -- what the kernel's time is proportional to.
Then the thickness of the scene's welded mesh at --resdiv with the example's options: evals per vertex and ms_device.
One JSON line per measurement.

    python tools/ray_bench.py [--scene npt-flange] [--width 1920 --height 1080] [--frames 20] [--resdiv 400]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
F = np.float32


def primary_rays(view, w, h):
    """(origins, directions) of the frame's aa = 1 samples, row 0 at the top: viewref.render's statements."""
    ro = np.array(view.ro[:], F)
    uu, vv, ww = np.array(view.uu[:], F), np.array(view.vv[:], F), np.array(view.ww[:], F)
    r, i = np.divmod(np.arange(w * h), w)
    fx = i.astype(F) + F(0.5)
    fy = (h - 1 - r).astype(F) + F(0.5)
    fw, fh = F(w), F(h)
    ox = oy = F(F(0) / F(1)) - F(0.5)
    px = (F(2) * (fx + ox) - fw) / fh
    py = (F(2) * (fy + oy) - fh) / fh
    x = (px * uu[0] + py * vv[0]) + F(1.5) * ww[0]
    y = (px * uu[1] + py * vv[1]) + F(1.5) * ww[1]
    z = (px * uu[2] + py * vv[2]) + F(1.5) * ww[2]
    n = np.sqrt((x * x + y * y) + z * z)
    d = np.stack([x / n, y / n, z / n], axis=1).astype(F)
    return np.tile(ro, (w * h, 1)).astype(F), d


def tile_order(w, h, tile=8):
    """Pixel numbers in view_kernel's claim order: tile-major, row-major inside a tile; pixels off the image's edge left out."""
    c = np.arange(((w + tile - 1) // tile) * ((h + tile - 1) // tile) * tile * tile)
    t, k = np.divmod(c, tile * tile)
    tiles_x = (w + tile - 1) // tile
    i, r = (t % tiles_x) * tile + k % tile, (t // tiles_x) * tile + k // tile
    ok = (i < w) & (r < h)
    return (r * w + i)[ok]


def wave_trips(per_lane):
    """Sum over waves of 64 consecutive lanes of the largest count in the wave."""
    n = len(per_lane)
    padded = np.zeros((n + 63) // 64 * 64, np.int64)
    padded[:n] = per_lane
    return int(padded.reshape(-1, 64).max(axis=1).sum())


def spread(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2], "min": xs[0], "max": xs[-1]}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scene", default="npt-flange")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--yaw", type=float, default=0.7)
    ap.add_argument("--pitch", type=float, default=0.45)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--resdiv", type=int, default=400)
    ap.add_argument("--interpreter", action="store_true", help="skip the per-tree kernel build")
    args = ap.parse_args(argv)

    from gsdf_amd import hip
    from scaffold.builder import Builder

    hip.init(0)
    shape = Builder().Scene(args.scene)
    sdf = hip.SDF3HIP(shape)
    if not args.interpreter:
        sdf.specialize()
    w, h = args.width, args.height
    view = hip.view_orbit(sdf.Bounds(), args.yaw, args.pitch, aa=1)
    o, r = primary_rays(view, w, h)
    rows = np.ascontiguousarray(np.concatenate([o, r], axis=1))
    order = tile_order(w, h)
    ro = hip.RayOpts(t0=0.0, tmax=F(F(1.3) * F(view.char_dist)), tol=F(1e-4), min_step=0.0, max_steps=int(view.max_steps), refine=0)
    L = hip.lib()
    evals_px = np.empty((h, w), np.uint32)
    st = hip.RayStats()

    def view_frame(out):
        t0 = time.perf_counter()
        hip._check(L.gsdf_hip_render3(sdf._h, C.byref(view), w, h, None, None, out))
        return (time.perf_counter() - t0) * 1e3

    def ray_frame(rays, steps=None):
        hip._check(L.gsdf_hip_raycast3(sdf._h, rays.ctypes.data, len(rays), C.byref(ro), 0.0, None, None, None, None if steps is None else steps.ctypes.data,
                                       C.byref(st)))
        return st.ms_device

    view_frame(evals_px.ctypes.data)
    view_evals = int(evals_px.sum(dtype=np.uint64))
    view_trips = wave_trips(evals_px.reshape(-1)[order])   # (the image's sizes are multiples of 8: a wave is one whole tile)
    forms = {"row-major": rows, "8x8 tiles": np.ascontiguousarray(rows[order])}
    for _ in range(args.warmup):
        view_frame(None)
        for rays in forms.values():
            ray_frame(rays)
    vms, rms = [], {k: [] for k in forms}
    for _ in range(args.frames):
        vms.append(view_frame(None))
        for k, rays in forms.items():
            rms[k].append(ray_frame(rays))
    kern = sdf.info()["kernels"]
    v = spread(vms)
    print(json.dumps({"scene": args.scene, "what": "render3 (host clock, blocking frame)", "w": w, "h": h, "aa": 1, "frames": args.frames, "ms": v,
                      "evals": view_evals, "ns_per_eval": {k: x * 1e6 / view_evals for k, x in v.items()}, "wave_trips": view_trips,
                      "lane_occupancy": view_evals / (64 * view_trips), "kernel": kern.get("eval", "")}), flush=True)
    for k, rays in forms.items():
        steps = np.empty(len(rays), np.uint16)
        ray_frame(rays, steps)
        rr, trips = spread(rms[k]), wave_trips(steps)
        counts = {n: int(st.count[j]) for j, n in enumerate(hip.RAY_STATUS) if st.count[j]}
        print(json.dumps({"scene": args.scene, "what": "raycast3 (ms_device, events around ray_kernel)", "order": k, "rays": len(rays), "frames": args.frames,
                          "ms": rr, "evals": int(st.evals), "ns_per_eval": {q: x * 1e6 / st.evals for q, x in rr.items()}, "wave_trips": trips,
                          "lane_occupancy": st.evals / (64 * trips), "ns_per_wave_trip": rr["median"] * 1e6 / trips,
                          "rays_per_s": len(rays) / (rr["median"] * 1e-3), "status": counts, "steps_max": int(st.steps_max), "kernel": kern.get("ray", "")}), flush=True)
    # wall thickness of the welded mesh, the example's options
    res = F(float(shape.Diagonal()) / args.resdiv)
    ix = hip.OctreeHIP(sdf, res, payload=hip.PAYLOAD_RECORDS).weld()
    quarter = res / F(4)
    tms = []
    for _ in range(args.warmup + args.frames):
        _, _, ts = ix.thickness(sdf, quarter, quarter, F(shape.Diagonal()), res / F(1024), dry=True)
        tms.append(ts.ms_device)
    t = spread(tms[args.warmup:])
    print(json.dumps({"scene": args.scene, "what": "indexed_thickness (ms_device)", "resdiv": args.resdiv, "verts": int(ts.n), "runs": args.frames, "ms": t,
                      "evals": int(ts.evals), "evals_per_vertex": ts.evals / ts.n, "ns_per_eval": t["median"] * 1e6 / ts.evals,
                      "ns_per_vertex": t["median"] * 1e6 / ts.n, "status": {n: int(ts.count[k]) for k, n in enumerate(hip.RAY_STATUS) if ts.count[k]},
                      "t_min": float(ts.t_min), "t_max": float(ts.t_max), "steps_max": int(ts.steps_max)}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
