#!/usr/bin/env python3
"""Timing of the UI's view (gsdf_hip_render3; kernels_view.h) on the GPU: per-tree kernels, 1920 x 1080, aa = 1 and 3.

For each scene and aa: ms per frame (host clock around `--frames` blocking frames, after `--warmup` frames; the frame's outputs
stay on the device, so the time is allocation + kernel + the counter's read-back), rays/s, SDF evaluations/s, and the A/B of the
refilling kernel against the plain one (GSDF_HIP_VIEW_REFILL), alternated `--rounds` times within this one process; then the same
tree's eval_kernel on a flat lattice of device-resident points (gsdf_hip_eval3_dev) as the ceiling the view is measured against.
One JSON line per measurement. Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own.

    python tools/view_bench.py [--scenes npt-flange,bolt] [--width 1920 --height 1080] [--frames 20] [--rounds 3]
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def frame_ms(hip, sdf, view, w, h, frames, plain):
    os.environ["GSDF_HIP_VIEW_REFILL"] = "0" if plain else "1"
    L = hip.lib()
    e0 = sdf.Evaluations()
    t0 = time.perf_counter()
    for _ in range(frames):
        hip._check(L.gsdf_hip_render3(sdf._h, C.byref(view), w, h, None, None, None))  # blocking: ends in a stream synchronise
    dt = time.perf_counter() - t0
    return dt * 1e3 / frames, (sdf.Evaluations() - e0) // frames


def lattice_rate(hip, sdf, n_side, reps):
    import torch
    bb = sdf.Bounds()
    axes = [torch.linspace(float(bb[a]), float(bb[a + 3]), n_side, dtype=torch.float32, device="cuda") for a in range(3)]
    pos = torch.stack(torch.meshgrid(*axes, indexing="ij"), -1).reshape(-1, 3).contiguous()
    dist = torch.empty(pos.shape[0], dtype=torch.float32, device="cuda")
    n = pos.shape[0]
    for _ in range(3):
        sdf.evaluate_dev(pos.data_ptr(), 12, dist.data_ptr(), n)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        sdf.evaluate_dev(pos.data_ptr(), 12, dist.data_ptr(), n)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    return n / dt, dt * 1e3, n


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="npt-flange,bolt")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--yaw", type=float, default=0.7)
    ap.add_argument("--pitch", type=float, default=0.45)
    ap.add_argument("--frames", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--lattice", type=int, default=256, help="points per side of the eval_kernel lattice")
    ap.add_argument("--no-lattice", action="store_true")
    args = ap.parse_args(argv)

    try:
        import torch  # noqa: F401  (initialised before the library's runtime: tests/conftest.py explains why)
        torch.cuda.init()
    except Exception:
        pass
    from gsdf_amd import hip
    from scaffold.builder import Builder

    hip.init(0)
    w, h = args.width, args.height
    for scene in args.scenes.split(","):
        sdf = hip.SDF3HIP(Builder().Scene(scene)).specialize()
        for aa in (1, 3):
            v = hip.view_orbit(sdf.Bounds(), args.yaw, args.pitch, aa=aa)
            for plain in (False, True):
                frame_ms(hip, sdf, v, w, h, args.warmup, plain)  # builds / loads the view module, warms both forms
            res = {False: [], True: []}
            evals = 0
            for _ in range(args.rounds):
                for plain in (False, True):
                    ms, evals = frame_ms(hip, sdf, v, w, h, args.frames, plain)
                    res[plain].append(ms)
            rays = w * h * aa * aa
            for plain in (False, True):
                ms = sorted(res[plain])[len(res[plain]) // 2]
                print(json.dumps({"scene": scene, "kernel": "plain" if plain else "refill", "w": w, "h": h, "aa": aa, "frames": args.frames,
                                  "rounds": args.rounds, "ms_per_frame_median": round(ms, 4), "ms_per_frame_all": [round(x, 4) for x in res[plain]],
                                  "rays_per_s": rays / (ms * 1e-3), "evals_per_frame": int(evals), "evals_per_s": evals / (ms * 1e-3),
                                  "kernels": sdf.info()["kernels"].get("eval", "")}), flush=True)
        if not args.no_lattice:
            rate, ms, n = lattice_rate(hip, sdf, args.lattice, 20)
            print(json.dumps({"scene": scene, "kernel": "eval_kernel (flat lattice, device-resident)", "points": n, "ms": round(ms, 4),
                              "evals_per_s": rate, "kernels": sdf.info()["kernels"].get("eval", "")}), flush=True)
    os.environ.pop("GSDF_HIP_VIEW_REFILL", None)
    return 0


if __name__ == "__main__":
    sys.exit(main())
