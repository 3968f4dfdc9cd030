#!/usr/bin/env python3
"""Timing of a 2-D part's picture (gsdf_hip_image2_color; kernels_image.h) on the GPU, for the reference's example pictures
(examples/render_png.py: image, text, thread) at 1080 and 4320 rows, RenderPNGFile's width.

For each scene, size, kernel form (interpreter / per-tree) and conversion (DEFAULT, IQ, GRADIENT, BW_SMOOTH): ms per picture, host
clock around `--reps` blocking calls after `--warmup`, the RGBA pixels copied back into one host array (allocation + kernel + copy +
synchronise; gsdf_hip_image2 also allocates its distance buffer, which it always fills), median of
`--rounds` rounds that alternate the conversions within this one process; gsdf_hip_image2 (the default conversion's kernel of
kernels_eval.h) the same way as the yardstick. Then render_png's host-inclusive time (picture, copy-back, PNG encoding and file)
and, at 1080 rows, the oracle's CPU render_image for scale. One JSON line per measurement. Kernel times: run this under
`rocprofv3 --kernel-trace --stats` in a run of its own.

    python tools/png_bench.py [--scenes image,text,thread] [--heights 1080,4320] [--reps 10] [--rounds 3]
"""
import argparse
import ctypes as C
import importlib.util
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _example():
    spec = importlib.util.spec_from_file_location("render_png", os.path.join(ROOT, "examples", "render_png.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def picture_ms(hip, sdf, conv, w, h, reps):
    import numpy as np
    L = hip.lib()
    rgba = np.empty((h, w, 4), np.uint8)  # the pixels only (no distances), copied back as a caller gets them
    t0 = time.perf_counter()
    for _ in range(reps):
        if conv is None:
            hip._check(L.gsdf_hip_image2(sdf._h, w, h, None, rgba.ctypes.data))
        else:
            hip._check(L.gsdf_hip_image2_color(sdf._h, C.byref(conv), w, h, rgba.ctypes.data, None))
    return (time.perf_counter() - t0) * 1e3 / reps


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--scenes", default="image,text,thread")
    ap.add_argument("--heights", default="1080,4320")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-oracle", action="store_true")
    args = ap.parse_args(argv)

    import numpy as np
    from gsdf_amd import hip
    from oracle.oracle import OracleSDF

    hip.init(0)
    ex = _example()
    for scene in args.scenes.split(","):
        shape = ex.scene(scene)
        handles = {"interpreter": hip.SDF2HIP(shape), "per-tree": hip.SDF2HIP(shape).specialize()}
        bb = handles["interpreter"].Bounds()
        convs = {"image2 (yardstick)": None, "default": hip.color_default(), "iq": ex.conversion(hip, "iq", bb),
                 "gradient": ex.conversion(hip, "gradient", bb), "bw": ex.conversion(hip, "bw", bb)}
        for height in [int(x) for x in args.heights.split(",")]:
            try:
                w = hip.picture_size(bb, height)
            except hip.HipError as e:  # RenderPNGFile's width beyond the library's 16384 pixels per side
                print(json.dumps({"scene": scene, "h": height, "skipped": str(e)}), flush=True)
                continue
            for form, sdf in handles.items():
                for conv in convs.values():
                    picture_ms(hip, sdf, conv, w, height, args.warmup)  # per-tree: builds / loads the picture module
                res = {k: [] for k in convs}
                for _ in range(args.rounds):
                    for k, conv in convs.items():
                        res[k].append(picture_ms(hip, sdf, conv, w, height, args.reps))
                for k, v in res.items():
                    ms = sorted(v)[len(v) // 2]
                    print(json.dumps({"scene": scene, "w": w, "h": height, "form": form, "conversion": k, "reps": args.reps,
                                      "rounds": args.rounds, "ms_per_picture_median": round(ms, 4), "ms_all": [round(x, 4) for x in v],
                                      "pixels_per_s": w * height / (ms * 1e-3), "kernels": sdf.info()["kernels"].get("eval", "")}), flush=True)
            with tempfile.TemporaryDirectory() as d:
                sdf = handles["per-tree"]
                path = os.path.join(d, "p.png")
                sdf.render_png(path, height)
                t0 = time.perf_counter()
                sdf.render_png(path, height)
                dt = time.perf_counter() - t0
                print(json.dumps({"scene": scene, "w": w, "h": height, "form": "per-tree", "conversion": "iq (RenderPNGFile default)",
                                  "what": "render_png, host-inclusive (picture, copy-back, zlib, file)", "ms": round(dt * 1e3, 2),
                                  "png_bytes": os.path.getsize(path)}), flush=True)
            if not args.no_oracle and height <= 1080:
                orc = OracleSDF(shape.tree())
                t0 = time.perf_counter()
                dist, _ = orc.render_image(w, height)
                dt = time.perf_counter() - t0
                print(json.dumps({"scene": scene, "w": w, "h": height, "form": "oracle (CPU)", "conversion": "default",
                                  "what": "OracleSDF.render_image, row by row", "ms": round(dt * 1e3, 2),
                                  "finite": bool(np.isfinite(dist).all())}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
