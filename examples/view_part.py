#!/usr/bin/env python3
"""Look at one of the reference's example parts without meshing it: one frame of gsdfaux.UI's ray-marched view
(gsdfaux/ui.go:247-355), rendered headless on the GPU and written as a PNG:

    python examples/view_part.py npt-flange --width 960 --height 540 --yaw 0.7 --pitch 0.4 --aa 3 -o flange.png

The camera orbits the origin at the UI's default distance (the bounding box's diagonal) unless --cam-dist is given; --aa 3 is
what the UI shows once the mouse rests. The PNG is written with the standard library only (zlib, struct)."""
import argparse
import os
import struct
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def write_png(path, rgba):
    """8-bit RGBA PNG of an (h, w, 4) uint8 array, rows from the top (filter 0 on every row)."""
    h, w = rgba.shape[:2]

    def chunk(kind, body):
        return struct.pack(">I", len(body)) + kind + body + struct.pack(">I", zlib.crc32(kind + body) & 0xffffffff)
    raw = b"".join(b"\x00" + rgba[r].tobytes() for r in range(h))
    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 6, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene", choices=["npt-flange", "bolt", "knurled-cylinder", "glyph-plate", "fibonacci-showerhead"])
    ap.add_argument("--width", type=int, default=960)
    ap.add_argument("--height", type=int, default=540)
    ap.add_argument("--yaw", type=float, default=0.7, help="radians about the vertical axis")
    ap.add_argument("--pitch", type=float, default=0.4, help="radians, clamped to +-(pi/2 - 0.01) as the UI does")
    ap.add_argument("--cam-dist", type=float, default=None, help="camera distance from the origin (default: the bounds' diagonal)")
    ap.add_argument("--aa", type=int, default=3, help="aa x aa samples per pixel (1 .. 8)")
    ap.add_argument("--interpreter", action="store_true", help="skip the per-tree kernel build")
    ap.add_argument("-o", "--output", default=None)
    args = ap.parse_args(argv)

    import numpy as np
    from gsdf_amd import hip
    from scaffold.builder import Builder

    hip.init(0)
    t0 = time.perf_counter()
    sdf = hip.SDF3HIP(Builder().Scene(args.scene))
    if not args.interpreter:
        sdf.specialize()
    t1 = time.perf_counter()
    rgba, depth, evals = sdf.render_view(args.width, args.height, yaw=args.yaw, pitch=args.pitch, cam_dist=args.cam_dist, aa=args.aa)
    t2 = time.perf_counter()
    out = args.output or f"{args.scene}.png"
    write_png(out, rgba)
    print(f"{args.scene} {args.width}x{args.height} aa {args.aa}: {np.isfinite(depth).mean() * 100:.1f} % of pixels hit, "
          f"{int(evals.astype(np.int64).sum())} evaluations; setup {t1 - t0:.2f} s, frame {(t2 - t1) * 1e3:.1f} ms "
          f"(first frame: includes the view kernel's build); written to {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
