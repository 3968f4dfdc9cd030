#!/usr/bin/env python3
"""The reference's 2-D pictures, rendered on the GPU: gsdfaux.RenderPNGFile (gsdfaux/gsdfaux.go:264-296) with its colour
conversions (gsdfaux/color.go), written as a PNG:

    python examples/render_png.py image -o image.png                  # examples/image: circle and triangle, 1080 rows, IQ colours
    python examples/render_png.py text --color bw -o text.png         # examples/image-text: "Abc123~", anti-aliased black on white
    python examples/render_png.py thread -o thread.png                # examples/fibonacci-showerhead: the thread profile (thread.png)

The width follows from the part's bounds and --height, as RenderPNGFile sizes it. --color picks the conversion: iq (RenderPNGFile's
default, ColorConversionInigoQuilez of the bounds' diagonal / 3), bw (ColorConversionLinearGradient(height of the part / 1000,
color.Black, color.White), as examples/image-text), gradient (the same length from a dark red to a light blue) or default
(ImageRendererSDF2's own black / white / red). Without --color each scene uses what its reference program passes. The PNG is
written with the standard library only (zlib, struct)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# scene -> (RenderPNGFile's picHeight, the conversion its reference program passes)
SCENES = {"image": (1080, "iq"), "text": (300, "bw"), "thread": (512, "iq")}


def scene(name):
    """The reference program's 2-D shape, built by the scaffold's Builder."""
    import numpy as np
    from scaffold.builder import Builder
    b = Builder()
    if name == "image":  # examples/image/image.go:17-27
        dim = 20.0
        return b.Union2D(b.NewCircle(dim), b.NewPolygon([(dim, 0), (3 * dim, dim), (3 * dim, -dim)]))
    if name == "text":  # examples/image-text: textsdf.Font over the ISO 3098 face, RelativeGlyphTolerance 0.001
        ttf = open(os.path.join(ROOT, "tests", "golden", "iso-3098.ttf"), "rb").read()
        return b.TextLine(ttf, "Abc123~", 0.001)
    if name == "thread":  # examples/fibonacci-showerhead: threads.PlasticButtress{D: 65, P: 5.0 / 3}.Thread
        return b._call("threads.PlasticButtress.Thread", [65.0, float(np.float32(5.0 / 3.0))])
    raise ValueError(name)


def conversion(hip, kind, bounds):
    import numpy as np
    bb = np.asarray(bounds, np.float32)
    edge = np.float32(np.float32(bb[4] - bb[1]) / np.float32(1000))  # image-text: charHeight / 1000
    if kind == "iq":
        return hip.color_iq(bb)
    if kind == "bw":
        return hip.color_gradient(edge)
    if kind == "gradient":
        return hip.color_gradient(edge * np.float32(20), (120, 10, 20, 255), (150, 200, 255, 255))
    return hip.color_default()


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("scene", choices=sorted(SCENES))
    ap.add_argument("--height", type=int, default=None, help="picture rows (default: the reference program's)")
    ap.add_argument("--color", choices=["iq", "gradient", "bw", "default"], default=None)
    ap.add_argument("--interpreter", action="store_true", help="skip the per-tree kernel build")
    ap.add_argument("-o", "--output", default=None)
    args = ap.parse_args(argv)

    from gsdf_amd import hip, png

    hip.init(0)
    height, kind = SCENES[args.scene]
    height = args.height or height
    kind = args.color or kind
    t0 = time.perf_counter()
    sdf = hip.SDF2HIP(scene(args.scene))
    if not args.interpreter:
        sdf.specialize()
    t1 = time.perf_counter()
    bb = sdf.Bounds()
    w = hip.picture_size(bb, height)
    rgba, _ = sdf.render_picture(w, height, conversion(hip, kind, bb))
    t2 = time.perf_counter()
    out = args.output or f"{args.scene}.png"
    png.write_png(out, rgba)
    print(f"{args.scene} {w}x{height} ({kind}): setup {t1 - t0:.2f} s, picture {(t2 - t1) * 1e3:.1f} ms (first picture: includes "
          f"the kernel's build); written to {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
