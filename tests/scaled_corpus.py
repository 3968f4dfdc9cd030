"""The shape corpus with a unit: tests/corpus.py's shapes with every length multiplied by u.

shapes3d(b, u) and shapes2d(b, u) keep corpus.py's names, its argument values at u = 1 (the random draws are taken in the same order,
so the base rung IS the existing corpus: tests/test_scale_ref.py compares the lowered programs) and scale what is a length: radii,
sizes, roundings, offsets, translations, array pitches, smoothing widths, thread diameter / pitch / length, polygon vertices. What is
no length stays: angles, counts, rotation axes, Scale's factor. A twist's rate is an angle per length: divided by u. With u a power
of two every scaled argument is the exact float32 multiple of the base argument, and the reference's evaluators are then homogeneous
bit for bit: f_u(u p) = u f_1(p) (tests/test_scale_ref.py states over which u).

Left out, each for a cause:
  shell             Shell(s, t) evaluates t * (|s(p / t)| - t) (the reference's operations.go:749-754): the thickness is a length and
                    a dimensionless zoom of the child at once, so no scaling of its arguments makes the node homogeneous.
  screw_npt         threads.NPT reads a table of nominal pipe sizes (npt.go:65-71): the builder refuses any other size.
  nut_hex, nut_knurl  threads.ISO takes the hex flat-to-flat distance from a table of millimetre sizes (threads.go:225-251, metricf2f):
                    the head does not scale with D.
  scene_*           the benchmark scenes take no unit: their dimensions are constants of the scaffold (scaffold/threads.hpp).
  (the text plates) glyph outlines are in font units scaled by a size the plate fixes; scene_glyph_plate is one of the scenes.
"""
import math

import numpy as np

from scaffold.builder import Builder

LEFT_OUT_3D = ("shell", "screw_npt", "nut_hex", "nut_knurl", "scene_npt_flange", "scene_bolt", "scene_knurled_cylinder", "scene_glyph_plate")


def _rng():
    return np.random.default_rng(1)


def _f(rng):
    return float(np.float32(rng.random()))


def unit(k):
    """2^k as a Python float (exact)."""
    return math.ldexp(1.0, k)


def shapes3d(bld=None, u=1.0):
    b = bld or Builder()
    rng = _rng()
    out = []
    maxdim = 1.0
    dv = (maxdim * u, maxdim * 0.47 * u, maxdim * 0.8 * u)
    thick = maxdim / 10 * u
    out += [("sphere", b.NewSphere(1 * u)), ("box", b.NewBox(dv[0], dv[1], dv[2], thick)),
            ("boxframe", b.NewBoxFrame(dv[0], dv[1], dv[2], thick)), ("cyl0", b.NewCylinder(dv[0], dv[1], 0)),
            ("cylr", b.NewCylinder(dv[0], dv[1], thick)), ("hexprism", b.NewHexagonalPrism(dv[0], dv[1])),
            ("torus", b.NewTorus(dv[0], dv[1])), ("triprism", b.NewTriangularPrism(1 * u, 0.5 * u))]
    s1 = b.NewSphere(1 * u)
    s2 = b.Translate(b.NewBox(1 * u, 0.6 * u, .8 * u, 0.1 * u), 0.5 * u, 0.7 * u, 0.8 * u)
    out += [("union", b.Union(s1, s2)), ("diff", b.Difference(s1, s2)), ("intersect", b.Intersection(s1, s2)),
            ("xor", b.Xor(s1, s2)), ("smoothunion", b.SmoothUnion(0.1 * u, s1, s2)),
            ("smoothdiff", b.SmoothDifference(0.1 * u, s1, s2)), ("smoothintersect", b.SmoothIntersect(0.1 * u, s1, s2))]
    out.append(("union3", b.Union(s1, s2, b.Translate(b.NewTorus(1 * u, 0.3 * u), -0.5 * u, 0.2 * u, 0.1 * u))))
    a = b.NewBox(1 * u, 0.61 * u, 0.8 * u, 0.3 * u)
    axis = (0.0, 0.0, 0.0)
    while math.sqrt(sum(x * x for x in axis)) < .5:
        axis = (_f(rng) * 3, _f(rng) * 3, _f(rng) * 3)
    angle = 0.0
    while abs(angle) < 1e-1 or abs(angle) > 1:
        angle = 2 * 3.14159 * (_f(rng) - 0.5)
    out.append(("rotate", b.Rotate(a, angle, axis)))
    bb = Builder().NewBox(1, 0.61, 0.8, 0.3).Bounds()   # the sizes corpus.py derives from: the box's bounds at u = 1
    size = bb[3:] - bb[:3]
    _f(rng)                          # (corpus.py's draw for the shell's thickness)
    out.append(("elongate", b.Elongate(a, 0.3 * _f(rng) * u, 0.3 * _f(rng) * u, 0.3 * _f(rng) * u)))
    mn = float(size.min())
    out.append(("round", b.Offset(a, -(mn / 64 + _f(rng) * (mn / 2 - mn / 64)) * u)))
    out.append(("scale", b.Scale(a, 0.01 + _f(rng) * (3 - 0.01))))
    out.append(("symmetry", b.Symmetry(a, True, False, True)))
    out.append(("symmetry_xyz", b.Symmetry(b.Translate(a, 0.3 * u, 0.2 * u, 0.1 * u), True, True, True)))
    out.append(("translate", b.Translate(a, 1.3 * _f(rng) * u, -0.7 * _f(rng) * u, 0.4 * u)))
    out.append(("array", b.Array(a, (_f(rng) + 0.1) * u, (_f(rng) + 0.1) * u, (_f(rng) + 0.1) * u, 3, 2, 5)))
    for i in range(3):
        div = int(rng.integers(0, 16)) + 3
        n = int(rng.integers(0, div)) + 1
        out.append((f"circarray{i}", b.CircularArray(b.Translate(a, 1.5 * u, 0, 0), n, div)))
    out.append(("twist", b.Twist(a, _f(rng) / u)))
    s2d = b.NewRectangle(1 * u, 0.57 * u)
    out.append(("extrude", b.Extrude(s2d, (0.01 + _f(rng) * 3.99) * u)))
    out.append(("revolve", b.Revolve(s2d, 0)))
    out.append(("revolve_off", b.Revolve(b.Translate2D(b.NewCircle(0.3 * u), 1.0 * u, 0.2 * u), 0.25 * u)))
    out.append(("screw_iso_ext", b.ScrewISO(1 * u, 0.1 * u, True, 2.0 * u)))
    out.append(("hexhead", b.HexHead(2.0 * u, 1.2 * u, True, True)))
    return b, out


def shapes2d(bld=None, u=1.0):
    b = bld or Builder()
    rng = _rng()
    out = []
    maxdim = 1.0
    dv = (maxdim * u, maxdim * 0.47 * u)
    thick = maxdim / 10 * u
    octv = [(math.cos(2 * math.pi * i / 8) * u, math.sin(2 * math.pi * i / 8) * u) for i in range(8)]
    segs = [(octv[i - 1], octv[i]) for i in range(8)]
    poly = b.NewPolygon(octv)
    out += [("circle", b.NewCircle(maxdim * u)), ("line", b.NewLine2D(0, 0, dv[0], dv[1], thick)),
            ("rect", b.NewRectangle(dv[0], dv[1])), ("arc", b.NewArc(dv[0], math.pi / 3, thick)),
            ("hexagon", b.NewHexagon(maxdim * u)), ("eqtri", b.NewEquilateralTriangle(maxdim * u)),
            ("ellipse", b.NewEllipse(1 * u, 2 * u)), ("poly", poly),
            ("poly_selfclosed", b.NewPolygon([(0, 0), (0, 1 * u), (1 * u, 1 * u), (0, 0)])),
            ("lines", b.NewLines2D(segs, 0.1 * u)), ("translatemulti", b.TranslateMulti2D(poly, octv)),
            ("octagon", b.NewOctagon(dv[0])), ("diamond", b.NewDiamond2D(dv[0], dv[1])),
            ("roundedx", b.NewRoundedX(dv[0], thick)),
            ("iso_thread_ext", b.ISOThread(1 * u, 0.1 * u, True)), ("iso_thread_int", b.ISOThread(1 * u, 0.1 * u, False))]
    out.append(("union_lines", b.Union2D(b.NewLine2D(1 * u, 2 * u, 3 * u, 4 * u, 0.5 * u), b.NewLine2D(2 * u, 3 * u, 0, 0, 0.2 * u),
                                          b.NewLine2D(2 * u, 3 * u, 4 * u, 5 * u, 0.2 * u),
                                          b.NewLines2D([((0, 0), (1 * u, 1 * u)), ((2 * u, 2 * u), (3 * u, 1 * u))], 0.5 * u))))
    s2 = b.NewRectangle(1 * u, 0.61 * u)
    s1 = b.Translate2D(b.NewCircle(0.4 * u), 0.45 * u, 1 * u)
    out += [("union2d", b.Union2D(s1, s2)), ("diff2d", b.Difference2D(s1, s2)), ("intersect2d", b.Intersection2D(s1, s2)),
            ("xor2d", b.Xor2D(s1, s2))]
    obj = b.Translate2D(b.NewRectangle(1 * u, 0.61 * u), 2 * u, .3 * u)
    for i in range(3):
        out.append((f"array2d{i}", b.Array2D(obj, (_f(rng) + 0.1) * u, (_f(rng) + 0.1) * u, int(rng.integers(0, 8)) + 1, int(rng.integers(0, 8)) + 1)))
        div = int(rng.integers(0, 16)) + 3
        out.append((f"circarray2d{i}", b.CircularArray2D(obj, int(rng.integers(0, div)) + 1, div)))
        out.append((f"rotate2d{i}", b.Rotate2D(obj, math.pi * _f(rng) + 0.001)))
        out.append((f"annulus{i}", b.Annulus(obj, (_f(rng) + 1e-3) * u)))
        out.append((f"offset2d{i}", b.Offset2D(obj, (_f(rng) - 0.5) * u)))
        out.append((f"scale2d{i}", b.Scale2D(obj, _f(rng) + 1e-2)))
        out.append((f"elongate2d{i}", b.Elongate2D(obj, _f(rng) * u, _f(rng) * u)))
    out.append(("symmetry2d_x", b.Symmetry2D(obj, True, False)))
    out.append(("symmetry2d_xy", b.Symmetry2D(obj, True, True)))
    return b, out


def bezier2d(bld=None, u=1.0):
    b = bld or Builder()
    return b, [("quadbezier", b.NewQuadraticBezier2D((1.0 * u, 0.47 * u), (2.0 * u, 0.47 * u), (1.0 * u, 1.47 * u), 0.1 * u))]


def scaled_points(pos, u):
    """pos * u in float32: exact for a power of two (no subnormals at the units the ladders use)."""
    return np.ascontiguousarray(np.asarray(pos, np.float32) * np.float32(u))


def mesh_shapes(bld=None, u=1.0):
    """The shapes the renderers are held to across units: a difference, the twist, the ISO screw, a circular array and an extruded
    polygon, plus a smooth union (its blend width is a divisor the lowering scales out of the exact-reciprocal range) and the array
    (its seams are cubes the octree must keep)."""
    b = bld or Builder()
    d = dict(shapes3d(b, u)[1])
    octv = [(math.cos(2 * math.pi * i / 8) * u, math.sin(2 * math.pi * i / 8) * u) for i in range(8)]
    names = ("diff", "twist", "screw_iso_ext", "circarray0", "smoothunion", "array")
    return b, [(n, d[n]) for n in names[:4]] + [("extrude_poly", b.Extrude(b.NewPolygon(octv), 0.8 * u))] + [(n, d[n]) for n in names[4:]]
