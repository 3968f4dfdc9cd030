"""Trees with degenerate parameters, which the reference's constructors would refuse (tests/test_gpu_nan.py states what the device
may do with them): built with legal parameters, then edited in a copy of the blob. [(name, tree)]"""
from scaffold.builder import Builder
from tree_edit import clone, first


def degenerate_trees():
    b = Builder()
    out = []
    # polygon with a repeated vertex: an edge of length zero, 0 / 0 in its projection (cpu_evaluators.go:803-806)
    t = clone(b.Union(b.Extrude(b.NewPolygon([(0, 0), (2, 0), (2, 1), (1, 1.5), (0, 1)]), 1.0), b.Translate(b.NewSphere(0.4), 1, 1, 0.6)).tree())
    n = t.nodes[first(t, "POLY2D")]
    t.aux[n.aux_off + 4], t.aux[n.aux_off + 5] = t.aux[n.aux_off + 2], t.aux[n.aux_off + 3]
    out.append(("polygon-repeated-vertex", t))
    # line whose ends coincide (NewLine2D turns it into a circle, primitives2d.go:24-29; the node itself divides by 0)
    t = clone(b.Extrude(b.NewLine2D(0.2, 0.1, 1.0, 0.5, 0.2), 0.5).tree())
    n = t.nodes[first(t, "LINE2D")]
    n.p[2], n.p[3] = n.p[0], n.p[1]
    out.append(("line-of-length-zero", t))
    # blend width zero: (b - a) / 0 is NaN where the two fields are equal, +-Inf elsewhere
    for name, mk in (("smooth-union-k0", b.SmoothUnion), ("smooth-diff-k0", b.SmoothDifference), ("smooth-intersect-k0", b.SmoothIntersect)):
        t = clone(mk(0.1, b.NewSphere(1.0), b.Translate(b.NewSphere(1.0), 1.0, 0, 0)).tree())
        t.nodes[t.root].p[0] = 0.0
        out.append((name, t))
    # scale by zero: positions times Inf (NaN on the axis planes), distance times 0
    t = clone(b.Union(b.Scale(b.NewBox(1, 1, 1, 0.1), 2.0), b.Translate(b.NewSphere(0.5), 2, 0, 0)).tree())
    t.nodes[first(t, "SCALE")].p[0] = 0.0
    out.append(("scale-zero", t))
    # an "ellipse" with equal axes: l = b^2 - a^2 = 0 (cpu_evaluators.go:759-762)
    t = clone(b.Extrude(b.NewEllipse(1.0, 0.5), 0.4).tree())
    n = t.nodes[first(t, "ELLIPSE2D")]
    n.p[1] = n.p[0]
    out.append(("ellipse-circle", t))
    # bezier whose control point is the midpoint of its chord: kk = 1 / 0 (cpu_evaluators.go:585-593)
    t = clone(b.Extrude(b.NewQuadraticBezier2D((0, 0), (1, 1.5), (2, 0), 0.1), 0.4).tree())
    n = t.nodes[first(t, "QUADBEZIER2D")]
    n.p[2], n.p[3] = 1.0, 0.0
    out.append(("bezier-straight", t))
    # shell of thickness zero: positions times Inf
    t = clone(b.Shell(b.NewBox(1, 1, 1, 0.1), 0.1).tree())
    t.nodes[first(t, "SHELL")].p[0] = 0.0
    out.append(("shell-zero", t))
    return out
