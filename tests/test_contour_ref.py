"""The contour tracer's CPU twin (tests/contourref.py, written from the "contours" section of include/gsdf_hip.h) over the oracle:
the properties the contract promises -- succ a permutation of exactly the cut edges, leaders on axis-1 edges, nothing forced outside
on the corpus, orientation -- the two saddle cases by count, a circle's area and perimeter, a flange slice with its hole, and
independence of the order the lattice is evaluated in."""
import math

import numpy as np
import pytest

import contourref
from contourref import check_structure, res_for, saddle_shape
import corpus
from oracle.oracle import OracleSDF
from scaffold.builder import Builder

F = np.float32


def test_corpus_structure():
    _, shapes = corpus.shapes2d()
    assert len(shapes) == 44
    empty = []
    for name, s in shapes:
        t = s.tree()
        o = OracleSDF(t)
        c = contourref.contour(o.Evaluate, o.Bounds(), res_for(o.Bounds(), 40))
        check_structure(c)
        assert c.stats["border_inside"] == 0, name
        assert 20 <= max(c.stats["nx"], c.stats["ny"]) <= 48 or name == "intersect2d", (name, c.stats)
        if c.stats["n_loops"]:
            assert c.areas().sum() > 0, name
        else:
            empty.append(name)
    # the disjoint intersection (empty bounds: a 4 x 4 lattice) has no loops; that is not an error
    assert "intersect2d" in empty, empty


def test_empty_bounds_and_no_inside_node():
    b = Builder()
    s = b.Intersection2D(b.Translate2D(b.NewCircle(0.4), 0.45, 1), b.NewRectangle(1, 0.61))
    o = OracleSDF(s.tree())
    c = contourref.contour(o.Evaluate, o.Bounds(), F(0.1))
    assert (c.stats["nx"], c.stats["ny"], c.stats["n_loops"], c.stats["n_verts"], c.stats["rank_rounds"]) == (4, 4, 0, 0, 0)
    assert c.loop_start.tolist() == [0]
    # a part smaller than a cell that no node falls into (the nodes next to it are the corners of its bounding box): no loops
    thin = b.Translate2D(b.NewCircle(0.01), 0.013, 0.0171)
    o = OracleSDF(thin.tree())
    c = contourref.contour(o.Evaluate, o.Bounds(), F(0.05))
    assert (o.Bounds()[3:5] > o.Bounds()[0:2]).all() and c.stats["n_loops"] == 0 and not any(l.cut.any() for l in c.layers)


@pytest.mark.parametrize("like, case", [(True, 5), (False, 10)])
def test_saddles(like, case):
    s = saddle_shape(Builder(), like)
    o = OracleSDF(s.tree())
    c = contourref.contour(o.Evaluate, o.Bounds(), F(0.3))
    check_structure(c)
    counts = c.layers[0].case_counts
    assert counts[case] == 1 and counts[15 - case] == 0, counts.tolist()
    assert c.stats["saddle_cells"] == 1
    assert c.stats["n_loops"] == 2 and (c.areas() > 0).all()  # the inside corners of a saddle are never joined: two outer loops


@pytest.mark.parametrize("div", [16, 64, 256])
def test_circle_area_and_perimeter(div):
    s = Builder().NewCircle(1.0)
    o = OracleSDF(s.tree())
    res = F(2.0 / div)
    c = contourref.contour(o.Evaluate, o.Bounds(), res)
    check_structure(c)
    assert c.stats["n_loops"] == 1
    loop = c.loops()[0]
    bound = float(res) ** 2  # (res / r)^2 with r = 1; a chord polygon's deficit is about a sixth of it
    ea, ep = abs(contourref.area(loop) / math.pi - 1), abs(contourref.perimeter(loop) / (2 * math.pi) - 1)
    print(f"circle res 2/{div}: area error {ea:.3g}, perimeter error {ep:.3g}, bound {bound:.3g}")
    assert ea < bound and ep < bound
    r = np.hypot(loop[:, 0].astype(np.float64), loop[:, 1].astype(np.float64))
    # linear interpolation along an edge misses the field by at most res^2 / 8 times its curvature, 1 / (1 - res) at worst
    assert np.abs(r - 1).max() < float(res) ** 2 / (8 * (1 - float(res))) + 1e-6


def flange_slice():
    s = Builder().Scene("npt-flange")
    bb = s.Bounds()
    res = F(float(s.Diagonal()) / 60)
    z = F((F(bb[2]) + F(bb[5])) * F(0.5))
    return s, res, np.array([z], F)


def test_flange_slice_has_a_hole():
    s, res, z = flange_slice()
    o = OracleSDF(s.tree())
    c = contourref.contour(o.Evaluate, o.Bounds(), res, z)
    check_structure(c)
    a = c.areas()
    assert len(a) == 2 and (a > 0).sum() == 1 and (a < 0).sum() == 1 and a.sum() > 0, a
    assert sorted(np.diff(c.loop_start.astype(np.int64)).tolist()) == [52, 84]
    assert c.stats["border_inside"] == 0 and c.stats["evals"] == c.stats["nx"] * c.stats["ny"]


def test_evaluation_order_does_not_matter():
    s, res, _ = flange_slice()
    o = OracleSDF(s.tree())
    z = contourref.layer_heights(o.Bounds(), F(float(o.Bounds()[5] - o.Bounds()[2]) / 3))
    a = contourref.contour(o.Evaluate, o.Bounds(), res, z)
    nx, ny = a.stats["nx"], a.stats["ny"]
    perm = np.random.default_rng(5).permutation(nx * ny)
    b = contourref.contour(o.Evaluate, o.Bounds(), res, z, order=perm)
    assert a.stats == b.stats and a.stats["n_layers"] == len(z) >= 3
    for f in ("xy", "keys", "loop_start", "loop_layer"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f


def test_layer_heights_match_the_library():
    from gsdf_amd import hip
    bb = Builder().Scene("bolt").Bounds()
    for h in (0.37, float(bb[5] - bb[2]) / 7, float(bb[5] - bb[2])):
        a, b = hip.layer_heights(bb, h), contourref.layer_heights(bb, h)
        assert a.dtype == np.float32 and a.tobytes() == b.tobytes() and len(a) >= 1
        assert a[0] == F(F(bb[2]) + F(F(0.5) * F(h))) and (a < bb[5]).all() and F(a[-1] + F(h)) >= bb[5]
    assert len(hip.layer_heights(bb, 4 * float(bb[5] - bb[2]))) == 0  # the first mid-height is already above the part
