"""The CPU twin of the loops' offset (tests/offsetref.py; include/gsdf_hip.h, section "contours: offset") held to closed forms and to
the facts the contract derives: no GPU. The device is held to the twin, to the byte, in tests/test_gpu_offset.py."""
import math

import numpy as np
import pytest

import contourref as R
import contoursimpref as S
import hatchref as H
import offsetref as O

F = np.float32
RECT = [(2, 1), (6, 1), (6, 3), (2, 3)]


def rect():
    return S.pack([np.array(RECT, F)])


def annulus():
    return S.pack(H.annulus())


def moved_polygon(n, r, d):
    """(area, perimeter) of the regular n-gon of circumradius r with its boundary moved by the distance d, inwards for d > 0 (the
    n-gon of the apothem less d), outwards for d < 0 (the sides moved out, the corners rounded: A + P |d| + pi d^2)."""
    apothem, tan = r * math.cos(math.pi / n), math.tan(math.pi / n)
    if d >= 0:
        p = apothem - d
        return n * p * p * tan, 2 * n * p * tan
    area, length = n * apothem * apothem * tan, 2 * n * apothem * tan
    return area + length * -d + math.pi * d * d, length + 2 * math.pi * -d


def source_edges(c, layer):
    a, b = O.layer_edges(c, layer)
    return a, b


def test_the_rectangle_s_closed_forms():
    o = O.offset(rect(), 0.5, [0.5])
    assert o.xy.tolist() == [[3, 1.5], [3.5, 1.5], [4, 1.5], [4.5, 1.5], [5, 1.5], [5.5, 2], [5, 2.5], [4.5, 2.5], [4, 2.5], [3.5, 2.5], [3, 2.5], [2.5, 2]]
    assert o.loop_start.tolist() == [0, 12] and o.loop_layer.tolist() == [0] and R.area(o.xy) == 2.5
    R.check_structure(o)
    o = O.offset(rect(), 0.5, [0.25])
    assert o.stats["n_loops"] == 1 and R.area(o.xy) == 5.125
    for inset in (1.0, 1.25):  # the field is exactly 0 on the medial line, and zero is outside
        o = O.offset(rect(), 0.5, [inset])
        assert o.stats["n_loops"] == 0 and o.stats["n_verts"] == 0 and o.loop_start.tolist() == [0]
    D = O.distance(rect(), 0.5, [1.0], 0)
    assert D[3, 2:9].tolist() == [-0.5, -1, -1, -1, -1, -1, -0.5] and (D[3] + F(1.0) >= 0).all()
    o = O.offset(rect(), 0.5, [-0.5])
    assert o.stats["n_loops"] == 1 and R.area(o.xy) == 14.5
    assert o.stats["nx"] == 14 and o.stats["ny"] == 10 and o.stats["x0"] == 1.0 and o.stats["y0"] == 0.0 and o.stats["band"] == 1.5


@pytest.mark.parametrize("res,n_verts,fragments", [(0.25, 442, 60), (0.5, 218, 24)])
def test_the_annulus_s_closed_forms(res, n_verts, fragments):
    c = annulus()
    for inset in (0.0, 0.5, 1.0, -1.0):
        o = O.offset(c, res, [inset])
        assert (o.stats["n_loops"], o.stats["n_verts"]) == (2, n_verts), inset
        R.check_structure(o)
        # |area - analytic| <= res x perimeter of the exact offset curves: every vertex lies within res of its curve (the contract's
        # vertex bound), so the region between the traced and the exact curve is inside a strip of half-width res along the exact one
        area, length = 0.0, 0.0
        for n, r, sign, d in ((90, 10.0, 1.0, inset), (40, 4.0, -1.0, -inset)):   # d > 0 moves this polygon's boundary inwards
            area_d, length_d = moved_polygon(n, r, d)
            area += sign * area_d
            length += length_d
        got = float(sum(R.area(l) for l in o.loops()))
        assert abs(got - area) <= res * length, (inset, got, area, res * length)
    assert O.offset(c, res, [3.1]).stats["n_loops"] == 0
    assert O.offset(c, res, [2.9]).stats["n_loops"] == fragments  # a remainder thinner than res fragments; not an error


# every closed-form case above as the call of its own that it is there (band = |inset| + 2 res: the clamp as tight as it gets), the
# hand loops, and calls of several insets
CASES = ([(rect, 0.5, (inset,)) for inset in (0.5, 0.25, 1.0, 1.25, -0.5)] +
         [(annulus, res, (inset,)) for res in (0.25, 0.5) for inset in (0.0, 0.5, 1.0, -1.0, 3.1, 2.9)] +
         [(H.hand_loops, 0.25, (0.3,)), (rect, 0.5, (0.5, 0.25, 1.0, 1.25)), (annulus, 0.25, (0.0, 0.5, 1.0, -1.0)), (annulus, 0.5, (3.1, 2.9))])


@pytest.fixture(scope="module")
def results():
    return [(make(), res, insets, O.offset(make(), res, insets)) for make, res, insets in CASES]


def test_the_clamp_changes_no_loop(results):
    for c, res, insets, o in results:
        O.same_bytes(O.offset(c, res, insets, clamp=False), o)


def test_every_vertex_keeps_its_distance(results):
    """| dist(v, source loops) - |inset| | <= res plus rounding, against an independent float64 distance (contoursimpref.seg_dist)."""
    seen = 0
    for c, res, insets, o in results:
        K = len(insets)
        for q in range(len(o.loop_layer)):
            l, i = divmod(int(o.loop_layer[q]), K)
            a, b = source_edges(c, l)
            d = S.seg_dist(o.xy[o.loop_start[q]:o.loop_start[q + 1]], a, b)
            assert (np.abs(d - abs(float(F(insets[i])))) <= res * (1 + 1e-6)).all(), (l, i, float(np.abs(d - abs(insets[i])).max()))
            seen += len(d)
    assert seen > 3000


def test_layers_are_numbered_l_n_plus_i_and_an_empty_layer_stays_empty():
    c = H.hand_loops()
    insets = (-0.4, 0.0, 0.5, 1.0)
    o = O.offset(c, 0.25, insets)
    assert o.n_layers == 20 and o.stats["n_layers_in"] == 5 and o.stats["n_insets"] == 4
    assert (np.diff(o.loop_layer.astype(np.int64)) >= 0).all()
    assert not set(o.loop_layer.tolist()) & {12, 13, 14, 15}          # input layer 3 has no loops
    assert (o.D[3] == o.band).all() and o.band == F(F(1.0) + F(0.5))
    # the layers' areas shrink with the inset
    area = [sum(R.area(l) for l in o.loops(k)) for k in range(20)]
    for l in (0, 1, 2, 4):
        assert area[4 * l] > area[4 * l + 1] > area[4 * l + 2] > area[4 * l + 3] > 0
    R.check_structure(o)


def test_an_inset_of_a_call_is_that_inset_alone_when_the_lattice_is_the_same():
    c = annulus()
    both = O.offset(c, 0.5, (0.5, 1.0))
    for i, inset in enumerate((0.5, 1.0)):
        one = O.offset(c, 0.5, (inset,))
        assert [l.tolist() for l in both.loops(i)] == [l.tolist() for l in one.loops()]


@pytest.mark.parametrize("k", [40, -40])
def test_scaling_by_a_power_of_two_scales_the_result_exactly(k):
    c = H.hand_loops()
    insets = np.array((0.3, -0.4), F)
    o = O.offset(c, 0.25, insets)
    s = O.offset(O.scaled(c, k), np.ldexp(F(0.25), k), np.ldexp(insets, k).astype(F))
    assert s.loop_start.tolist() == o.loop_start.tolist() and s.loop_layer.tolist() == o.loop_layer.tolist() and (s.keys == o.keys).all()
    assert (s.xy.view(np.uint32) == np.ldexp(o.xy, k).astype(F).view(np.uint32)).all()
    for a, b in zip(s.D, o.D):
        assert (a.view(np.uint32) == np.ldexp(b, k).astype(F).view(np.uint32)).all()
    assert {x: s.stats[x] for x in ("n_verts", "n_loops", "inside_nodes", "band_nodes", "nx", "ny")} == {x: o.stats[x] for x in ("n_verts", "n_loops", "inside_nodes", "band_nodes", "nx", "ny")}


def test_arguments_and_a_handle_without_loops():
    c = rect()
    for res, insets in ((0.0, [0.5]), (math.nan, [0.5]), (0.5, []), (0.5, [0.1] * 9), (0.5, [math.inf]), (0.5, [math.nan]), (1e-12, [0.5])):
        with pytest.raises(ValueError):
            O.offset(c, res, insets)
    with pytest.raises(ValueError):
        O.distance(c, 0.5, [0.5], 1)
    empty = S.Loops(np.zeros((0, 2), F), [0], n_layers=2)
    o = O.offset(empty, 0.5, [0.5, -1.0])
    assert o.n_layers == 4 and o.stats["n_loops"] == 0 and o.loop_start.tolist() == [0] and o.stats["nx"] == 8 and (o.D[1] == F(2.0)).all()
    assert len(O.stats_bytes(o.stats)) == 80
