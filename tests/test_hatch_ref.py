"""The CPU twin of the hatch fill (tests/hatchref.py) against what the contract must MEAN (include/gsdf_hip.h, "contours: hatch
fill"), not against itself: even crossings on every line, segments inside and gaps outside under an independent point-in-polygon
test, the Riemann-sum bound on spacing x length against the loops' area, a closed form, the symmetry under a reversed direction, the
argument checks; and the Python layouts of the records against the header's sizes. No GPU."""
import ctypes as C
import math

import numpy as np
import pytest

import contoursimpref as S
import hatchref as H

F = np.float32


def layer_loops(c, layer):
    return [l for l, q in zip(c.loops(), c.loop_layer) if q == layer]


def test_every_line_has_an_even_number_of_crossings():
    """Also with lines through the rectangle's lattice vertices and along its sides (0 / 90 degrees, spacing 0.125, offset 0: the
    sides y = 0 and y = 5.125, x = 0 and x = 4.625 are lines); t stays within [-0.0, 1.0]."""
    nested = S.pack(H.annulus() + [S.rectangle(37, 41)], [0, 0, 1], 2)
    for c, spacings in ((S.mixed_loops(300, 3), (0.125, 0.5, 3.0)), (nested, (0.125, 0.5, 3.0)), (H.hand_loops(), (0.125,))):
        for angles in ((45.0, 135.0), (0.0, 90.0)):
            for sp in spacings:
                h = H.hatch(c, sp, H.directions(angles))
                assert h.stats["n_crossings"] > 0 and (h.line_counts % 2 == 0).all(), (angles, sp)
                assert h.t.min() >= 0.0 and h.t.max() <= 1.0, (angles, sp, h.t.min(), h.t.max())
                assert 2 * h.stats["n_segments"] == h.stats["n_crossings"] == int(h.line_counts.sum())
                assert h.layer_start[0] == 0 and h.layer_start[-1] == len(h.seg) and (np.diff(h.layer_start.astype(np.int64)) >= 0).all()
    assert h.stats["max_line_crossings"] <= 58      # (what the prototype of the contract saw on these inputs)


def test_lines_along_the_sides_of_the_lattice_rectangle():
    """A vertex on a line counts as above it and an edge on a line does not cross it: of the two horizontal sides only the upper one
    comes out as a segment, and it is the last line of the layer."""
    c = S.pack([S.rectangle(37, 41)])
    h = H.hatch(c, 0.125, [(1.0, 0.0)])
    assert (h.layers[0]["k_min"], h.layers[0]["k_max"]) == (1, 41) and h.stats["n_segments"] == 41
    assert h.seg[-1].tolist() == [0.0, 5.125, 4.625, 5.125] and h.seg[0].tolist() == [0.0, 0.125, 4.625, 0.125]


def test_segments_are_inside_and_gaps_outside():
    """Midpoints of the segments longer than 1e-3 are inside under even-odd ray casting, midpoints of the gaps between the segments
    of one line are outside. The offset keeps every line off the lattice vertices: a segment along a side has its midpoint ON the
    boundary, where the independent test says nothing."""
    c = H.hand_loops()
    seen = 0
    for angles in ((45.0, 135.0), (0.0, 90.0), (17.0,)):
        for sp in (0.125, 0.5, 3.0):
            h = H.hatch(c, sp, H.directions(angles), 0.0437)
            for l in range(c.n_layers):
                seg, k = h.segments(l).astype(np.float64), h.line[h.layer_start[l]:h.layer_start[l + 1]]
                if not len(seg):
                    continue
                loops = layer_loops(c, l)
                long_ = np.hypot(seg[:, 2] - seg[:, 0], seg[:, 3] - seg[:, 1]) > 1e-3
                mid = 0.5 * (seg[:, :2] + seg[:, 2:])
                assert H.inside_even_odd(mid[long_], loops).all(), (angles, sp, l)
                same = k[1:] == k[:-1]
                gap_a, gap_b = seg[:-1, 2:][same], seg[1:, :2][same]
                wide = np.hypot(*(gap_b - gap_a).T) > 1e-3
                assert not H.inside_even_odd(0.5 * (gap_a + gap_b)[wide], loops).any(), (angles, sp, l)
                seen += int(long_.sum()) + int(wide.sum())
    assert seen > 1500


def test_spacing_times_length_is_the_area_within_spacing_times_perimeter():
    """Properly nested loops only. The Riemann sum of the chord length over lines `spacing` apart has total variation at most the
    perimeter: |spacing length_l - area_l| <= spacing perimeter_l; 1e-6 covers |dir| differing from 1 by float32 rounding."""
    c = H.hand_loops()
    _, layers = S.measures(c)
    for angles in ((45.0, 135.0), (0.0, 90.0), (17.0, 73.0, 121.0)):
        for sp in (0.125, 0.5, 3.0):
            h = H.hatch(c, sp, H.directions(angles))
            for l in range(c.n_layers):
                got, area, per = sp * float(h.layers[l]["length"]), float(layers[l]["area"]), float(layers[l]["length"])
                assert abs(got - area) <= sp * per * (1 + 1e-6), (angles, sp, l, got, area, per)
            assert h.stats["length"] == pytest.approx(float(h.layers["length"].sum()), rel=1e-12)
    assert h.layers[3].tolist() == (0.0, 0, 0, -1)              # the empty layer


def test_a_dyadic_rectangle_in_closed_form():
    """[2, 6] x [1, 3], lines y = k / 2 along +x: crossed iff 1 < c_k <= 3, the end points exact."""
    c = S.pack([np.array([(2, 1), (6, 1), (6, 3), (2, 3)], F)])
    h = H.hatch(c, 0.5, [(1.0, 0.0)])
    want = np.array([(2, y, 6, y) for y in (1.5, 2.0, 2.5, 3.0)], F)
    assert h.seg.tobytes() == want.tobytes() and h.line.tolist() == [3, 4, 5, 6] and h.layer_start.tolist() == [0, 4]
    assert h.layers[0].tolist() == (16.0, 4, 3, 6) and h.stats["length"] == 16.0 and h.stats["zero_length"] == 0
    assert h.stats["n_lines"] == 4 and h.stats["max_line_crossings"] == 2
    # along +y, offset 0.25: s = -x, lines -x = 0.25 + k / 2
    h = H.hatch(c, 0.5, [(0.0, 1.0)], 0.25)
    xs = [-(0.25 + 0.5 * k) for k in range(-12, -4)]
    assert h.line.tolist() == list(range(-12, -4)) and h.seg.tobytes() == np.array([(x, 1, x, 3) for x in xs], F).tobytes()
    assert h.layers[0]["length"] == 16.0


def test_a_reversed_direction_gives_the_same_end_points():
    """(-dx, -dy) with -offset: s, u and c change sign exactly, line k becomes line -k, t is the same number, so every end point has
    the same bits and every segment runs the other way. (With a vertex exactly ON a line the two differ, by the rule that such a
    vertex is above: the offset here keeps the lines off the vertices.)"""
    c = H.hand_loops()
    for angles in ((45.0, 135.0), (0.0, 90.0), (17.0, 73.0, 121.0)):
        d = H.directions(angles)
        a, b = H.hatch(c, 0.5, d, 0.0437), H.hatch(c, 0.5, -d, -0.0437)
        assert a.layer_start.tolist() == b.layer_start.tolist() and a.stats["n_segments"] > 100
        for l in range(c.n_layers):
            sa = a.segments(l).view(np.uint64).reshape(-1, 2)
            sb = b.segments(l).view(np.uint64).reshape(-1, 2)[:, ::-1]
            assert sorted(map(tuple, sa.tolist())) == sorted(map(tuple, sb.tolist())), (angles, l)
            assert a.layers[l]["length"] == b.layers[l]["length"]


def test_ties_in_u_are_broken_by_the_tail():
    """Where two teeth of the comb touch, two crossings of a line share u_c: the lower vertex number comes first, so the zero-length
    pair never forms and every tooth gives its own segment."""
    c = H.comb(40)
    h = H.hatch(c, 0.25, [(1.0, 0.0)], 0.125)
    assert h.stats["max_line_crossings"] == 80 and h.stats["zero_length"] == 0 and h.stats["n_segments"] == 40 * 12
    assert (h.seg[:, 2] - h.seg[:, 0] == 0.5).all() and h.layers[0]["length"] == 40 * 12 * 0.5


def test_argument_checks():
    c = S.pack([S.circle(40)])
    d = [(1.0, 0.0)]
    for sp in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError):
            H.hatch(c, sp, d)
    for off in (math.nan, math.inf, -math.inf):
        with pytest.raises(ValueError):
            H.hatch(c, 1.0, d, off)
    for dirs in ([], [(1, 0)] * 5, [(0.0, 0.0)], [(1.5, 0.0)], [(0.0, -1.25)], [(math.nan, 0.0)], [(1.0, 0.0), (0.0, math.inf)]):
        with pytest.raises(ValueError):
            H.hatch(c, 1.0, dirs)
    # e = 4 for a circle of radius 10 about (3, -2): 2^5 / spacing >= 2^29 from spacing = 2^-24 down
    with pytest.raises(ValueError, match="too small"):
        H.hatch(c, 2.0 ** -24, d)
    with pytest.raises(ValueError, match="too small"):
        H.hatch(c, 1.0, d, 2.0 ** 29)
    assert H.hatch(c, 1.0, d, 2.0 ** 28).stats["n_segments"] == 20      # y runs from -12 to 8: the lines y = -11 .. 8
    # no loops: no segments
    empty = S.Loops(np.zeros((0, 2), F), [0], n_layers=2)
    h = H.hatch(empty, 1.0, d)
    assert h.stats["n_segments"] == 0 and h.layer_start.tolist() == [0, 0, 0] and h.layers.tolist() == [(0.0, 0, 0, -1)] * 2


def test_the_python_records_have_the_header_s_layout():
    from gsdf_amd import hip
    assert C.sizeof(hip.HatchOpts) == 48 and hip.HatchOpts.dir.offset == 16 and hip.HatchOpts.dry.offset == 12
    assert C.sizeof(hip.HatchLayer) == 24 == hip.HATCH_LAYER_DTYPE.itemsize == H.LAYER_DTYPE.itemsize and hip.HATCH_LAYER_DTYPE == H.LAYER_DTYPE
    assert C.sizeof(hip.HatchStats) == 64 and hip.HatchStats.ms_device.offset == 56 == hip.HatchStats.RESULT_BYTES and hip.HatchStats.length.offset == 48
    for s in ("gsdf_hip_contour_hatch", "gsdf_hip_hatch_counts", "gsdf_hip_hatch_read", "gsdf_hip_hatch_destroy"):
        assert s in hip.SYMBOLS
