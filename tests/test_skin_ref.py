"""The CPU twin of the skin classification (tests/skinref.py) against what the contract must MEAN (include/gsdf_hip.h, "contours:
skin classification of the hatch"), not against itself: a closed form, every piece inside its own layer and its class bits what an
independent point-in-polygon test of the neighbouring layers says, agreement with the plain hatch, whole-layer skin, bit-identical
layers without slivers; and the Python layouts of the records against the header's sizes. No GPU."""
import ctypes as C

import numpy as np
import pytest

import contoursimpref as S
import hatchref as H
import skinref as K

F = np.float32
ANGLES = ((45.0, 135.0), (0.0, 90.0), (17.0, 73.0, 121.0))


def layer_loops(c, layer):
    return [l for l, q in zip(c.loops(), c.loop_layer) if q == layer] if 0 <= layer < c.n_layers else []


def test_a_pyramid_of_two_squares_in_closed_form():
    """[0, 8]^2 under [2, 6]^2, lines y = k + 0.5 along +x, below 0, above 1: layer 0 is top skin where layer 1 does not cover it,
    layer 1 (its upper neighbour is missing) top skin throughout."""
    h = K.skin(K.pyramid(), 1.0, [(1.0, 0.0)], 0, 1, 0.5)
    assert (h.stats["n_segments"], h.stats["n_lines"], h.stats["n_crossings"], h.stats["n_own_crossings"]) == (20, 12, 32, 24)
    want, cls, line = [], [], []
    for k in range(8):
        y = k + 0.5
        parts = [(0, 2, 2), (2, 6, 0), (6, 8, 2)] if 2 <= k <= 5 else [(0, 8, 2)]
        want += [(a, y, b, y) for a, b, _ in parts]
        cls += [c for _, _, c in parts]
        line += [k] * len(parts)
    want += [(2, k + 0.5, 6, k + 0.5) for k in range(2, 6)]
    cls += [2] * 4
    line += list(range(2, 6))
    assert h.seg.tobytes() == np.array(want, F).tobytes() and h.cls.tolist() == cls and h.line.tolist() == line
    assert h.layer_start.tolist() == [0, 16, 20] and h.stats["max_line_crossings"] == 4 and h.stats["zero_length"] == 0
    assert h.skin_layers[0]["length"].tolist() == [16.0, 0.0, 48.0, 0.0] and h.skin_layers[0]["n_segments"].tolist() == [4, 0, 12, 0]
    assert h.skin_layers[1]["length"].tolist() == [0.0, 0.0, 16.0, 0.0] and h.layers.tolist() == [(64.0, 16, 0, 7), (16.0, 4, 2, 5)]
    assert h.stats["n_class"] == [4, 0, 16, 0] and h.stats["length"] == [16.0, 0.0, 64.0, 0.0]
    # seen from above: below 1, above 0 -- all of layer 0 is bottom skin (no layer under it), layer 1 rests on layer 0
    h = K.skin(K.pyramid(), 1.0, [(1.0, 0.0)], 1, 0, 0.5)
    assert h.cls.tolist() == [1] * 8 + [0] * 4 and h.stats["n_crossings"] == 16 + 8 + 8


@pytest.mark.parametrize("make", [K.square_stack, H.hand_loops], ids=["squares", "hand_loops"])
def test_pieces_are_inside_and_their_classes_are_what_the_neighbours_say(make):
    """The midpoint of every piece longer than 1e-3 is inside its own layer under even-odd ray casting, and the class bits are what
    the same test says of the layers under and over it. The offset keeps the lines off the vertices."""
    c = make()
    seen = skipped = 0
    for below, above in ((1, 1), (2, 2)):
        for angles in ANGLES:
            h = K.skin(c, 0.5, H.directions(angles), below, above, 0.0437)
            for l in range(c.n_layers):
                seg, cls = h.segments(l).astype(np.float64), h.cls[h.layer_start[l]:h.layer_start[l + 1]]
                long_ = np.hypot(seg[:, 2] - seg[:, 0], seg[:, 3] - seg[:, 1]) > 1e-3
                skipped += int((~long_).sum())
                mid = 0.5 * (seg[:, :2] + seg[:, 2:])[long_]
                if not len(mid):
                    continue
                assert H.inside_even_odd(mid, layer_loops(c, l)).all(), (below, above, angles, l)
                covered = lambda ls: np.logical_and.reduce([H.inside_even_odd(mid, layer_loops(c, m)) if layer_loops(c, m) else np.zeros(len(mid), bool) for m in ls])  # noqa: E731
                bottom = ~covered(range(l - below, l))
                top = ~covered(range(l + 1, l + above + 1))
                assert (cls[long_] == bottom.astype(np.uint8) + 2 * top.astype(np.uint8)).all(), (below, above, angles, l)
                seen += len(mid)
    assert seen > 500 and skipped <= 0.02 * (seen + skipped), (seen, skipped)


def test_no_window_is_the_plain_hatch():
    """below = above = 0: every piece has class 0, and on inputs without same-layer ties the segments and lines are the hatch's."""
    for c in (H.hand_loops(), K.square_stack(), K.pyramid()):
        for angles in ANGLES:
            d = H.directions(angles)
            a, b = K.skin(c, 0.5, d, 0, 0, 0.0437), H.hatch(c, 0.5, d, 0.0437)
            assert a.seg.tobytes() == b.seg.tobytes() and a.line.tobytes() == b.line.tobytes() and a.layer_start.tobytes() == b.layer_start.tobytes()
            assert a.layers.tobytes() == b.layers.tobytes() and not a.cls.any() and a.stats["n_segments"] > 20
            assert a.stats["n_crossings"] == a.stats["n_own_crossings"] == b.stats["n_crossings"] and a.stats["n_lines"] == b.stats["n_lines"]
            assert a.stats["length"][0] == b.stats["length"] and a.stats["zero_length"] == b.stats["zero_length"]


def test_the_pieces_of_a_line_merge_into_the_plain_hatch():
    """For any window the pieces of a line, joined where one ends at the value the next starts at, are the plain hatch's segments.
    The layers' totals are the hatch's lengths to within the terms' roundings: a term is below 2^(e+2), so its subtraction is off
    by at most 2^(e-51) and its quantisation by 2^(e-59): together less than 2^(e-50) for each piece and each segment."""
    for c in (H.hand_loops(), K.square_stack()):
        for below, above in ((1, 1), (2, 3), (0, 1), (8, 8)):
            d = H.directions((17.0, 73.0, 121.0))
            a, b = K.skin(c, 0.5, d, below, above, 0.0437), H.hatch(c, 0.5, d, 0.0437)
            join = np.concatenate([[False], (a.line[1:] == a.line[:-1]) & (a.start_u[1:] == a.end_u[:-1])])
            join[a.layer_start[1:-1][a.layer_start[1:-1] < len(join)]] = False
            first = np.flatnonzero(~join)
            last = np.concatenate([first[1:] - 1, [len(join) - 1]])
            merged = np.concatenate([a.seg[first, :2], a.seg[last, 2:]], axis=1)
            assert merged.tobytes() == b.seg.tobytes() and a.line[first].tobytes() == b.line.tobytes(), (below, above)
            assert a.stats["n_own_crossings"] == b.stats["n_crossings"] and a.stats["n_lines"] == b.stats["n_lines"]
            for l in range(c.n_layers):
                assert abs(a.layers[l]["length"] - b.layers[l]["length"]) <= float(a.layers[l]["n_segments"] + b.layers[l]["n_segments"]) * 2.0 ** (a.exponent - 50)
                assert a.layers[l]["n_segments"] == a.skin_layers[l]["n_segments"].sum()


def test_whole_layer_skin():
    """A window wider than the stack: every source but the layer itself is missing somewhere, so every piece is both top and bottom
    skin. With (2, 1) the first two layers are bottom skin and the last one top skin throughout."""
    c = K.square_stack()
    d = H.directions((45.0, 135.0))
    h = K.skin(c, 0.5, d, 8, 8, 0.0437)
    assert h.stats["n_segments"] > 100 and (h.cls == 3).all() and h.stats["n_class"] == [0, 0, 0, h.stats["n_segments"]]
    h = K.skin(c, 0.5, d, 2, 1, 0.0437)
    assert (h.cls[:h.layer_start[2]] & 1).all() and (h.cls[h.layer_start[6]:] & 2).all() and set(h.cls.tolist()) == {0, 1, 2, 3}


def test_bit_identical_layers_make_no_slivers():
    """Five equal squares: the layers' crossings tie on every line, the own layer's crossing decides the coordinates, the middle
    layers are inner throughout and every layer has the plain hatch's segments."""
    c = S.pack([K.square(3, 0.25, 0.5)] * 5, list(range(5)), 5)
    for angles in ANGLES:
        d = H.directions(angles)
        a, b = K.skin(c, 0.5, d, 1, 1, 0.0437), H.hatch(c, 0.5, d, 0.0437)
        assert a.seg.tobytes() == b.seg.tobytes() and a.stats["zero_length"] == 0
        assert (a.cls[:a.layer_start[1]] == 1).all() and (a.cls[a.layer_start[1]:a.layer_start[4]] == 0).all() and (a.cls[a.layer_start[4]:] == 2).all()
    # three combs of 40 teeth of width 0.5, each shifted by one tooth: [0, 20], [0.5, 20.5], [1, 21]. Where two teeth touch, two
    # crossings of one source share a value and its parity does not change there: the teeth do not split the pieces, the layers' ends do
    h = K.skin(K.shifted_combs(40), 0.25, [(1.0, 0.0)], 1, 1, 0.125)
    assert h.stats["max_line_crossings"] == 240 and h.stats["zero_length"] == 0 and (h.end_u > h.start_u).all()
    assert h.stats["n_segments"] == 12 * 7 and h.cls.tolist() == [3, 1] * 12 + [2, 0, 1] * 12 + [2, 3] * 12
    assert h.seg[:2, [0, 2]].tolist() == [[0, 0.5], [0.5, 20]] and h.seg[24:27, [0, 2]].tolist() == [[0.5, 1], [1, 20], [20, 20.5]]


def test_argument_checks():
    c = S.pack([S.circle(40)])
    for below, above in ((9, 0), (0, 9), (-1, 0)):
        with pytest.raises(ValueError):
            K.skin(c, 1.0, [(1.0, 0.0)], below, above)
    with pytest.raises(ValueError):
        K.skin(c, 0.0, [(1.0, 0.0)], 1, 1)
    empty = S.Loops(np.zeros((0, 2), F), [0], n_layers=2)
    h = K.skin(empty, 1.0, [(1.0, 0.0)], 1, 1)
    assert h.stats["n_segments"] == 0 and h.layer_start.tolist() == [0, 0, 0] and h.layers.tolist() == [(0.0, 0, 0, -1)] * 2 and len(h.cls) == 0


def test_the_python_records_have_the_header_s_layout():
    from gsdf_amd import hip
    assert C.sizeof(hip.SkinOpts) == 8 and hip.SkinOpts.above.offset == 4
    assert C.sizeof(hip.SkinLayer) == 64 == hip.SKIN_LAYER_DTYPE.itemsize == K.SKIN_LAYER_DTYPE.itemsize and hip.SkinLayer.n_segments.offset == 32
    assert hip.SKIN_LAYER_DTYPE == K.SKIN_LAYER_DTYPE
    st = hip.SkinStats
    assert C.sizeof(st) == 136 and st.ms_device.offset == 128 == st.RESULT_BYTES
    assert (st.zero_length.offset, st.n_class.offset, st.length.offset, st.n_layers.offset, st.below.offset, st.above.offset) == (40, 48, 80, 112, 116, 120)
    for s in ("gsdf_hip_contour_hatch_skin", "gsdf_hip_hatch_read_skin", "gsdf_hip_skin_rank_ms"):
        assert s in hip.SYMBOLS
    hdr = open(hip.__file__.replace("gsdf_amd/hip.py", "include/gsdf_hip.h")).read()
    for text in ("sizeof(gsdf_skin_opts) == 8", "sizeof(gsdf_skin_layer) == 64", "sizeof(gsdf_skin_stats) == 136", "offsetof(gsdf_skin_stats, ms_device) == 128"):
        assert text in hdr, text
