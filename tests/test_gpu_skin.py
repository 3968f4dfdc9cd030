"""Skin classification of the hatch on the device (gsdf_hip_contour_hatch_skin; gsdf_amd/csrc/kernels_skin.h) against the CPU twin of
the contract (tests/skinref.py): segments, line numbers, classes, layer starts, both kinds of layer records and the statistics'
leading block identical, as bytes -- stacks of squares at every window, hand loops with an empty layer, thousands of small loops
across workgroups, combs whose layers tie at every tooth, traced and simplified handles, bit-identical layers of an extrusion, dry
runs, the handle's history, the errors."""
import ctypes as C

import numpy as np
import pytest

import contourref
import contoursimpref as S
import hatchref as H
import skinref as K
from scaffold.builder import Builder

pytestmark = pytest.mark.gpu

F = np.float32
BAD_ARGUMENT, CAPACITY = -3, -10
WINDOWS = ((0, 0), (1, 1), (2, 3), (8, 8), (0, 1))


def upload(gpu, c):
    return gpu.ContourHIP.from_arrays(c.xy, c.loop_start, c.loop_layer, c.n_layers, c.keys)


def stats_bytes(gpu, st):
    """The twin's statistics as the leading block of a gsdf_skin_stats."""
    r = gpu.SkinStats()
    for f in K.STATS_FIELDS:
        if f in ("n_class", "length"):
            for a in range(4):
                getattr(r, f)[a] = st[f][a]
        else:
            setattr(r, f, st[f])
    return r.result_bytes()


def same(gpu, got, want, what):
    assert (got.n_layers, got.n_segments) == (want.stats["n_layers"], want.stats["n_segments"]), (what, got.n_segments, want.stats)
    for f in ("line", "cls", "layer_start", "seg", "layers", "skin_layers"):
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero(a != b) if a.ndim == 1 else np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).any(axis=1))
            raise AssertionError((what, f, len(bad), bad[:5].tolist(), a[bad[:3]].tolist(), b[bad[:3]].tolist()))
    st = got.stats
    assert st.result_bytes() == stats_bytes(gpu, want.stats), (what, [getattr(st, f) for f in K.STATS_FIELDS[:6]], list(st.n_class), list(st.length), want.stats)


def check(gpu, dev, ref, spacing, dirs, below, above, offset=0.0, what=None):
    """Skin on the device and in the twin: the same bytes; the dry run says the same and builds nothing."""
    want = K.skin(ref, spacing, dirs, below, above, offset)
    got = dev.skin_dirs(spacing, dirs, below, above, offset)
    same(gpu, got, want, what)
    assert got.stats.ms_device > 0 or got.n_segments == 0, what
    none, dry = dev.skin_dirs(spacing, dirs, below, above, offset, dry=True)
    assert none is None and dry.result_bytes() == got.stats.result_bytes(), what
    return got, want


def code(gpu, fn):
    with pytest.raises(gpu.HipError) as e:
        fn()
    return e.value.code, e.value.msg


# ---- hand-made stacks ----------------------------------------------------------------------------------------------------------------
def test_stacks_of_squares_at_every_window(gpu):
    """Seven squares (equal, shrinking, shifted, equal) and the pyramid, one to four directions -- with two or three the direction of a
    layer differs from its neighbours', whose edges are crossed under the TARGET's --, every window of the contract's edge cases: none,
    symmetric, asymmetric, wider than the stack, above only."""
    pieces = set()
    for ref in (K.square_stack(), K.pyramid()):
        dev = upload(gpu, ref)
        for below, above in WINDOWS:
            for angles in ((30.0,), (45.0, 135.0), (17.0, 73.0, 121.0), (0.0, 45.0, 90.0, 135.0)):
                for sp, off in ((0.5, 0.0437), (0.125, 0.0)):
                    got, want = check(gpu, dev, ref, sp, H.directions(angles), below, above, off, (ref.n_layers, below, above, angles, sp))
                    pieces |= set(got.cls.tolist())
            if (below, above) == (8, 8):
                assert (got.cls == 3).all()
    assert pieces == {0, 1, 2, 3}
    # the closed form of the twin's own test, from the device
    got = upload(gpu, K.pyramid()).skin_dirs(1.0, [(1.0, 0.0)], 0, 1, 0.5)
    assert (got.n_segments, got.stats.n_lines, got.stats.n_crossings) == (20, 12, 32) and got.cls.tolist() == ([2] * 2 + [2, 0, 2] * 4 + [2] * 2) + [2] * 4
    assert got.seg[2:5].tolist() == [[0, 2.5, 2, 2.5], [2, 2.5, 6, 2.5], [6, 2.5, 8, 2.5]] and list(got.stats.length) == [16.0, 0.0, 64.0, 0.0]


def test_hand_loops_with_an_empty_layer(gpu):
    """Five layers, layer 3 empty: layer 2 is top skin and layer 4 bottom skin throughout once the window reaches it; raw directions
    that are no unit vectors; the angles through ContourHIP.skin."""
    ref = H.hand_loops()
    dev = upload(gpu, ref)
    for below, above in WINDOWS:
        for angles in ((45.0, 135.0), (0.0, 90.0), (17.0, 73.0, 121.0)):
            for sp, off in ((0.125, 0.0), (0.5, 0.0437), (3.0, 0.0437)):
                got, want = check(gpu, dev, ref, sp, H.directions(angles), below, above, off, (below, above, angles, sp, off))
                assert got.layers[3].tolist() == (0.0, 0, 0, -1) and not got.skin_layers[3]["n_segments"].any()
                if above:
                    assert (got.cls[got.layer_start[2]:got.layer_start[3]] & 2).all()
    check(gpu, dev, ref, 0.25, np.array([(1.0, 1.0), (-0.5, 0.25), (2.0 ** -20, -1.0)], F), 1, 2, -0.3, "raw directions")
    a, b = dev.skin(0.5, (45.0, 135.0), 1, 1, 0.0437), dev.skin_dirs(0.5, H.directions((45.0, 135.0)), 1, 1, 0.0437)
    assert a.seg.tobytes() == b.seg.tobytes() and a.cls.tobytes() == b.cls.tobytes() and a.stats.result_bytes() == b.stats.result_bytes()
    # no window: the plain hatch's segments, every one of class 0
    plain, none = dev.hatch(0.5, (45.0, 135.0), 0.0437), dev.skin(0.5, (45.0, 135.0), 0, 0, 0.0437)
    assert plain.seg.tobytes() == none.seg.tobytes() and plain.line.tobytes() == none.line.tobytes() and plain.layers.tobytes() == none.layers.tobytes()
    assert not none.cls.any() and plain.cls is None and plain.skin_layers is None


# ---- scale ---------------------------------------------------------------------------------------------------------------------------
def test_thousands_of_small_loops_across_blocks(gpu):
    """Buckets filled from many workgroups in arbitrary order by three source layers each; waves that span several buckets and
    buckets that span several waves."""
    ref = S.mixed_loops(1500, 5)
    dev = upload(gpu, ref)
    d = H.directions((45.0, 135.0))
    got, want = check(gpu, dev, ref, 0.5, d, 1, 1, 0.0, "mixed")
    assert want.stats["n_crossings"] > 200 * 256 and want.stats["max_line_crossings"] > 256 and min(want.stats["n_class"]) > 1000
    again = dev.skin_dirs(0.5, d, 1, 1)
    for f in ("seg", "line", "cls", "layer_start", "layers", "skin_layers"):
        assert getattr(again, f).tobytes() == getattr(got, f).tobytes(), f
    assert again.stats.result_bytes() == got.stats.result_bytes()
    check(gpu, dev, ref, 3.0, H.directions((0.0, 90.0, 30.0)), 2, 3, 1.5, "mixed, wide")


def test_combs_whose_layers_tie_at_every_tooth(gpu):
    """hatchref.comb(400) in three layers, each shifted by one tooth: 2 400 crossings on a line, and at every tooth's side two
    crossings of each of up to three sources share one value."""
    ref = K.shifted_combs(400)
    dev = upload(gpu, ref)
    got, want = check(gpu, dev, ref, 0.25, [(1.0, 0.0)], 1, 1, 0.125, "combs")
    assert want.stats["max_line_crossings"] == 2400 and want.stats["zero_length"] == 0 and got.n_segments == 12 * 7
    assert got.cls.tolist() == [3, 1] * 12 + [2, 0, 1] * 12 + [2, 3] * 12
    check(gpu, dev, ref, 0.25, [(1.0, 0.0)], 1, 1, 0.0, "combs, through the corners")
    check(gpu, dev, ref, 0.25, [(-1.0, 0.0)], 0, 1, 0.0, "combs, reversed")
    check(gpu, dev, ref, 0.375, H.directions((3.0, 177.0)), 2, 2, 0.0, "combs, tilted")


# ---- through the pipeline ------------------------------------------------------------------------------------------------------------
def test_slices_of_a_part_traced_and_simplified(gpu):
    """Four and six slices of the bolt; the handle is what it was afterwards, and the result does not need it."""
    s = Builder().Scene("bolt")
    bb = s.Bounds()
    res = F(float(s.Diagonal()) / 60)
    sdf = gpu.SDF3HIP(s)
    d = H.directions((45.0, 135.0))
    for n in (4, 6):
        dev = gpu.ContourHIP.slices(sdf, res, contourref.layer_heights(bb, F(F(bb[5] - bb[2]) / F(n))))
        assert dev.n_layers == n
        ref = S.Loops.of(dev)
        before = (dev.xy.tobytes(), dev.loop_start.tobytes(), dev.stats.result_bytes())
        got, want = check(gpu, dev, ref, F(F(4) * res), d, 1, 1, 0.0, ("bolt", n))
        assert want.stats["n_segments"] > 0 and len(set(got.cls.tolist())) > 1
        check(gpu, dev, ref, F(F(4) * res), d, 2, 3, 0.0, ("bolt", n, "wide"))
        simple, _ = dev.simplify(F(res / F(8)))
        check(gpu, simple, S.simplify(ref, F(res / F(8)))[0], F(F(4) * res), d, 1, 1, 0.0, ("bolt", n, "simplified"))
        assert before == (dev.xy.tobytes(), dev.loop_start.tobytes(), dev.stats.result_bytes())
        # gsdf_hip_hatch_read on a skin handle: the layers' totals over the four classes
        assert got.layers["n_segments"].tolist() == got.skin_layers["n_segments"].sum(axis=1).tolist() == np.diff(got.layer_start.astype(np.int64)).tolist()
        seg, cls = got.seg.copy(), got.cls.copy()
        dev.close()
        back, back_cls = np.empty_like(seg), np.empty_like(cls)
        assert gpu.lib().gsdf_hip_hatch_read(got._h, back.ctypes.data, None, None, None) == 0 and back.tobytes() == seg.tobytes()
        assert gpu.lib().gsdf_hip_hatch_read_skin(got._h, back_cls.ctypes.data, None) == 0 and back_cls.tobytes() == cls.tobytes()


def test_the_middle_layers_of_an_extrusion_are_inner(gpu):
    """A plate with a hole, extruded: the slices away from its two faces are bit-identical loops, so between them every crossing of a
    layer ties with its neighbours'. Only class 0 may appear there, and no sliver."""
    b = Builder()
    s = b.Extrude(b.Difference2D(b.NewRectangle(3.0, 2.0), b.Translate2D(b.NewCircle(0.5), 0.4, 0.1)), 2.0)
    bb = s.Bounds()
    res = F(float(s.Diagonal()) / 60)
    dev = gpu.ContourHIP.slices(gpu.SDF3HIP(s), res, contourref.layer_heights(bb, F(F(bb[5] - bb[2]) / F(8))))
    L = dev.n_layers
    assert L == 8 and dev.n_loops == 2 * L
    per = [np.concatenate(dev.loops(l)).tobytes() for l in range(L)]
    assert len(set(per[1:L - 1])) == 1          # the loops of the layers 1 .. L-2 are the same bytes
    ref = S.Loops.of(dev)
    got, want = check(gpu, dev, ref, F(F(3) * res), H.directions((45.0, 135.0, 10.0)), 1, 1, 0.0, "extrusion")
    mid = got.cls[got.layer_start[2]:got.layer_start[L - 2]]
    assert len(mid) > 50 and not mid.any() and got.stats.zero_length == 0
    assert (got.cls[:got.layer_start[1]] & 1).all() and (got.cls[got.layer_start[L - 1]:] & 2).all()
    plain = dev.hatch_dirs(F(F(3) * res), H.directions((45.0, 135.0, 10.0)))
    assert plain.seg[plain.layer_start[2]:plain.layer_start[L - 2]].tobytes() == got.seg[got.layer_start[2]:got.layer_start[L - 2]].tobytes()


# ---- errors and the empty handle -----------------------------------------------------------------------------------------------------
def test_argument_errors(gpu):
    ref = S.pack([S.circle(40)])
    c = upload(gpu, ref)
    d = [(1.0, 0.0)]
    for sp in (0.0, -1.0, float("nan"), float("inf")):
        assert code(gpu, lambda: c.skin_dirs(sp, d, 1, 1))[0] == BAD_ARGUMENT, sp
    assert code(gpu, lambda: c.skin_dirs(1.0, d, 1, 1, float("nan")))[0] == BAD_ARGUMENT
    for dirs in ([], [(1, 0)] * 5, [(0.0, 0.0)], [(1.5, 0.0)], [(float("nan"), 0.0)]):
        assert code(gpu, lambda: c.skin_dirs(1.0, dirs, 1, 1))[0] == BAD_ARGUMENT, dirs
    for below, above in ((9, 0), (0, 9), (2 ** 32 - 1, 0)):
        rc, msg = code(gpu, lambda: c.skin_dirs(1.0, d, below, above))
        assert rc == BAD_ARGUMENT and "0 .. 8" in msg, (below, above)
    check(gpu, c, ref, 1.0, d, 8, 8, 0.0, "the widest window")
    L = gpu.lib()
    o, k = gpu.HatchOpts(F(1.0), F(0.5), 1, 0), gpu.SkinOpts(1, 1)      # the lines y = -11.5 .. 7.5 (offset 0 puts one through the top vertex)
    o.dir[0][0] = 1.0
    h, st = C.c_void_p(), gpu.SkinStats()
    assert L.gsdf_hip_contour_hatch_skin(c._h, C.byref(o), C.byref(k), C.byref(h), C.byref(st)) == 0 and h.value and st.n_segments == 20 and list(st.n_class) == [0, 0, 0, 20]
    L.gsdf_hip_hatch_destroy(h)
    assert L.gsdf_hip_contour_hatch_skin(c._h, C.byref(o), None, C.byref(h), None) == BAD_ARGUMENT          # no skin options
    assert L.gsdf_hip_contour_hatch_skin(c._h, None, C.byref(k), C.byref(h), None) == BAD_ARGUMENT
    assert L.gsdf_hip_contour_hatch_skin(None, C.byref(o), C.byref(k), C.byref(h), None) == BAD_ARGUMENT
    assert L.gsdf_hip_contour_hatch_skin(c._h, C.byref(o), C.byref(k), None, None) == BAD_ARGUMENT          # out NULL without dry
    assert L.gsdf_hip_hatch_read_skin(None, None, None) == BAD_ARGUMENT
    o.dry = 1
    h = C.c_void_p(12345)
    assert L.gsdf_hip_contour_hatch_skin(c._h, C.byref(o), C.byref(k), C.byref(h), None) == 0 and not h.value   # dry: nothing built
    assert L.gsdf_hip_contour_hatch_skin(c._h, C.byref(o), C.byref(k), None, None) == 0
    rc, msg = code(gpu, lambda: c.skin_dirs(2.0 ** -24, d, 1, 1))
    assert rc == BAD_ARGUMENT and "spacing is too small for these coordinates" in msg
    # a plain hatch has no classes
    plain = c.hatch_dirs(1.0, d)
    cls = np.zeros(plain.n_segments, np.uint8)
    assert L.gsdf_hip_hatch_read_skin(plain._h, cls.ctypes.data, None) == BAD_ARGUMENT
    assert "no classes" in L.gsdf_hip_last_error().decode()


def test_capacity_errors(gpu):
    """The hatch's two cases (e = 10, spacing 1.05 x 2^-18: five layers with a small loop at either end, 2^31 line slots or more; five
    slivers, 2^32 own crossings or more), refused from the range pass's counts. And one that only the neighbours make: a sliver per
    layer in three layers is 0.70 x 2^32 own crossings (0.23 x 2^32 each, 0.35 x 2^31 line slots), and with two layers over each
    1 + 2 + 3 slivers cross the layers' own lines: 1.4 x 2^32, refused from the second range pass's count, dry or not."""
    sp = F(1.05 * 2.0 ** -18)
    d = [(0.0, 1.0)]          # s = -x
    small = np.array([(0, 0), (2.0 ** -10, 0), (0, 2.0 ** -10)], F)
    loops, layers = [], []
    for l in range(5):
        loops += [small + F(-1000), small + F(999)]
        layers += [l, l]
    rc, msg = code(gpu, lambda: upload(gpu, S.pack(loops, layers, 5)).skin_dirs(sp, d, 1, 1))
    assert rc == CAPACITY and "line slots" in msg
    slivers = [np.array([(-1000, y), (1000, y), (1000, y + 0.25)], F) for y in range(5)]
    rc, msg = code(gpu, lambda: upload(gpu, S.pack(slivers)).skin_dirs(sp, d, 1, 1))
    assert rc == CAPACITY and "crossings" in msg
    stack = upload(gpu, S.pack([slivers[0]] * 3, [0, 1, 2], 3))
    for dry in (False, True):
        rc, msg = code(gpu, lambda: stack.skin_dirs(sp, d, 0, 2, dry=dry))
        assert rc == CAPACITY and "skin: 2^32 crossings" in msg, dry


def test_no_loops_at_all(gpu):
    b = Builder()
    s = b.Intersection2D(b.Translate2D(b.NewCircle(0.4), 0.45, 1), b.NewRectangle(1, 0.61))
    dev = gpu.ContourHIP.outline(gpu.SDF2HIP(s), F(0.1))
    assert dev.n_loops == 0
    h = dev.skin(0.05, (45.0,), 1, 1)
    assert (h.n_segments, h.n_layers, h.layer_start.tolist(), h.layers.tolist(), len(h.cls)) == (0, 1, [0, 0], [(0.0, 0, 0, -1)], 0)
    assert not h.skin_layers["n_segments"].any() and not h.skin_layers["length"].any()
    empty = {f: 0 for f in K.STATS_FIELDS}
    empty.update(n_class=[0] * 4, length=[0.0] * 4, n_layers=1, below=1, above=1)
    assert h.stats.result_bytes() == stats_bytes(gpu, empty)
    assert h.stats.ms_device == 0 and dev.skin(0.05, (45.0,), 1, 1, dry=True)[1].result_bytes() == h.stats.result_bytes()
    # loops that no line meets: a handle without segments as well
    ref = S.pack([S.circle(12, 0.2, 0.5, 0.5)] * 2, [0, 1], 2)
    got, _ = check(gpu, upload(gpu, ref), ref, 2.0, [(1.0, 0.0)], 1, 1, 1.0, "between two lines")
    assert got.n_segments == 0
