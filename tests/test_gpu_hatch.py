"""Hatch fill on the device (gsdf_hip_contour_hatch; gsdf_amd/csrc/kernels_hatch.h) against the CPU twin of the contract
(tests/hatchref.py): segments, line numbers, layer starts, the layers' records and the statistics' leading block identical, as bytes
-- hand loops at every direction, thousands of small loops across workgroups, a comb whose lines carry 800 crossings with ties,
edges that cross thousands of lines, traced and simplified handles, dry runs, the handle's history, the errors."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import contourref
import contoursimpref as S
import hatchref as H
from contourref import res_for
from scaffold.builder import Builder

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
BAD_ARGUMENT, CAPACITY = -3, -10


def upload(gpu, c):
    return gpu.ContourHIP.from_arrays(c.xy, c.loop_start, c.loop_layer, c.n_layers, c.keys)


def stats_bytes(gpu, st):
    """The twin's statistics as the leading block of a gsdf_hatch_stats."""
    r = gpu.HatchStats()
    for f in ("n_segments", "n_crossings", "n_lines", "max_line_crossings", "zero_length", "n_layers", "length"):
        setattr(r, f, st[f])
    return r.result_bytes()


def same(gpu, got, want, what):
    assert (got.n_layers, got.n_segments) == (want.stats["n_layers"], want.stats["n_segments"]), (what, got.n_segments, want.stats)
    for f in ("line", "layer_start", "seg", "layers"):
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, a.dtype, b.dtype, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero(a != b) if a.ndim == 1 else np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)).any(axis=1))
            raise AssertionError((what, f, len(bad), bad[:5].tolist(), a[bad[:3]].tolist(), b[bad[:3]].tolist()))
    st = got.stats
    assert st.result_bytes() == stats_bytes(gpu, want.stats), (what, [getattr(st, f) for f in ("n_segments", "n_crossings", "n_lines", "max_line_crossings", "zero_length", "length")], want.stats)


def check(gpu, dev, ref, spacing, dirs, offset=0.0, what=None):
    """Hatch on the device and in the twin: the same bytes; the dry run says the same and builds nothing."""
    want = H.hatch(ref, spacing, dirs, offset)
    got = dev.hatch_dirs(spacing, dirs, offset)
    same(gpu, got, want, what)
    assert got.stats.ms_device > 0 or got.n_segments == 0, what
    none, dry = dev.hatch_dirs(spacing, dirs, offset, dry=True)
    assert none is None and dry.result_bytes() == got.stats.result_bytes(), what
    return got, want


def code(gpu, fn):
    with pytest.raises(gpu.HipError) as e:
        fn()
    return e.value.code, e.value.msg


# ---- hand loops ----------------------------------------------------------------------------------------------------------------------
def test_hand_loops_at_every_direction(gpu):
    """Five layers, one of them empty; one to four directions (three over five layers: l % 3), reversed ones, lines through the
    lattice vertices and along the sides (0 / 90 degrees at offset 0), every spacing of the twin's own tests."""
    ref = H.hand_loops()
    dev = upload(gpu, ref)
    segs = 0
    for angles in ((45.0, 135.0), (0.0, 90.0), (17.0, 73.0, 121.0), (0.0, 45.0, 90.0, 135.0), (30.0,)):
        d = H.directions(angles)
        for sp in (0.125, 0.5, 3.0):
            for off in (0.0, 0.0437):
                got, want = check(gpu, dev, ref, sp, d, off, (angles, sp, off))
                check(gpu, dev, ref, sp, -d, -off, (angles, sp, off, "reversed"))
                segs += got.n_segments
                assert got.layers[3].tolist() == (0.0, 0, 0, -1) and len(got.segments(3)) == 0
    assert segs > 6000          # (more than 600 at spacing 0.125 for each of the ten direction sets and offsets)
    # raw directions that are no unit vectors; the angles through ContourHIP.hatch
    check(gpu, dev, ref, 0.25, np.array([(1.0, 1.0), (-0.5, 0.25), (2.0 ** -20, -1.0)], F), -0.3, "raw directions")
    a, b = dev.hatch(0.5, (45.0, 135.0), 0.0437), dev.hatch_dirs(0.5, H.directions((45.0, 135.0)), 0.0437)
    assert a.seg.tobytes() == b.seg.tobytes() and a.stats.result_bytes() == b.stats.result_bytes()


def test_a_dyadic_rectangle_in_closed_form(gpu):
    ref = S.pack([np.array([(2, 1), (6, 1), (6, 3), (2, 3)], F)])
    got, _ = check(gpu, upload(gpu, ref), ref, 0.5, [(1.0, 0.0)], 0.0, "rectangle")
    assert got.seg.tobytes() == np.array([(2, y, 6, y) for y in (1.5, 2.0, 2.5, 3.0)], F).tobytes() and got.line.tolist() == [3, 4, 5, 6]
    assert got.layers[0].tolist() == (16.0, 4, 3, 6) and got.stats.length == 16.0


# ---- scale ---------------------------------------------------------------------------------------------------------------------------
def test_thousands_of_small_loops_across_blocks(gpu):
    """Buckets filled from many workgroups in arbitrary order: the loops overlap, a line carries hundreds of crossings from edges that
    are thousands of vertices apart."""
    ref = S.mixed_loops(3000, 5)
    dev = upload(gpu, ref)
    got, want = check(gpu, dev, ref, 0.5, H.directions((45.0, 135.0)), 0.0, "mixed")
    assert want.stats["n_crossings"] > 200 * 256 and want.stats["max_line_crossings"] > 256
    again = dev.hatch(0.5, (45.0, 135.0))
    assert again.seg.tobytes() == got.seg.tobytes() and again.line.tobytes() == got.line.tobytes() and again.stats.result_bytes() == got.stats.result_bytes()
    assert again.layers.tobytes() == got.layers.tobytes() and again.layer_start.tobytes() == got.layer_start.tobytes()
    check(gpu, dev, ref, 3.0, H.directions((0.0, 90.0, 30.0)), 1.5, "mixed, wide")


def test_a_comb_with_800_crossings_on_a_line_and_ties(gpu):
    """400 thin rectangles in a row under horizontal lines: buckets larger than a workgroup; where two teeth touch, two crossings have
    the same u_c and the tail's vertex number decides. With offset 0 the lines run through the teeth's corners too."""
    ref = H.comb(400)
    dev = upload(gpu, ref)
    got, want = check(gpu, dev, ref, 0.25, [(1.0, 0.0)], 0.125, "comb")
    assert want.stats["max_line_crossings"] == 800 and want.stats["zero_length"] == 0 and got.n_segments == 400 * 12
    assert (got.seg[:, 2] - got.seg[:, 0] == 0.5).all()
    check(gpu, dev, ref, 0.25, [(1.0, 0.0)], 0.0, "comb, through the corners")
    check(gpu, dev, ref, 0.25, [(-1.0, 0.0)], 0.0, "comb, reversed")
    check(gpu, dev, ref, 0.375, H.directions((3.0,)), 0.0, "comb, tilted")


def test_single_edges_that_cross_thousands_of_lines(gpu):
    """One triangle of side about 100 at spacing 1 / 64: an edge crosses more than 256 lines (a workgroup of crossings from one edge)
    and more than 65 536 / 64."""
    ref = S.pack([np.array([(-31.7, -20.3), (68.9, -17.1), (12.3, 70.9)], F)])
    dev = upload(gpu, ref)
    for angles, off in (((45.0,), 0.0), ((0.0,), 0.013), ((101.0,), -7.0)):
        got, want = check(gpu, dev, ref, 1.0 / 64, H.directions(angles), off, ("triangle", angles))
        assert want.stats["n_lines"] > 4096 and want.stats["max_line_crossings"] == 2
        area = float(S.measures(ref)[1][0]["area"])
        assert abs(got.stats.length / 64 - area) <= float(S.measures(ref)[1][0]["length"]) / 64 * (1 + 1e-6)


# ---- through the pipeline ------------------------------------------------------------------------------------------------------------
def hatch_traced_and_simplified(gpu, dev, res, what):
    ref = S.Loops.of(dev)
    d = H.directions((45.0, 135.0))
    before = (dev.xy.tobytes(), dev.loop_start.tobytes(), dev.stats.result_bytes())
    got, want = check(gpu, dev, ref, F(F(4) * res), d, 0.0, what)
    assert want.stats["n_segments"] > 0
    simple, _ = dev.simplify(F(res / F(8)))
    check(gpu, simple, S.simplify(ref, F(res / F(8)))[0], F(F(4) * res), d, 0.0, (what, "simplified"))
    # the handle was hatched and simplified: its answer is what it was, and so is the handle
    again = dev.hatch_dirs(F(F(4) * res), d)
    for f in ("seg", "line", "layer_start", "layers"):
        assert getattr(again, f).tobytes() == getattr(got, f).tobytes(), (what, f)
    assert again.stats.result_bytes() == got.stats.result_bytes()
    assert before == (dev.xy.tobytes(), dev.loop_start.tobytes(), dev.stats.result_bytes())
    # the result does not need the loops it came from
    seg = got.seg.copy()
    dev.close()
    back = np.empty_like(seg)
    assert gpu.lib().gsdf_hip_hatch_read(got._h, back.ctypes.data, None, None, None) == 0 and back.tobytes() == seg.tobytes()
    return got


def test_the_text_outline(gpu):
    spec = importlib.util.spec_from_file_location("render_png", os.path.join(ROOT, "examples", "render_png.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sdf = gpu.SDF2HIP(mod.scene("text"))
    res = res_for(sdf.Bounds(), 60)
    hatch_traced_and_simplified(gpu, gpu.ContourHIP.outline(sdf, res), res, "text")


def test_four_slices_of_a_part(gpu):
    s = Builder().Scene("bolt")
    bb = s.Bounds()
    res = F(float(s.Diagonal()) / 60)
    z = contourref.layer_heights(bb, F(F(bb[5] - bb[2]) / F(4)))
    dev = gpu.ContourHIP.slices(gpu.SDF3HIP(s), res, z)
    assert dev.n_layers == 4
    got = hatch_traced_and_simplified(gpu, dev, res, "bolt")
    assert len({tuple(got.layers[l].tolist()) for l in range(4)}) > 1


# ---- errors and the empty handle -----------------------------------------------------------------------------------------------------
def test_argument_errors(gpu):
    ref = S.pack([S.circle(40)])
    c = upload(gpu, ref)
    d = [(1.0, 0.0)]
    for sp in (0.0, -1.0, float("nan"), float("inf")):
        assert code(gpu, lambda: c.hatch_dirs(sp, d))[0] == BAD_ARGUMENT, sp
    for off in (float("nan"), float("inf"), -float("inf")):
        assert code(gpu, lambda: c.hatch_dirs(1.0, d, off))[0] == BAD_ARGUMENT, off
    for dirs in ([], [(1, 0)] * 5, [(0.0, 0.0)], [(1.5, 0.0)], [(0.0, -1.25)], [(float("nan"), 0.0)], [(1.0, 0.0), (0.0, float("inf"))]):
        assert code(gpu, lambda: c.hatch_dirs(1.0, dirs))[0] == BAD_ARGUMENT, dirs
    # a bad direction behind n_dirs is not looked at
    o = gpu.HatchOpts(F(1.0), F(0.0), 1, 0)
    o.dir[0][0], o.dir[1][0] = 1.0, float("nan")
    L = gpu.lib()
    h, st = C.c_void_p(), gpu.HatchStats()
    assert L.gsdf_hip_contour_hatch(c._h, C.byref(o), C.byref(h), C.byref(st)) == 0 and h.value and st.n_segments == 20
    L.gsdf_hip_hatch_destroy(h)
    assert L.gsdf_hip_contour_hatch(c._h, C.byref(o), None, None) == BAD_ARGUMENT            # out NULL without dry
    assert L.gsdf_hip_contour_hatch(c._h, None, C.byref(h), None) == BAD_ARGUMENT
    assert L.gsdf_hip_contour_hatch(None, C.byref(o), C.byref(h), None) == BAD_ARGUMENT
    assert L.gsdf_hip_hatch_counts(None, None, None) == BAD_ARGUMENT and L.gsdf_hip_hatch_read(None, None, None, None, None) == BAD_ARGUMENT
    o.dry = 1
    h = C.c_void_p(12345)
    assert L.gsdf_hip_contour_hatch(c._h, C.byref(o), C.byref(h), None) == 0 and not h.value   # dry: nothing built, out set to NULL
    assert L.gsdf_hip_contour_hatch(c._h, C.byref(o), None, None) == 0
    L.gsdf_hip_hatch_destroy(None)
    # e = 4 (the circle of radius 10 about (3, -2)): 2^5 / spacing reaches 2^29 at spacing 2^-24
    rc, msg = code(gpu, lambda: c.hatch_dirs(2.0 ** -24, d))
    assert rc == BAD_ARGUMENT and "spacing is too small for these coordinates" in msg
    rc, msg = code(gpu, lambda: c.hatch_dirs(1.0, d, 2.0 ** 29))
    assert rc == BAD_ARGUMENT and "spacing is too small for these coordinates" in msg
    check(gpu, c, ref, 1.0, d, 2.0 ** 28, "a large offset")


def test_capacity_errors(gpu):
    """e = 10 for coordinates up to 1000, so spacing 1.05 x 2^-18 is allowed and a span of 2000 holds 0.93 x 2^29 lines. Five layers
    with a small loop at either end: 2^31 line slots or more, a handful of crossings. Five slivers of that length in one layer: ten
    long edges, 2^32 crossings or more. Both are refused from the range pass's counts, before anything of that size is allocated."""
    sp = F(1.05 * 2.0 ** -18)
    d = [(0.0, 1.0)]          # s = -x
    small = np.array([(0, 0), (2.0 ** -10, 0), (0, 2.0 ** -10)], F)
    loops, layers = [], []
    for l in range(5):
        loops += [small + F(-1000), small + F(999)]
        layers += [l, l]
    rc, msg = code(gpu, lambda: upload(gpu, S.pack(loops, layers, 5)).hatch_dirs(sp, d))
    assert rc == CAPACITY and "line slots" in msg
    slivers = [np.array([(-1000, y), (1000, y), (1000, y + 0.25)], F) for y in range(5)]
    rc, msg = code(gpu, lambda: upload(gpu, S.pack(slivers)).hatch_dirs(sp, d))
    assert rc == CAPACITY and "crossings" in msg
    rc, msg = code(gpu, lambda: upload(gpu, S.pack(slivers)).hatch_dirs(sp, d, dry=True))
    assert rc == CAPACITY


def test_no_loops_at_all(gpu):
    b = Builder()
    s = b.Intersection2D(b.Translate2D(b.NewCircle(0.4), 0.45, 1), b.NewRectangle(1, 0.61))
    dev = gpu.ContourHIP.outline(gpu.SDF2HIP(s), F(0.1))
    assert dev.n_loops == 0
    h = dev.hatch(0.05)
    assert (h.n_segments, h.n_layers, h.layer_start.tolist(), h.layers.tolist()) == (0, 1, [0, 0], [(0.0, 0, 0, -1)])
    st = h.stats
    assert st.result_bytes() == stats_bytes(gpu, {"n_segments": 0, "n_crossings": 0, "n_lines": 0, "max_line_crossings": 0, "zero_length": 0, "n_layers": 1, "length": 0.0})
    assert st.ms_device == 0 and dev.hatch(0.05, dry=True)[1].result_bytes() == st.result_bytes()
    # loops that no line meets: a handle without segments as well
    ref = S.pack([S.circle(12, 0.2, 0.5, 0.5)])
    got, _ = check(gpu, upload(gpu, ref), ref, 2.0, [(1.0, 0.0)], 1.0, "between two lines")
    assert got.n_segments == 0
