"""The loops' offset on the device (gsdf_hip_contour_offset / gsdf_hip_contour_distance; gsdf_amd/csrc/kernels_offset.h) against the CPU
twin of the contract (tests/offsetref.py), which tests every node against every edge: xy, keys, loop_start, loop_layer, the D lattice
of every input layer and bytes 0 .. 79 of the statistics identical, as bytes -- closed forms, hand loops with an empty layer, an
annulus that vanishes and one that fragments, a stack of many loops over ragged tiles and several batches of edges, a comb of
touching loops, a traced handle offset, hatched and skinned; chunks, repeats, dry runs, the handle's history, scaling, the errors."""
import ctypes as C

import numpy as np
import pytest

import contoursimpref as S
import hatchref as H
import offsetref as O
from contourref import res_for
from handle_acts import SLICE_LADDER
from scaffold.builder import Builder

pytestmark = pytest.mark.gpu

F = np.float32
BAD_ARGUMENT, CAPACITY = -3, -10
RECT = S.pack([np.array([(2, 1), (6, 1), (6, 3), (2, 3)], F)])
_TWIN = {}


def twin(name, ref, res, insets):
    """The twin's result, computed once per case and shared."""
    key = (name, float(res), tuple(float(F(v)) for v in insets))
    if key not in _TWIN:
        _TWIN[key] = O.offset(ref, res, insets)
    return _TWIN[key]


def upload(gpu, c):
    return gpu.ContourHIP.from_arrays(c.xy, c.loop_start, c.loop_layer, c.n_layers, c.keys)


def same(got, want, what):
    assert (got.n_layers, got.n_loops, got.n_verts) == (want.n_layers, want.stats["n_loops"], want.stats["n_verts"]), (what, got.n_loops, got.n_verts, want.stats)
    for f in ("loop_start", "loop_layer", "keys"):
        assert getattr(got, f).tolist() == getattr(want, f).tolist(), (what, f)
    a, b = got.xy.view(np.uint32), want.xy.view(np.uint32)
    if a.tobytes() != b.tobytes():
        bad = np.flatnonzero((a != b).any(axis=1))
        raise AssertionError((what, "xy", len(bad), bad[:5].tolist(), got.xy[bad[:3]].tolist(), want.xy[bad[:3]].tolist()))


def check(gpu, dev, ref, res, insets, name, max_nodes=0, lattices=True):
    """Offset on the device and in the twin: the same bytes, loops, D lattices and statistics; the dry run says the same."""
    want = twin(name, ref, res, insets)
    got = dev.offset(res, insets, max_nodes)
    same(got, want, name)
    st = got.offset_stats
    assert st.result_bytes() == O.stats_bytes(want.stats), (name, [(f, getattr(st, f)) for f, _ in st._fields_[:14]], want.stats)
    cs = got.stats
    assert (cs.nx, cs.ny, cs.n_layers, cs.evals, cs.n_verts, cs.n_loops, cs.nonfinite_nodes) == (st.nx, st.ny, want.n_layers, 0, st.n_verts, st.n_loops, 0)
    assert st.ms_field > 0 and st.ms_trace > 0 and cs.ms_eval == st.ms_field
    if lattices:
        for l in range(ref.n_layers):
            d = dev.distance(res, insets, l)
            assert d.shape == want.D[l].shape and d.tobytes() == want.D[l].tobytes(), (name, l, np.argwhere(d.view(np.uint32) != want.D[l].view(np.uint32))[:5].tolist())
    none, dry = dev.offset(res, insets, max_nodes, dry=True)
    assert none is None and dry.result_bytes() == st.result_bytes(), name
    return got, want


def code(gpu, fn):
    with pytest.raises(gpu.HipError) as e:
        fn()
    return e.value.code, e.value.msg


# ---- closed forms --------------------------------------------------------------------------------------------------------------------
def test_the_rectangle_s_closed_forms(gpu):
    dev = upload(gpu, RECT)
    got, _ = check(gpu, dev, RECT, 0.5, (0.5, 0.25, 1.0, 1.25), "rect")
    assert got.loops(0)[0].tolist() == [[3, 1.5], [3.5, 1.5], [4, 1.5], [4.5, 1.5], [5, 1.5], [5.5, 2], [5, 2.5], [4.5, 2.5], [4, 2.5], [3.5, 2.5], [3, 2.5], [2.5, 2]]
    loops, layers = got.measures()
    assert layers["area"].tolist() == [2.5, 5.125, 0.0, 0.0] and layers["n_loops"].tolist() == [1, 1, 0, 0]
    got, _ = check(gpu, dev, RECT, 0.5, (-0.5,), "rect out")
    assert got.measures()[1]["area"].tolist() == [14.5]


def test_hand_loops_with_an_empty_layer(gpu):
    ref = H.hand_loops()
    dev = upload(gpu, ref)
    check(gpu, dev, ref, 0.25, (0.3,), "hand")
    got, want = check(gpu, dev, ref, 0.25, (-0.4, 0.0, 0.5, 1.0), "hand4")
    assert got.n_layers == 20 and not set(got.loop_layer.tolist()) & {12, 13, 14, 15} and got.n_loops > 20


@pytest.mark.parametrize("res", [0.25, 0.5])
def test_an_annulus_that_shrinks_vanishes_and_fragments(gpu, res):
    ref = S.pack(H.annulus())
    dev = upload(gpu, ref)
    got, _ = check(gpu, dev, ref, res, (0.0, 0.5, 1.0, 3.1, 2.9), "annulus")
    per_layer = np.bincount(got.loop_layer, minlength=5).tolist()
    assert per_layer[:4] == [2, 2, 2, 0] and per_layer[4] > 20
    got, _ = check(gpu, dev, ref, res, (-1.0,), "annulus out")
    assert got.n_loops == 2 and got.n_verts == (442 if res == 0.25 else 218)


# ---- many loops: ragged tiles, several batches of edges, tiles that no edge is near ---------------------------------------------------
def test_many_loops_over_ragged_tiles_and_batches_of_edges(gpu):
    ref = S.mixed_loops(n_loops=44, n_layers=2, seed=11)
    res, insets = F(1.5), (0.4, -0.7)
    want = twin("mixed", ref, res, insets)
    nx, ny = want.stats["nx"], want.stats["ny"]
    assert nx > 48 and ny > 48 and nx % 16 and ny % 16                     # at least 3 x 3 tiles, the last ones ragged
    per_layer = np.bincount(np.repeat(ref.loop_layer, np.diff(ref.loop_start.astype(np.int64))), minlength=2)
    assert per_layer.max() > 512 and all(n % 256 for n in per_layer)     # three batches of 256 edges, the last one ragged
    # some tile's near list is empty: no edge's box within band (and the kernel's margin, far below 1 %) of the tile's box
    a, b = O.layer_edges(ref, 0)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    reach = 1.01 * float(want.band)
    empty = 0
    for j0 in range(0, ny, 16):
        for i0 in range(0, nx, 16):
            x0, x1, y0, y1 = want.xs[i0], want.xs[min(i0 + 15, nx - 1)], want.ys[j0], want.ys[min(j0 + 15, ny - 1)]
            near = (lo[:, 0] <= x1 + reach) & (hi[:, 0] >= x0 - reach) & (lo[:, 1] <= y1 + reach) & (hi[:, 1] >= y0 - reach)
            empty += not near.any()
    assert empty > 0
    got, _ = check(gpu, upload(gpu, ref), ref, res, insets, "mixed")
    assert got.n_loops > 40


def test_a_comb_of_touching_loops(gpu):
    """Forty thin rectangles in a row, each touching the next: edges that coincide, crossings tied in x."""
    ref = H.comb(40)
    check(gpu, upload(gpu, ref), ref, 0.125, (0.125, 0.0, -0.25), "comb")


# ---- chunks, repeats, the handle's history ---------------------------------------------------------------------------------------------
def test_chunks_repeats_and_the_handle_s_history(gpu):
    ref = H.hand_loops()
    res, insets = 0.25, (-0.4, 0.0, 0.5, 1.0)
    dev = upload(gpu, ref)
    got, want = check(gpu, dev, ref, res, insets, "hand4", lattices=False)
    one_layer = want.stats["nx"] * want.stats["ny"]
    for max_nodes in (one_layer, 4 * one_layer, 9 * one_layer, 1):        # a chunk per input layer (one cannot split its insets), two layers
        again = dev.offset(res, insets, max_nodes)
        same(again, want, max_nodes)
        assert again.offset_stats.result_bytes() == got.offset_stats.result_bytes()
    # the source destroyed before the result is read through the library again
    out = dev.offset(res, insets)
    dev.close()
    fresh = gpu.ContourHIP(out._h)
    out._h = None
    same(fresh, want, "source destroyed")
    # every accessor works on the result: simplify, measures, sections, hatch, skin
    simp, st = fresh.simplify(0.05)
    assert 0 < st.n_verts_out < fresh.n_verts and simp.n_loops == fresh.n_loops
    w = S.Loops.of(want)
    loops, layers = fresh.measures()
    wl, wy = S.measures(w)
    assert loops.tobytes() == wl.tobytes() and layers.tobytes() == wy.tobytes()
    assert fresh.sections()[1]["area"].tolist() == layers["area"].tolist()
    h = fresh.hatch_dirs(0.5, H.directions((45.0, 135.0)))
    wh = H.hatch(w, 0.5, H.directions((45.0, 135.0)))
    assert h.seg.tobytes() == wh.seg.tobytes() and h.layer_start.tolist() == wh.layer_start.tolist()
    assert fresh.skin(0.5, (45.0, 135.0), 1, 1).n_segments > 0


def test_offsetting_an_offset_handle(gpu):
    ref = S.pack(H.annulus())
    first, want1 = check(gpu, upload(gpu, ref), ref, 0.25, (0.5,), "annulus once", lattices=False)
    ref2 = S.Loops.of(want1)
    second, _ = check(gpu, first, ref2, 0.25, (0.5, -0.5), "annulus twice")
    assert second.n_layers == 2 and second.n_loops == 4
    # a handle without loops gives a handle without loops
    none = upload(gpu, RECT).offset(0.5, (1.0,))
    assert (none.n_layers, none.n_loops, none.n_verts) == (1, 0, 0)
    empty = S.Loops(np.zeros((0, 2), F), [0], n_layers=1)
    got, want = check(gpu, none, empty, 0.5, (0.5, -1.0), "empty")
    assert (got.n_layers, got.n_loops) == (2, 0) and got.loop_start.tolist() == [0]
    assert got.hatch(0.5).n_segments == 0


@pytest.mark.parametrize("k", [40, -40])
def test_scaling_by_a_power_of_two(gpu, k):
    ref = H.hand_loops()
    insets = np.array((0.3, -0.4), F)
    base = twin("hand2", ref, 0.25, insets)
    sref = O.scaled(ref, k)
    got, want = check(gpu, upload(gpu, sref), sref, np.ldexp(F(0.25), k), np.ldexp(insets, k).astype(F), "hand2 2^%d" % k)
    assert got.loop_start.tolist() == base.loop_start.tolist() and got.xy.tobytes() == np.ldexp(base.xy, k).astype(F).tobytes()


# ---- a traced handle: offset once, then hatched and skinned -------------------------------------------------------------------------------
@pytest.mark.parametrize("rung", [0, 1, 2])
def test_a_traced_stack_offset_then_hatched_and_skinned(gpu, rung):
    s = Builder().Scene("bolt")
    bb = np.asarray(s.Bounds(), F)
    z = (bb[2] + (bb[5] - bb[2]) * np.array([0.23, 0.5, 0.81], F)).astype(F)
    res = res_for(bb, SLICE_LADDER[rung])
    src = gpu.ContourHIP.slices(gpu.SDF3HIP(s), res, z)
    inset = F(0.5) * res
    ref = S.Loops.of(src)
    got, want = check(gpu, src, ref, res, (inset,), "bolt %d" % rung, lattices=rung < 2)
    assert got.n_layers == 3 and np.bincount(got.loop_layer, minlength=3).min() >= 1
    # ends are computed in float64 and rounded once to float32: within a few float32 ulps of the inset loops, or strictly inside them;
    # and no fill closer to the part's own outline than the inset less the lattice spacing (the contract's vertex bound)
    ulp = 4 * float(np.abs(got.xy).max()) * 2.0 ** -24
    for h in (got.hatch(F(0.5) * res, (45.0, 135.0)), got.skin(F(0.5) * res, (45.0, 135.0), 1, 1)):
        assert h.n_segments > 0
        for l in range(3):
            seg = h.segments(l).astype(np.float64)
            ends = np.concatenate([seg[:, :2], seg[:, 2:]])
            loops = got.loops(l)
            a = np.concatenate(loops)
            b = np.concatenate([np.roll(q, -1, axis=0) for q in loops])
            on_boundary = S.seg_dist(ends, a, b) <= ulp
            assert (H.inside_even_odd(ends, loops) | on_boundary).all(), (l, int((~on_boundary).sum()))
            mid = 0.5 * (seg[:, :2] + seg[:, 2:])
            clear = S.seg_dist(mid, a, b) > ulp
            assert H.inside_even_odd(mid[clear], loops).all()
            sa, sb = O.layer_edges(ref, l)
            assert (S.seg_dist(ends, sa, sb) >= float(inset) - float(res) * (1 + 1e-6) - ulp).all()


# ---- errors ------------------------------------------------------------------------------------------------------------------------------
def test_every_error_of_the_contract(gpu):
    c = upload(gpu, RECT)
    for res in (0.0, -1.0, float("nan"), float("inf")):
        assert code(gpu, lambda: c.offset(res, (0.5,)))[0] == BAD_ARGUMENT, res
    assert code(gpu, lambda: c.offset(0.5, ()))[0] == BAD_ARGUMENT
    assert code(gpu, lambda: c.offset(0.5, (0.1,) * 9))[0] == BAD_ARGUMENT
    for v in (float("nan"), float("inf"), -float("inf")):
        assert code(gpu, lambda: c.offset(0.5, (0.5, v)))[0] == BAD_ARGUMENT, v
        assert code(gpu, lambda: c.distance(0.5, (v,), 0))[0] == BAD_ARGUMENT, v
    # the lattice's refusals: a quotient >= 2^31, nx ny >= 2^31, nx ny n_insets >= 2^31, a box that is not finite -- before any allocation
    for res, insets in ((1e-12, (0.5,)), (4e-5, (0.5,)), (1e-4, (0.1,) * 8), (0.5, (-3e38,))):
        assert code(gpu, lambda: c.offset(res, insets))[0] == BAD_ARGUMENT, (res, insets)
    assert code(gpu, lambda: c.distance(0.5, (0.5,), 1))[0] == BAD_ARGUMENT
    lib = gpu.lib()
    o = gpu.ContourHIP._offset_opts(0.5, (0.5,), 0, False)
    h = C.c_void_p()
    assert lib.gsdf_hip_contour_offset(c._h, C.byref(o), None, None) == BAD_ARGUMENT        # out NULL without dry
    o.reserved = 1
    assert lib.gsdf_hip_contour_offset(c._h, C.byref(o), C.byref(h), None) == BAD_ARGUMENT and not h.value
    d = np.zeros(12 * 8, F)
    assert lib.gsdf_hip_contour_distance(c._h, C.byref(o), 0, d.ctypes.data, None) == BAD_ARGUMENT
    o.reserved = 0
    assert lib.gsdf_hip_contour_distance(c._h, C.byref(o), 0, None, None) == BAD_ARGUMENT
    assert lib.gsdf_hip_contour_offset(None, C.byref(o), C.byref(h), None) == BAD_ARGUMENT and lib.gsdf_hip_contour_offset(c._h, None, C.byref(h), None) == BAD_ARGUMENT
    # 2^32 output layers: refused from the counts
    tall = gpu.ContourHIP.from_arrays(RECT.xy, RECT.loop_start, None, 2 ** 29)
    assert code(gpu, lambda: tall.offset(0.5, (0.1,) * 8))[0] == CAPACITY
    # nothing was changed by the refusals
    same(c.offset(0.5, (0.5,)), twin("rect one", RECT, 0.5, (0.5,)), "after the errors")
