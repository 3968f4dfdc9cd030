"""Every consumer of a gsdf_contour handle on the device against its CPU twin, as bytes, on the ground of tests/loop_corpus.py: what
gsdf_hip_contour_create accepts and no slicer produces -- repeated vertices, loops that are a point or lie on a line, bow-ties, the
same loop twice, vertices exactly on hatch lines and on the offset's lattice nodes, raw directions that are no unit vectors, 300
layers of which 292 are empty, and counts that are exact multiples of a wave, a workgroup, a tile and a batch. Measures, sections,
simplify, hatch, skin, offset and distance run on every case; the comparisons are those of the consumers' own test files
(test_gpu_contour_simplify, test_gpu_mass, test_gpu_hatch, test_gpu_skin, test_gpu_offset), imported, so each is byte identity of
every output array and of the statistics' leading block, with the dry run. Nowhere is there a tolerance. What the corpus reaches is
stated, on the twins, in tests/test_loop_corpus_ref.py."""
import numpy as np
import pytest

import contoursimpref as S
import loop_corpus as LC
import test_gpu_contour_simplify as TS
import test_gpu_hatch as TH
import test_gpu_mass as TM
import test_gpu_offset as TO
import test_gpu_skin as TK

pytestmark = pytest.mark.gpu

F = np.float32


def upload(gpu, c):
    return gpu.ContourHIP.from_arrays(c.xy, c.loop_start, c.loop_layer, c.n_layers, c.keys)


def step(name, consumer, fn):
    """One consumer on one case: a failure names both, whatever the comparison's own message says."""
    try:
        return fn()
    except Exception as e:          # (a comparison that fails, or the library's own error)
        raise AssertionError(("loop corpus", name, consumer, repr(e)[:300])) from e


def offset_and_distance(gpu, dev, c, name, k, res, insets, layers=None):
    """TO.check with the D lattice of every layer, or (layers given) of those layers alone."""
    what = "%s / offset %d" % (name, k)
    if layers is None:
        return TO.check(gpu, dev, c, res, insets, what)
    got, want = TO.check(gpu, dev, c, res, insets, what, lattices=False)
    for l in layers:
        d = dev.distance(res, insets, l)
        assert d.shape == want.D[l].shape and d.tobytes() == want.D[l].tobytes(), (what, l, np.argwhere(d.view(np.uint32) != want.D[l].view(np.uint32))[:5].tolist())
    return got, want


def every_consumer(gpu, name, c, hand=False, tall=False, offsets=(), lattice_layers=None):
    """The table of the module's docstring on one stack; returns the handle and the twins' hatch, skin and offset results."""
    dev = step(name, "upload", lambda: upload(gpu, c))
    step(name, "upload", lambda: TS.same_loops(dev, c, name))
    step(name, "measures", lambda: TS.check_measures(dev, c, name))
    step(name, "sections", lambda: TM.check_sections(gpu, c.xy, c.loop_start, c.loop_layer, c.n_layers, name, dev))
    for tol, passes in LC.SIMPLIFIES:
        step(name, ("simplify", tol, passes), lambda: TS.check(gpu, dev, c, F(tol), 8, passes, (name, "simplify", tol, passes)))
    seen = {}
    for k, (sp, dirs, off) in enumerate(LC.HATCHES):
        seen["hatch", k] = step(name, ("hatch", k), lambda: TH.check(gpu, dev, c, sp, dirs, off, (name, "hatch", k)))[1]
    for k, (sp, dirs, below, above, off) in enumerate(LC.SKINS + ((LC.TALL_SKIN,) if tall else ())):
        seen["skin", k] = step(name, ("skin", k), lambda: TK.check(gpu, dev, c, sp, dirs, below, above, off, (name, "skin", k)))[1]
    for k, (res, insets) in enumerate(LC.OFFSETS + ((LC.EIGHT_INSETS,) if hand else ()) + tuple(offsets)):
        seen["offset", k] = step(name, ("offset", k), lambda: offset_and_distance(gpu, dev, c, name, k, res, insets, lattice_layers))[1]
    # the handle is what it was
    step(name, "the handle afterwards", lambda: TS.same_loops(dev, c, name))
    return dev, seen


# ---- the generator's seeds -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("first", range(0, 64, 8))
def test_grid_loops_eight_seeds_at_a_time(gpu, first):
    """Seeds first .. first + 7 (0 .. 63 over the eight cases; none skipped or filtered), every consumer on each. Every group reaches
    zero-length pieces in the hatch and exact zeros of both signs in D, so that no group passes on tame input alone."""
    zero_length = signed_zeros = 0
    for seed in range(first, first + 8):
        _, seen = every_consumer(gpu, "grid_loops(%d)" % seed, LC.grid_loops(seed))
        zero_length += sum(seen["hatch", k].stats["zero_length"] for k in range(len(LC.HATCHES)))
        signed_zeros += sum(int(((D == 0) & np.signbit(D)).sum()) for D in seen["offset", 0].D)
    assert zero_length > 0 and signed_zeros > 0


@pytest.mark.parametrize("first", range(0, 16, 8))
def test_grid_loops_with_negative_zero_coordinates(gpu, first):
    """loop_corpus.negative_zeros of the seeds first .. first + 7: crossings at one place that differ in the sign bit of a zero, so the
    order inside a tie group of the skin, (r, j), shows in the segments' bytes (test_loop_corpus_ref states it)."""
    for seed in range(first, first + 8):
        every_consumer(gpu, "negative_zeros(grid_loops(%d))" % seed, LC.negative_zeros(LC.grid_loops(seed)))


# ---- hand cases ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LC.hand_cases()))
def test_hand_cases(gpu, name):
    c = LC.hand_cases()[name]
    dev, seen = every_consumer(gpu, name, c, hand=True)
    if name == "point":
        # the closed form of the twin's own test, from the device: the distance to the point, +0.0 at the node that is the point
        for res, insets in LC.OFFSETS + (LC.EIGHT_INSETS,):
            d = dev.distance(res, insets, 0)
            assert not np.isnan(d).any() and not np.signbit(d).any() and (d == 0).sum() == 1
    if name in ("doubled", "reversed"):
        for k in range(len(LC.HATCHES)):
            st = dev.hatch_dirs(*LC.HATCHES[k][:2], LC.HATCHES[k][2]).stats
            assert st.length == 0.0 and st.zero_length == st.n_segments > 0
        assert dev.offset(*LC.OFFSETS[0]).offset_stats.inside_nodes == 0
    if name == "stack":
        assert seen["skin", 1].stats["zero_length"] > 0 and seen["hatch", 0].stats["zero_length"] > 0


# ---- 300 layers ------------------------------------------------------------------------------------------------------------------------
def test_the_tall_stack(gpu):
    """Kernels that run a layer per lane, and per-layer records, past the first wave and the first workgroup of 256: layers 63 .. 65
    and 255 .. 257 occupied, 299 the last. The D lattices are read for the eight occupied layers and two empty ones (1 and 254) only:
    a lattice costs a device pass over all 300 layers, and the empty ones are all alike (the band everywhere)."""
    c = LC.tall_stack()
    dev, seen = every_consumer(gpu, "tall_stack", c, tall=True, lattice_layers=LC.TALL_OCCUPIED + LC.TALL_EMPTY_READ)
    wide = seen["skin", len(LC.SKINS)]
    assert (wide.cls == 3).all() and np.flatnonzero(np.diff(wide.layer_start.astype(np.int64))).tolist() == list(LC.TALL_OCCUPIED)
    got = dev.skin_dirs(*LC.SKINS[0][:4], LC.SKINS[0][4])
    for l, classes in ((64, {0, 2}), (256, {0, 1})):
        assert set(got.cls[got.layer_start[l]:got.layer_start[l + 1]].tolist()) == classes, l
    for l in LC.TALL_EMPTY_READ:
        assert (seen["offset", 0].D[l] == seen["offset", 0].band).all()


# ---- boundary sizes ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LC.boundary_cases()))
def test_boundary_sizes(gpu, name):
    """Counts that are exact multiples (loop_corpus.boundary_cases asserts each): a batch loop that ends with a full batch, a lattice
    with no ragged tile and one with a single node beyond, line buckets of exactly 64 and 256 records (192 and 768 in the skin), a
    handle of exactly a workgroup of vertices and one whose last loop closes from workgroup 1 back into workgroup 0."""
    c = LC.boundary_cases()[name]
    tiles = name.startswith("tiles")
    dev, seen = every_consumer(gpu, name, c, offsets=(LC.TILE_INSETS,) if tiles else ())
    if tiles:
        st = seen["offset", len(LC.OFFSETS)].stats
        assert (st["nx"] % 16, st["ny"] % 16) == ((0, 0) if "32" in name else (1, 1)) and st["n_loops"] >= 4
    if name.startswith("comb "):
        assert seen["hatch", 0].stats["max_line_crossings"] == 2 * int(name.split()[1])
    if name.startswith("combs "):
        _, want = step(name, "skin, one direction", lambda: TK.check(gpu, dev, c, 1.0, [(1.0, 0.0)], 1, 1, 0.0, (name, "skin, one direction")))
        assert want.stats["max_line_crossings"] == 6 * int(name.split()[1])


# ---- one chain -------------------------------------------------------------------------------------------------------------------------
def test_a_degenerate_stack_offset_then_simplified_then_hatched_and_skinned(gpu):
    """grid_loops(5) offset, the result simplified at tol 0, that hatched and skinned: every step against the twins chained the same
    way (as test_gpu_offset.test_chunks_repeats_and_the_handle_s_history does for hand loops)."""
    name = "chain of grid_loops(5)"
    c = LC.grid_loops(5)
    res, insets = 0.5, (0.0, 0.25)
    moved, want = step(name, "offset", lambda: TO.check(gpu, upload(gpu, c), c, res, insets, name))
    assert want.stats["n_loops"] > 4 and want.stats["saddle_cells"] > 0
    ref1 = S.Loops.of(want)
    simple, ref2, st = step(name, "simplify", lambda: TS.check(gpu, moved, ref1, F(0.0), 8, 1, name))
    assert st["n_verts_out"] < st["n_verts_in"]
    step(name, "measures", lambda: TS.check_measures(simple, ref2, name))
    step(name, "sections", lambda: TM.check_sections(gpu, ref2.xy, ref2.loop_start, ref2.loop_layer, ref2.n_layers, name, simple))
    for k, (sp, dirs, off) in enumerate(LC.HATCHES):
        _, h = step(name, ("hatch", k), lambda: TH.check(gpu, simple, ref2, sp, dirs, off, (name, "hatch", k)))
    assert h.stats["n_segments"] > 0
    for k, (sp, dirs, below, above, off) in enumerate(LC.SKINS):
        _, s = step(name, ("skin", k), lambda: TK.check(gpu, simple, ref2, sp, dirs, below, above, off, (name, "skin", k)))
    assert s.stats["n_segments"] > 0
    step(name, "offset again", lambda: TO.check(gpu, simple, ref2, res, (0.25,), name + ", again"))
