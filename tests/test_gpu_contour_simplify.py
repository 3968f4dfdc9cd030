"""Loops after tracing on the device (gsdf_hip_contour_create / _simplify / _measures; gsdf_amd/csrc/kernels_contour_simplify.h)
against the CPU twin of the contract (tests/contoursimpref.py): coordinates, keys, loop starts, loop layers, the statistics' leading
block and the measures' records identical, as bytes -- hand loops at the 3 2^k edges and at every branch of q2, thousands of small
loops across workgroups, a circle that reaches level 16 (twice), the traced 2-D corpus and a stack of slices, dry runs, simplified
handles simplified again, an SVG round trip, the argument errors, simplify_to and the example."""
import importlib.util
import math
import os

import numpy as np
import pytest

import contourref
import contoursimpref as S
import corpus
from contourref import res_for
from scaffold.builder import Builder

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def upload(gpu, c):
    return gpu.ContourHIP.from_arrays(c.xy, c.loop_start, c.loop_layer, c.n_layers, c.keys)


def stats_bytes(gpu, st):
    """The twin's statistics as the leading block of a gsdf_contour_simplify_stats."""
    r = gpu.ContourSimplifyStats()
    r.n_verts_in, r.n_verts_out, r.n_loops, r.loops_changed = st["n_verts_in"], st["n_verts_out"], st["n_loops"], st["loops_changed"]
    for k, v in enumerate(st["spans"]):
        r.spans[k] = v
    r.max_level, r.max_dev = st["max_level"], st["max_dev"]
    return r.result_bytes()


def same_loops(dev, ref, what):
    assert (dev.n_layers, dev.n_loops, dev.n_verts) == (ref.n_layers, len(ref.loop_layer), len(ref.xy)), what
    for f in ("keys", "loop_start", "loop_layer", "xy"):
        a, b = getattr(dev, f), getattr(ref, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero((a.reshape(len(a), -1).view(np.uint32) != b.reshape(len(b), -1).view(np.uint32)).any(axis=1))
            raise AssertionError((what, f, len(bad), bad[:5].tolist(), a[bad[:3]].tolist(), b[bad[:3]].tolist()))
    st = dev.stats
    assert (st.n_verts, st.n_loops, st.n_layers) == (dev.n_verts, dev.n_loops, dev.n_layers), what
    assert bytes(st)[16:48] == bytes(32) and bytes(st)[48:56] == bytes(8) and bytes(st)[60:] == bytes(len(bytes(st)) - 60), what  # every other integer 0, the times 0


def check(gpu, dev, ref, tol, levels=8, passes=1, what=None):
    """Simplify on the device and in the twin: the same loops, the same leading block; the dry run says the same and builds nothing."""
    want, st = S.simplify(ref, tol, levels, passes)
    got, dst = dev.simplify(tol, levels, passes)
    same_loops(got, want, what)
    assert dst.result_bytes() == stats_bytes(gpu, st), (what, [getattr(dst, f) for f in ("n_verts_in", "n_verts_out", "n_loops", "loops_changed", "max_level", "max_dev")],
                                                        list(dst.spans), st)
    assert dst.ms_device > 0 or dev.n_loops == 0, what
    none, dry = dev.simplify(tol, levels, passes, dry=True)
    assert none is None and dry.result_bytes() == dst.result_bytes(), what
    return got, want, st


def check_measures(dev, ref, what):
    loops, layers = dev.measures()
    rl, ry = S.measures(ref)
    assert loops.dtype == rl.dtype and layers.dtype == ry.dtype
    assert loops.tobytes() == rl.tobytes(), (what, np.flatnonzero(loops != rl)[:5].tolist())
    assert layers.tobytes() == ry.tobytes(), (what, layers, ry)


# ---- hand loops ----------------------------------------------------------------------------------------------------------------------
def test_loop_sizes_at_the_level_edges(gpu):
    """n = 3 .. 25 around 3 2^k (kmax changes at 6, 12, 24); 13 and 25 also cut the last span short at n, so that it ends at the leader."""
    sizes = [3, 4, 5, 6, 7, 11, 12, 13, 24, 25]
    loops = [S.circle(n, 1.0 + n) for n in sizes] + [S.rectangle(3, 3)[:n] for n in (11, 12)] + [S.rectangle(7, 6)[:25], S.rectangle(6, 7)]
    ref = S.pack(loops, [0] * 8 + [1] * 4 + [3] * 2, 5)
    dev = upload(gpu, ref)
    same_loops(dev, ref, "upload")
    for tol in (0.0, 0.01, 0.3, 2.0, np.inf):
        for levels in (1, 2, 3, 8):
            check(gpu, dev, ref, F(tol), levels, 1, ("sizes", tol, levels))
    _, want, st = check(gpu, dev, ref, np.inf, 16, 1, "sizes, inf")
    assert np.diff(want.loop_start.astype(np.int64))[:10].tolist() == [-(-n // (1 << S.kmax_of(n, 16))) for n in sizes]
    check_measures(dev, ref, "sizes")


def test_every_branch_of_q2_and_the_exact_boundary(gpu):
    up = float(np.nextafter(F(0.5), F(1)))
    # a = (0, 0), b = (8, 0) is the span (1, 0) of a 6-vertex loop; its one interior vertex is p
    on = np.array([(0, 0), (4, 0.5), (8, 0), (8, 6), (4, 7), (0, 6)], F)
    over = on.copy()
    over[1, 1] = up
    behind = on.copy()
    behind[1] = (-0.5, 0.0)      # t <= 0: the distance to a, 0.5 exactly
    beyond = on.copy()
    beyond[1] = (8.5, 0.0)       # t >= dd: the distance to b
    # a hairpin, and a span whose two ends have equal coordinates (dd == 0)
    hairpin = np.array([(0, 0), (9, 0.25), (0.5, 0.5), (-3, 0.25), (4, 0), (4, 5), (2, 6), (0, 5), (-1, 3), (0, 2), (-0.5, 1), (0.25, 0.5)], F)
    closed = np.array([(1, 1), (1.25, 1.25), (1, 1), (5, 1), (5, 5), (1, 5)], F)
    ref = S.pack([on, over, behind, beyond, hairpin, closed])
    dev = upload(gpu, ref)
    got, want, st = check(gpu, dev, ref, F(0.5), 8, 1, "boundary")
    kept = np.diff(want.loop_start.astype(np.int64)).tolist()
    assert kept[0] == 5 and kept[1] == 6, kept                    # q2 == tol2 == 0.25 is dropped, the next float32 above is kept
    assert kept[2] == 5 and kept[3] == 5 and kept[5] == 5, kept    # both end branches at exactly tol; dd == 0 within tol
    assert st["max_dev"] == 0.5
    for tol in (0.0, 0.25, 0.36, 1.0, 8.0):
        for passes in (1, 2):
            check(gpu, dev, ref, F(tol), 8, passes, ("branches", tol, passes))
    check_measures(dev, ref, "branches")


# ---- scale ---------------------------------------------------------------------------------------------------------------------------
def test_thousands_of_small_loops_across_blocks(gpu):
    ref = S.mixed_loops(3000, 5)
    assert len(ref.xy) > 100 * 256 and len(set(ref.loop_layer.tolist())) == 5
    dev = upload(gpu, ref)
    for tol, passes in ((0.0, 1), (0.02, 1), (0.02, 3), (0.5, 2)):
        got, want, st = check(gpu, dev, ref, F(tol), 8, passes, ("mixed", tol, passes))
    assert 0 < st["loops_changed"] and st["n_verts_out"] < st["n_verts_in"]
    check_measures(dev, ref, "mixed")
    check_measures(got, want, "mixed, simplified")


def test_a_circle_that_reaches_level_16_twice(gpu):
    ref = S.pack([S.circle(200_000, 1000.0)])
    dev = upload(gpu, ref)
    _, _, st = check(gpu, dev, ref, F(600.0), 16, 1, "circle, every level")     # (a span of level 16 bulges 485 from its chord)
    assert st["max_level"] == 16 and st["n_verts_out"] == 4
    a, want, st = check(gpu, dev, ref, F(0.75), 16, 1, "circle")
    assert st["max_level"] >= 10 and st["n_verts_out"] < 1000
    b, _ = dev.simplify(F(0.75), 16, 1)
    for f in ("xy", "keys", "loop_start", "loop_layer"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), f
    la, lb = dev.measures(), dev.measures()
    assert la[0].tobytes() == lb[0].tobytes() and la[1].tobytes() == lb[1].tobytes()
    check_measures(dev, ref, "circle")
    assert abs(la[0][0]["area"] / (math.pi * 1e6) - 1) < 1e-6 and abs(la[0][0]["length"] / (2000 * math.pi) - 1) < 1e-6


# ---- through the pipeline ------------------------------------------------------------------------------------------------------------
def test_corpus_outlines(gpu):
    total = dropped = 0
    for name, s in corpus.shapes2d()[1]:
        sdf = gpu.SDF2HIP(s)
        res = res_for(sdf.Bounds(), 40)
        dev = gpu.ContourHIP.outline(sdf, res)
        before = (dev.xy.tobytes(), dev.keys.tobytes(), dev.loop_start.tobytes(), dev.stats.result_bytes())
        ref = S.Loops.of(dev)
        for passes in (1, 3):
            got, want, st = check(gpu, dev, ref, F(res / F(8)), 8, passes, (name, passes))
        total, dropped = total + st["n_verts_in"], dropped + st["n_verts_in"] - st["n_verts_out"]
        check_measures(dev, ref, name)
        check_measures(got, want, (name, "simplified"))
        # simplifying a simplified handle; the traced handle is as it was
        check(gpu, got, want, F(res / F(4)), 8, 1, (name, "again"))
        assert before == (dev.xy.tobytes(), dev.keys.tobytes(), dev.loop_start.tobytes(), dev.stats.result_bytes())
        if dev.n_loops:
            # (the host's float64 shoelace sum rounds n terms of up to max |x y| each: far above the device's quantisation)
            assert np.allclose(dev.measures()[0]["area"], dev.areas(), rtol=0, atol=dev.n_verts * 2.0 ** -50 * float(np.abs(dev.xy).max()) ** 2)
    assert 4 * dropped >= total > 4000, (dropped, total)


def test_slices_of_a_part_and_an_empty_layer(gpu):
    s = Builder().Scene("bolt")
    bb = s.Bounds()
    res = F(float(s.Diagonal()) / 60)
    z = contourref.layer_heights(bb, F(F(bb[5] - bb[2]) / F(7)))
    dev = gpu.ContourHIP.slices(gpu.SDF3HIP(s), res, z)
    ref = S.Loops.of(dev)
    assert dev.n_layers == 7 and 0 not in set(dev.loop_layer.tolist())     # the lowest mid-height meets no material: a layer without loops
    for passes in (1, 3):
        got, want, _ = check(gpu, dev, ref, F(res / F(8)), 8, passes, ("bolt", passes))
    check_measures(dev, ref, "bolt")
    check_measures(got, want, "bolt, simplified")
    layers = dev.measures()[1]
    assert layers[0]["n_loops"] == 0 and layers[0]["bbox"].tolist() == [np.inf, np.inf, -np.inf, -np.inf] and layers[0]["area"] == 0


def test_no_loops_at_all(gpu):
    b = Builder()
    s = b.Intersection2D(b.Translate2D(b.NewCircle(0.4), 0.45, 1), b.NewRectangle(1, 0.61))
    dev = gpu.ContourHIP.outline(gpu.SDF2HIP(s), F(0.1))
    got, st = dev.simplify(0.1)
    assert (got.n_loops, got.n_verts, got.n_layers, got.loop_start.tolist()) == (0, 0, 1, [0]) and st.n_verts_out == 0 and st.max_dev == 0
    loops, layers = dev.measures()
    assert len(loops) == 0 and layers[0]["n_loops"] == 0 and layers[0]["length"] == 0


def test_svg_of_a_simplified_handle_reads_back(gpu, tmp_path):
    from gsdf_amd import svg
    spec = importlib.util.spec_from_file_location("render_png", os.path.join(ROOT, "examples", "render_png.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sdf = gpu.SDF2HIP(mod.scene("text"))
    res = res_for(sdf.Bounds(), 150)
    dev = gpu.ContourHIP.outline(sdf, res)
    got, st = dev.simplify(F(res / F(8)), passes=2)
    assert st.n_verts_out < dev.n_verts
    path = str(tmp_path / "text.svg")
    svg.write_svg(path, [got.loops(k) for k in range(got.n_layers)])
    back = svg.read_svg(path)
    assert len(back) == 1 and len(back[0]) == got.n_loops
    assert np.concatenate(back[0]).tobytes() == got.xy.tobytes()
    again = gpu.ContourHIP.from_arrays(np.concatenate(back[0]), np.concatenate([[0], np.cumsum([len(l) for l in back[0]])]))
    assert again.measures()[0].tobytes() == got.measures()[0].tobytes()


# ---- errors and composition ----------------------------------------------------------------------------------------------------------
def test_argument_errors(gpu):
    import ctypes as C
    c = upload(gpu, S.pack([S.circle(40)]))
    BAD_ARGUMENT, EMPTY = -3, -1

    def code(fn):
        with pytest.raises(gpu.HipError) as e:
            fn()
        return e.value.code

    for tol in (-1.0, float("nan"), -float("inf")):
        assert code(lambda: c.simplify(tol)) == BAD_ARGUMENT, tol
    assert code(lambda: c.simplify(0.1, levels=17)) == BAD_ARGUMENT
    assert code(lambda: c.simplify(0.1, passes=9)) == BAD_ARGUMENT
    o = gpu.ContourSimplifyOpts(F(0.1), 0, 0, 0)
    L = gpu.lib()
    assert L.gsdf_hip_contour_simplify(c._h, C.byref(o), None, None) == BAD_ARGUMENT          # out NULL without dry
    assert L.gsdf_hip_contour_simplify(c._h, None, None, None) == BAD_ARGUMENT
    assert L.gsdf_hip_contour_measures(None, None, None) == BAD_ARGUMENT
    o.dry = 1
    h = C.c_void_p(12345)
    assert L.gsdf_hip_contour_simplify(c._h, C.byref(o), C.byref(h), None) == 0 and not h.value  # dry: nothing built, out set to NULL
    # levels 0 and passes 0 are the defaults 8 and 1
    a, b = c.simplify(0.2, 0, 0)[0], c.simplify(0.2, 8, 1)[0]
    assert a.xy.tobytes() == b.xy.tobytes() and a.n_verts < 40
    xy = S.circle(8)
    assert code(lambda: gpu.ContourHIP.from_arrays(xy[:0], [0])) == EMPTY
    assert code(lambda: gpu.ContourHIP.from_arrays(xy, [0, 2, 8])) == BAD_ARGUMENT
    assert code(lambda: gpu.ContourHIP.from_arrays(xy, [0, 4, 8], [1, 0], 2)) == BAD_ARGUMENT
    assert code(lambda: gpu.ContourHIP.from_arrays(xy, [0, 4, 8], [0, 1], 1)) == BAD_ARGUMENT
    bad = xy.copy()
    bad[3, 0] = np.nan
    assert code(lambda: gpu.ContourHIP.from_arrays(bad, [0, 8])) == BAD_ARGUMENT
    assert c.simplify(np.inf)[0].n_verts == -(-40 // 8)                                        # tol = +Inf is allowed


def test_simplify_to_ends_at_or_under_its_count(gpu):
    ref = S.mixed_loops(300, 2)
    dev = upload(gpu, ref)
    floor = dev.simplify(np.inf, dry=True)[1].n_verts_out
    for max_verts in (dev.n_verts, dev.n_verts // 2, floor + 50, floor):
        got, st, tol = dev.simplify_to(max_verts, 1e-4)
        assert got.n_verts == st.n_verts_out <= max_verts
        if tol > F(1e-4):
            assert dev.simplify(F(tol / F(2)), dry=True)[1].n_verts_out > max_verts             # the first tol of the doubling that fits
        same_loops(got, S.simplify(ref, tol)[0], ("simplify_to", max_verts))
    with pytest.raises(ValueError):
        dev.simplify_to(floor - 1, 1e-4)
    with pytest.raises(ValueError):
        dev.simplify_to(10, 0.0)


def test_the_example_end_to_end(gpu, tmp_path, capsys):
    from gsdf_amd import svg
    spec = importlib.util.spec_from_file_location("render_svg", os.path.join(ROOT, "examples", "render_svg.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    plain, simple = str(tmp_path / "a.svg"), str(tmp_path / "b.svg")
    assert mod.main(["text", "--resdiv", "120", "--interpreter", "-o", plain]) == 0
    assert mod.main(["text", "--resdiv", "120", "--interpreter", "--simplify", "0.125", "--report", "-o", simple]) == 0
    out = capsys.readouterr().out
    assert "max_dev" in out and "simplified" in out
    a, b = svg.read_svg(plain)[0], svg.read_svg(simple)[0]
    assert len(a) == len(b) and sum(map(len, b)) < sum(map(len, a))
    sdf = gpu.SDF2HIP(mod.scene("text"))
    tol = float(mod.spacing(sdf.Bounds(), False, 120.0)) * 0.125
    for old, new in zip(a, b):
        h_on, h_no = S.hausdorff(old, new)
        assert h_on <= tol * (1 + 1e-6) and h_no <= tol * (1 + 1e-6)
    capped = str(tmp_path / "c.svg")
    assert mod.main(["text", "--resdiv", "120", "--interpreter", "--simplify", "0.01", "--max-verts", "400", "-o", capped]) == 0
    assert sum(map(len, svg.read_svg(capped)[0])) <= 400
