"""The CPU twin of the loops' simplification and measures (tests/contoursimpref.py, written from the section "contours: simplify and
measures" of include/gsdf_hip.h), held to what that section derives: the Hausdorff and area bounds by brute force, the floor of
vertices per loop, leaders and loop order, monotony in tol and levels, what tol 0 and tol +Inf do, the measures against float64 sums
within the quantisation bound -- over the traced outlines of the 2-D corpus and over hand loops. And the ABI's struct layouts and
host-side argument checks, which need no device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import contourref
import contoursimpref as S
import corpus
from contourref import res_for
from oracle.oracle import OracleSDF

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def outlines():
    """The traced outlines of the 2-D corpus that have loops: [(name, res, Loops)]."""
    out = []
    for name, s in corpus.shapes2d()[1]:
        o = OracleSDF(s.tree())
        res = res_for(o.Bounds(), 40)
        c = contourref.contour(o.Evaluate, o.Bounds(), res)
        if c.stats["n_loops"]:
            out.append((name, res, S.Loops.of(c)))
    assert len(out) >= 40
    return out


def hand_loops():
    rng = np.random.default_rng(3)
    loops = {"rect": S.rectangle(40, 23), "circle": S.circle(1000), "small": S.circle(7)}
    th = np.sort(rng.uniform(0, 2 * math.pi, 777))
    loops["noisy"] = (np.stack([np.cos(th), np.sin(th)], 1) * (1 + 0.002 * rng.standard_normal((777, 1)))).astype(F)
    loops["hairpin"] = np.array([(0, 0), (4, 0.01), (8, 0), (3, 0.02), (-2, 0.01), (9, 0.03), (9, 5), (0, 5), (0, 3), (-1, 2), (0, 1), (0.5, 0.5)], F)
    return loops


def check_guarantees(old, new, st, tol, levels, passes, what):
    assert (new.loop_layer == old.loop_layer).all() and len(new.loop_start) == len(old.loop_start), what
    assert new.loop_start[0] == 0 and new.loop_start[-1] == len(new.xy) == st["n_verts_out"], what
    slack = passes * float(tol) * (1 + 1e-9) + 1e-12 * float(np.abs(old.xy).max())
    for q, (a, b) in enumerate(zip(old.loops(), new.loops())):
        n = len(a)
        floor = -(-n // (1 << S.kmax_of(n, levels))) if passes == 1 else 3
        assert len(b) >= max(floor, 3) and len(b) <= n, (what, q)
        assert (b[0].view(np.uint32) == a[0].view(np.uint32)).all(), (what, q)       # the leader stays
        # kept vertices are old vertices, bit for bit and in order
        ka, kb = old.keys[old.loop_start[q]:old.loop_start[q + 1]], new.keys[new.loop_start[q]:new.loop_start[q + 1]]
        rows = {(int(x), int(y), int(k)) for (x, y), k in zip(a.view(np.uint32), ka)}
        assert all((int(x), int(y), int(k)) in rows for (x, y), k in zip(b.view(np.uint32), kb)), (what, q)
        if np.isfinite(tol):
            h_on, h_no = S.hausdorff(a, b)
            assert h_on <= slack and h_no <= slack, (what, q, h_on, h_no, slack)
            assert abs(contourref.area(a) - contourref.area(b)) <= slack * contourref.perimeter(a) + 1e-12, (what, q)
    assert st["max_dev"] <= float(tol) or not np.isfinite(tol), what


def test_corpus_bounds_and_share(outlines):
    """Hausdorff <= passes tol both ways, |area change| <= tol perimeter, >= 3 vertices, leaders and order kept, on every outline of the
    corpus at res = diag / 40, tol = res / 8, passes 1 and 3. So that the device comparison over the same outlines cannot be vacuous: at
    tol = res / 8 and one pass the twin drops at least a quarter of all the corpus's vertices (measured: 3165 of 4648, 68.1 %)."""
    total = dropped = 0
    for name, res, c in outlines:
        tol = F(res / F(8))
        for passes in (1, 3):
            new, st = S.simplify(c, tol, 8, passes)
            check_guarantees(c, new, st, tol, 8, passes, (name, passes))
            if passes == 1:
                total += st["n_verts_in"]
                dropped += st["n_verts_in"] - st["n_verts_out"]
    print("corpus: dropped %d of %d vertices at tol = res / 8" % (dropped, total))
    assert 4 * dropped >= total, (dropped, total)


@pytest.mark.parametrize("name", sorted(hand_loops()))
def test_hand_loops_bounds(name):
    c = S.pack([hand_loops()[name]])
    for tol in (0.0, 1e-3, 0.05, 0.5):
        for levels in (1, 3, 16):
            for passes in (1, 2):
                new, st = S.simplify(c, F(tol), levels, passes)
                check_guarantees(c, new, st, F(tol), levels, passes, (name, tol, levels, passes))


def test_monotone_in_tol_and_levels(outlines):
    loops = [c for _, _, c in outlines[:12]] + [S.pack([l]) for l in hand_loops().values()]
    for c in loops:
        prev = None
        for tol in (0.0, 1e-4, 1e-3, 1e-2, 1e-1, 1.0, np.inf):
            keep = S.one_pass(c.xy, c.loop_start, float(F(tol)) ** 2, 8)[0]
            assert prev is None or not (keep & ~prev).any()      # what a smaller tol dropped stays dropped
            prev = keep
        prev = None
        for levels in range(1, 17):
            keep = S.one_pass(c.xy, c.loop_start, 1e-4, levels)[0]
            assert prev is None or not (keep & ~prev).any()
            prev = keep


def test_tol_zero_drops_exactly_the_collinear():
    """tol 0: a vertex goes iff its q2 against the chord of some span is exactly 0. A rectangle's sides are exactly collinear (their
    coordinates are multiples of 1/8): everything but the span ends goes; a second pass at tol 0 leaves the corners and little else."""
    r = S.rectangle(37, 41)
    c = S.pack([r])
    new, st = S.simplify(c, 0.0, 8, 1)
    assert st["max_dev"] == 0.0 and st["loops_changed"] == 1
    assert [S.simplify(c, 0.0, 8, p)[1]["n_verts_out"] for p in (1, 2, 3)] == [19, 10, 6]     # the header's example: 156 vertices
    keep = S.one_pass(c.xy, c.loop_start, 0.0, 8)[0]
    for j in np.flatnonzero(~keep):                                  # every dropped vertex lies on a side, between kept ones
        a, b = r[j - 1].astype(np.float64), r[(j + 1) % len(r)].astype(np.float64)
        p = r[j].astype(np.float64)
        assert (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0]) == 0.0
    corners = {(0.0, 0.0), (4.625, 0.0), (4.625, 5.125), (0.0, 5.125)}
    assert corners <= {tuple(map(float, p)) for p in new.xy}
    new3, st3 = S.simplify(c, 0.0, 8, 3)
    assert corners <= {tuple(map(float, p)) for p in new3.xy}
    # a circle has no three collinear vertices: tol 0 drops nothing
    new, st = S.simplify(S.pack([S.circle(500)]), 0.0, 16, 2)
    assert st["n_verts_out"] == 500 and st["loops_changed"] == 0 and sum(st["spans"]) == 0 and st["max_level"] == 0


@pytest.mark.parametrize("levels", [1, 4, 8, 16])
def test_tol_inf_leaves_the_floor(levels):
    sizes = [3, 4, 5, 6, 7, 11, 12, 13, 24, 25, 100, 257, 1000, 8191]
    c = S.pack([S.circle(n, 2.0 + n) for n in sizes])
    new, st = S.simplify(c, np.inf, levels, 1)
    for n, got in zip(sizes, np.diff(new.loop_start.astype(np.int64))):
        k = S.kmax_of(n, levels)
        assert got == -(-n // (1 << k)) >= 3, (n, levels)
        assert (k == 0) == (n < 6)
    assert st["loops_changed"] == sum(1 for n in sizes if n >= 6)


def test_measures_against_float64(outlines):
    """area and length of every loop against the float64 shoelace sum and perimeter: within the quantisation bound of the header
    (n / 2 units of 2^(2e-62) resp. 2^(e-60)) plus the float64 summation error of the comparison itself; boxes exactly."""
    cases = [c for _, _, c in outlines] + [S.mixed_loops(200, 3), S.pack([S.circle(5000, 1e-3), S.circle(9, 1e6)], [0, 2], 4)]
    for c in cases:
        loops, layers = S.measures(c)
        e = S.exponent(c.xy)
        for q, l in enumerate(c.loops()):
            n = len(l)
            ref_a, ref_l = contourref.area(l), contourref.perimeter(l)
            assert abs(loops[q]["area"] - ref_a) <= n / 2 * 2.0 ** (2 * e - 62) + 4 * n * 2.0 ** -53 * (abs(l[:, 0]).max() * abs(l[:, 1]).max() * n)
            assert abs(loops[q]["length"] - ref_l) <= n / 2 * 2.0 ** (e - 60) + 4 * n * 2.0 ** -53 * ref_l
            assert loops[q]["bbox"].tolist() == [l[:, 0].min(), l[:, 1].min(), l[:, 0].max(), l[:, 1].max()]
            assert loops[q]["n_verts"] == n and loops[q]["layer"] == c.loop_layer[q]
        for lay in range(c.n_layers):
            m = c.loop_layer == lay
            assert layers[lay]["n_loops"] == m.sum() and layers[lay]["n_verts"] == loops["n_verts"][m].sum()
            assert math.isclose(layers[lay]["area"], loops["area"][m].sum(), rel_tol=1e-12, abs_tol=2.0 ** (2 * e - 40))
            if not m.any():
                assert layers[lay]["bbox"].tolist() == [np.inf, np.inf, -np.inf, -np.inf] and layers[lay]["area"] == 0 and layers[lay]["length"] == 0
    # order independence: the loop's sums do not depend on where the loop starts
    l = S.circle(1234, 7.0)
    a = S.measures(S.pack([l]))[0][0]
    b = S.measures(S.pack([np.roll(l, 500, axis=0)]))[0][0]
    assert a["area"] == b["area"] and a["length"] == b["length"] and a["bbox"].tolist() == b["bbox"].tolist()


def test_abi_symbols_and_struct_sizes():
    """The library exports the new entry points; the ctypes / numpy mirrors are laid out as the header asserts; the argument checks of
    gsdf_hip_contour_create run on the host, before anything is allocated."""
    from gsdf_amd import hip
    hdr = open(os.path.join(ROOT, "include", "gsdf_hip.h")).read()
    L = hip.lib()
    for name in ("gsdf_hip_contour_create", "gsdf_hip_contour_simplify", "gsdf_hip_contour_measures"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert hasattr(L, name) and name in hip.SYMBOLS, name
    size = lambda t: int(re.search(r"GSDF_ABI_ASSERT\(sizeof\(%s\) == (\d+)," % t, hdr).group(1))
    assert C.sizeof(hip.ContourSimplifyOpts) == size("gsdf_contour_simplify_opts") == 16
    assert C.sizeof(hip.ContourSimplifyStats) == size("gsdf_contour_simplify_stats") == 192
    assert hip.LOOP_MEASURE_DTYPE.itemsize == size("gsdf_loop_measure") == 40 and hip.LOOP_MEASURE_DTYPE == S.LOOP_DTYPE
    assert hip.LAYER_MEASURE_DTYPE.itemsize == size("gsdf_layer_measure") == 40 and hip.LAYER_MEASURE_DTYPE == S.LAYER_DTYPE
    for f, off in (("levels", 4), ("passes", 8), ("dry", 12)):
        assert getattr(hip.ContourSimplifyOpts, f).offset == off and re.search(r"offsetof\(gsdf_contour_simplify_opts, %s\) == %d\b" % (f, off), hdr), f
    for f, off in (("n_loops", 16), ("spans", 32), ("max_level", 168), ("max_dev", 176), ("ms_device", 184)):
        assert getattr(hip.ContourSimplifyStats, f).offset == off and re.search(r"offsetof\(gsdf_contour_simplify_stats, %s\) == %d\b" % (f, off), hdr), f
    assert hip.ContourSimplifyStats.RESULT_BYTES == hip.ContourSimplifyStats.ms_device.offset
    for t, dt, fields in (("gsdf_loop_measure", hip.LOOP_MEASURE_DTYPE, (("length", 8), ("bbox", 16), ("n_verts", 32), ("layer", 36))),
                          ("gsdf_layer_measure", hip.LAYER_MEASURE_DTYPE, (("length", 8), ("bbox", 16), ("n_loops", 32), ("n_verts", 36)))):
        for f, off in fields:
            assert dt.fields[f][1] == off and re.search(r"offsetof\(%s, %s\) == %d\b" % (t, f, off), hdr), (t, f)
    # host-side argument checks need no device
    h = C.c_void_p()
    xy = S.circle(8)
    create = lambda xy, nv, ls, nl, lay, nlay: L.gsdf_hip_contour_create(xy.ctypes.data, nv, np.asarray(ls, np.uint32).ctypes.data, nl,
                                                                         None if lay is None else np.asarray(lay, np.uint32).ctypes.data, nlay, None, C.byref(h))
    err = lambda: L.gsdf_hip_last_error().decode()
    assert create(xy, 0, [0, 8], 1, None, 1) == -1 and create(xy, 8, [0, 8], 0, None, 1) == -1      # GSDF_ERR_EMPTY_BUFFERS
    assert create(xy, 2 ** 32, [0, 8], 1, None, 1) == -10                                            # GSDF_ERR_CAPACITY
    assert create(xy, 8, [1, 8], 1, None, 1) == -3 and "loop 0" in err()
    assert create(xy, 8, [0, 7], 1, None, 1) == -3 and "vertex 7" in err()
    assert create(xy, 8, [0, 3, 5, 8], 3, None, 1) == -3 and "loop 1" in err() and "fewer than 3" in err()
    assert create(xy, 8, [0, 4, 8], 2, [1, 0], 2) == -3 and "loop 1" in err()
    assert create(xy, 8, [0, 4, 8], 2, [0, 2], 2) == -3 and "layer 2" in err()
    assert create(xy, 8, [0, 8], 1, None, 0) == -3
    for bad in (np.nan, np.inf, -np.inf):
        v = xy.copy()
        v[5, 1] = bad
        assert create(v, 8, [0, 8], 1, None, 1) == -3 and "vertex 5" in err()
    assert not h.value
    assert L.gsdf_hip_contour_simplify(None, None, None, None) == -3 and L.gsdf_hip_contour_measures(None, None, None) == -3
