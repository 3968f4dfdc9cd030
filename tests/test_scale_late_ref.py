"""The twins of the later features across float32 magnitudes, CPU only: what holds before the device is asked for it.

tests/test_scale_ref.py did this for the evaluators, the meshers, weld, report and cluster simplification. Here: the contour tracer,
loop simplification and measures, section properties, hatch fill and skin classes (loop stacks), and adaptive simplification, clean,
projection / deviation and rays / thickness (indexed meshes). Each twin is run on scaled input with every length among its parameters
scaled alike, and held to the BASE result times u^p, bit for bit (covariance). Every ladder below is a literal: the rungs over which
the twin is covariant, found here, with the cause of every rung that is not. tests/test_gpu_scale_contours.py and
tests/test_gpu_scale_indexed.py hold the device to the twins on the same rungs, and to its own base rung where a literal here says so.

Loop stacks are placed by the exponent their handle derives, e = max(biased exponent of the largest |coordinate|, 1) - 126: a rung
is the "top" t with the largest |coordinate| in [2^(t-1), 2^t), so e = t for t >= -125.

  STACK_TOPS        128 104 44 12 -4 -36 -96 -120 -125, and SUBNORMAL_TOP = -129 (the largest coordinate itself subnormal: e stays -125)
  STACK_COVARIANT   the first seven, 128 .. -96: 7 of 10 rungs. At these every scaled coordinate and parameter is the exact float32
                    multiple, every float64 term of the twins an exact multiple (products reach 2^(4 * 128) = 2^512 and 2^(-4 * 125)
                    = 2^-500, inside float64), and every float32 result is normal.
  below, -120 -125 -129: NOT covariant, for two causes. (1) The input: a coordinate of 2^-24 of the top (hand loops, mixed loops:
                    circle points near an axis) falls below 2^-126 and loses bits in the subnormal grid -- STACK_INPUT_EXACT says for
                    which fixtures the coordinates survive (the dyadic comb and pyramid do); the lengths 0.0437 u and 0.02 u do not.
                    (2) The output: a float64 crossing converted to float32 lands on the subnormal grid, one rounding of u x where the
                    base has u times one rounding of x; so the hatch of the exact comb is not covariant either. At -129 the
                    exponent is clamped (e = -125 for a top of -129), so the quantisation steps 2^(58-e) .. no longer follow the data.
                    There the twin is the only yardstick: it runs, stays finite, and the device must equal it.

The tracer (contourref over the oracle) is covariant on every rung of RUNGS for every shape of scaled_corpus.shapes2d (each on its
rungs_of), and its slices on every rung of MESH_RUNGS: 10 of 10 and 8 of 8. It has no absolute constant: lattice nodes are
fl(fl(lo - res) + fl(i res)), cut vertices a + t (b - a) with t = da / (da - db), all homogeneous in float32.

projectref and rayref over the oracle are covariant on every rung of MC_RUNGS (6 of 6) and on all of RUNGS; the float32
normalisation s = g . g of a central difference g (|g| about the tap distance step = res / 4 = 2^-5 at u = 1) is the first
thing to leave the normal range: NORMALISATION_END states the rungs found.

adaptiveref and cleanref on arrays at the ends of the exponent range (the mass test's construction): covariant at e = 128 (exact
input); at e = -125 the input is exact only for the box, and what then holds is stated per fixture in ARRAYS_COVARIANT_LOW.
"""
import functools
import math

import numpy as np
import pytest

import adaptiveref as A
import cleanref as K
import contourref
import contoursimpref as S
import hatchref as H
import massref as M
import projectref as P
import rayref as R
import scaled_corpus as SC
import skinref
import toporef as T
from contourref import res_for
from oracle.oracle import OracleSDF
from scaffold.builder import Builder
from test_scale_ref import MC_RUNGS, MESH_RUNGS, RUNGS, rungs_of

F = np.float32

# ---- the literals ----------------------------------------------------------------------------------------------------------------------
STACK_TOPS = (128, 104, 44, 12, -4, -36, -96, -120, -125)
SUBNORMAL_TOP = -129
STACK_COVARIANT = (128, 104, 44, 12, -4, -36, -96)                 # 7 of the 10 rungs; the causes of the other three are above
STACK_INPUT_EXACT = {"hand": False, "mixed": False, "comb": True, "pyramid": True}     # the scaled coordinates below -96
# name -> (maker, spacing, offset, tol of simplify): base values, every one a length
STACKS = {"hand": (H.hand_loops, 0.5, 0.0437, 0.02), "mixed": (lambda: S.mixed_loops(200, 3), 0.5, 0.0437, 0.02),
          "comb": (lambda: H.comb(40), 0.25, 0.125, 0.02), "pyramid": (skinref.pyramid, 0.5, 0.0437, 0.02)}
STACK_ANGLES = (17.0, 73.0, 121.0)                                  # three directions over five layers (l % 3)

TRACER_COVARIANT = RUNGS                                            # 10 of 10 (each shape on its rungs_of)
SLICES_COVARIANT = MESH_RUNGS                                       # 8 of 8
SLICE_SHAPES = ("diff", "circarray0")                               # one loop per layer that changes with z; four loops per layer
# the whole chain runs on these per rung: (a hole -- the only shape of the corpus with one, on its rungs_of --, eight loops, a polygon)
CHAIN_SHAPES = ("lines", "circarray2d1", "poly")
OUTLINE_DIV = 40                                                    # outlines at bounds / 40

INDEXED_SHAPES = ("diff", "extrude_poly")
INDEXED_COVARIANT = MC_RUNGS                                        # projectref, rayref: 6 of 6
# s = g . g in float32: for `diff` the twins are covariant down to u = 2^-54 and no longer at 2^-56, where |g|^2 of about
# (2^-5 2^-56 / ...)^2 drops below 2^-126; upwards nothing ends before 2^64. (`extrude_poly` ends at 2^-50 already: the ORACLE's
# polygon, not the normalisation.) Both ends lie outside RUNGS, so no rung is lost to it.
NORMALISATION_END = {"holds": (-54, 64), "fails": (-56,)}
ARRAY_TOPS = (128, -125)
# at e = -125: (adaptive covariant, clean covariant). The sphere's scaled coordinates are inexact, so its cluster means differ; the
# soup's are inexact too but its faces survive over the same 299 pool vertices; clean compares bits, and equal bits stay equal
ARRAYS_COVARIANT_LOW = {"sphere": (False, True), "box": (True, True), "soup": (None, None)}


# ---- scaling: shared with the GPU files -------------------------------------------------------------------------------------------------
def times(a, k):
    """float32 a times 2^k with ONE rounding (exact unless the product is subnormal or overflows), via float64."""
    return np.ldexp(np.asarray(a, F).astype(np.float64), k).astype(F)


def is_exact(a, k):
    a = np.asarray(a, F).astype(np.float64)
    ok = np.isfinite(a)
    return bool((times(a, k).astype(np.float64)[ok] == np.ldexp(a, k)[ok]).all())


def length(x, k):
    """A parameter that is a length, scaled: float32."""
    return F(times(F(x), k))


def stack_at(c, top):
    """The loops of c with the largest |coordinate| moved into [2^(top-1), 2^top): (Loops, k, whether every coordinate is exact)."""
    k = top - S.exponent(c.xy)
    return S.Loops(times(c.xy, k), c.loop_start, c.loop_layer, c.n_layers, c.keys), k, is_exact(c.xy, k)


def stack_dirs():
    return H.directions(STACK_ANGLES)


# ---- covariance: [] where got is base times 2^(p k) bit for bit, else the names of what differs. Twin and device results alike
def _f64(b, g, p, k):
    return np.ldexp(np.ascontiguousarray(b, np.float64), p * k).tobytes() == np.ascontiguousarray(g, np.float64).tobytes()


def _f32(b, g, k):
    return times(b, k).tobytes() == np.ascontiguousarray(g, F).tobytes()


def _eq(b, g):
    return np.ascontiguousarray(b).tobytes() == np.ascontiguousarray(g).tobytes()


def measures_differ(base, got, k):
    bad = []
    for which, b, g in zip(("loops", "layers"), base, got):
        bad += [(which, f) for f, p in (("area", 2), ("length", 1)) if not _f64(b[f], g[f], p, k)]
        bad += [(which, "bbox")] * (not _f32(b["bbox"], g["bbox"], k))
        bad += [(which, f) for f in b.dtype.names if f not in ("area", "length", "bbox") and not _eq(b[f], g[f])]
    return bad


def sections_differ(base, got, k):
    bad = []
    for which, b, g in zip(("loops", "layers"), base, got):
        bad += [(which, f) for f, p in (("area", 2), ("first", 3), ("second", 4), ("centroid", 1), ("central", 4)) if not _f64(b[f], g[f], p, k)]
        bad += [(which, f) for f in ("n_verts", "layer_or_n_loops") if not _eq(b[f], g[f])]
    return bad


def loops_differ(base, got, k):
    return [f for f in ("keys", "loop_start", "loop_layer") if not _eq(getattr(base, f), getattr(got, f))] + ["xy"] * (not _f32(base.xy, got.xy, k))


def hatch_differ(base, got, k):
    """A hatch or a skin (cls and skin_layers where base has them)."""
    bad = [f for f in ("line", "layer_start") if not _eq(getattr(base, f), getattr(got, f))] + ["seg"] * (not _f32(base.seg, got.seg, k))
    bad += ["layers." + f for f in ("n_segments", "k_min", "k_max") if not _eq(base.layers[f], got.layers[f])]
    bad += ["layers.length"] * (not _f64(base.layers["length"], got.layers["length"], 1, k))
    if getattr(base, "cls", None) is not None:
        bad += ["cls"] * (not _eq(base.cls, got.cls)) + ["skin_layers.n_segments"] * (not _eq(base.skin_layers["n_segments"], got.skin_layers["n_segments"]))
        bad += ["skin_layers.length"] * (not _f64(base.skin_layers["length"], got.skin_layers["length"], 1, k))
    return bad


def simplify_stats_differ(base, got, k):
    """The twin's stats dicts of two simplifications."""
    return [f for f in base if f != "max_dev" and base[f] != got[f]] + ["max_dev"] * (math.ldexp(base["max_dev"], k) != got["max_dev"])


def stack_twins(c, spacing, offset, tol):
    """Every twin of a loop stack: what tests/test_gpu_scale_contours.py asks of the device for the same arguments."""
    d = stack_dirs()
    return {"measures": S.measures(c), "sections": M.sections(c.xy, c.loop_start, c.loop_layer, c.n_layers)[:2], "simplify": S.simplify(c, tol, 8, 2),
            "hatch": H.hatch(c, spacing, d, offset), "reversed": H.hatch(c, spacing, -d, -offset), "skin": skinref.skin(c, spacing, d, 1, 1, offset)}


def stack_differ(base, got, k):
    bad = [("measures", x) for x in measures_differ(base["measures"], got["measures"], k)] + [("sections", x) for x in sections_differ(base["sections"], got["sections"], k)]
    bad += [("simplify", x) for x in loops_differ(base["simplify"][0], got["simplify"][0], k) + simplify_stats_differ(base["simplify"][1], got["simplify"][1], k)]
    bad += [("simplified measures", x) for x in measures_differ(S.measures(base["simplify"][0]), S.measures(got["simplify"][0]), k)]
    for w in ("hatch", "reversed", "skin"):
        bad += [(w, x) for x in hatch_differ(base[w], got[w], k)]
        bad += [(w, "stats", f) for f in base[w].stats if f != "length" and base[w].stats[f] != got[w].stats[f]]
        bl, gl = np.atleast_1d(base[w].stats["length"]), np.atleast_1d(got[w].stats["length"])
        bad += [(w, "stats", "length")] * (not _f64(bl, gl, 1, k))
    return bad


def stack_finite(r):
    ok = all(np.isfinite(a[f]).all() for a in r["measures"] for f in ("area", "length"))
    ok &= all(np.isfinite(a[f]).all() for a in r["sections"] for f in ("area", "first", "second"))
    ok &= bool(np.isfinite(r["simplify"][0].xy).all()) and math.isfinite(r["simplify"][1]["max_dev"])
    for w in ("hatch", "reversed", "skin"):
        ok &= bool(np.isfinite(r[w].seg).all() and np.isfinite(r[w].layers["length"]).all() and np.isfinite(np.atleast_1d(r[w].stats["length"])).all())
    return bool(ok)


# ---- loop stacks ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(STACKS))
def test_loop_stacks_on_the_exponent_ladder(name):
    make, sp, off, tol = STACKS[name]
    c = make()
    base = stack_twins(c, F(sp), F(off), F(tol))
    assert base["hatch"].stats["n_segments"] > 20 and base["skin"].stats["n_segments"] > 20 and len(c.xy) == {"hand": 361, "mixed": 8810, "comb": 160, "pyramid": 8}[name]
    held = 0
    for top in STACK_TOPS + (SUBNORMAL_TOP,):
        cs, k, exact = stack_at(c, top)
        args = (length(sp, k), length(off, k), length(tol, k))
        assert S.exponent(cs.xy) == M.loop_exponent(cs.xy) == max(top, -125), (name, top)
        got = stack_twins(cs, *args)
        assert stack_finite(got), (name, top)
        if top in STACK_COVARIANT:
            assert exact and all(is_exact(F(x), k) for x in (sp, off, tol)), (name, top)
            assert stack_differ(base, got, k) == [], (name, top)
            held += 1
        else:
            assert exact == STACK_INPUT_EXACT[name], (name, top)
            assert not is_exact(F(tol), k)                                      # (the lengths that are no powers of two lose bits)
            assert hatch_differ(base["hatch"], got["hatch"], k), (name, top)    # the ladder is not shorter than it has to be
    assert held == len(STACK_COVARIANT) == 7


def mixed_magnitudes():
    """64 four-vertex loops in layer 0 whose magnitudes alternate between 2^100 (even) and 2^-100 (odd), and eight loops of 2^-100 in
    layer 1: one wave of edges holds loops 2^200 apart, and e = 100 belongs to the handle. Squares on a grid of pitch 0.2 about the
    origin (half sides 0.07 .. 0.133: the largest |coordinate| is 0.833, so e = 100 exactly), in units of 2^100 or 2^-100."""
    loops, layers = [], []
    for i in range(64):
        cx, cy, a = ((i % 8) - 3.5) * 0.2, ((i // 8) - 3.5) * 0.2, 0.07 + 0.001 * i
        loops.append(times(skinref.square(a, cx, cy), 100 if i % 2 == 0 else -100))
        layers.append(0)
    for i in range(8):
        loops.append(loops[2 * i + 1 + 24].copy())              # the small loops of rows 3 and 4: they straddle the lines through 0
        layers.append(1)
    return S.pack(loops, layers, 2)


def small_layer_alone(c):
    """Layer 1 of mixed_magnitudes() as a stack of its own: e = -100."""
    mine = np.flatnonzero(c.loop_layer == 1)
    return S.pack([c.loops()[q] for q in mine], [0] * len(mine), 1)


MIXED_SPACING, MIXED_ANGLES = 0.05, (17.0, 73.0)                     # in units of the handle's 2^e; offset 0: a line through the origin


def test_mixed_magnitudes_in_one_stack():
    c = mixed_magnitudes()
    assert S.exponent(c.xy) == 100 and len(c.xy) == 72 * 4
    loops, layers = S.measures(c)
    small = np.arange(64) % 2 == 1
    assert (loops["area"][:64][small] == 0).all() and (loops["area"][:64][~small] > 0).all()       # 2^-200 2^(61-200) quantises to 0
    assert (loops["area"][64:] == 0).all() and layers[1]["area"] == 0 and layers[1]["length"] == 0 and layers[1]["n_loops"] == 8
    sl, sy, _ = M.sections(c.xy, c.loop_start, c.loop_layer, c.n_layers)
    assert (sl["area"][:64][small] == 0).all() and sy[1]["area"] == 0 and np.isnan(sy[1]["centroid"]).all()
    d = H.directions(MIXED_ANGLES)
    h = H.hatch(c, length(MIXED_SPACING, 100), d, 0.0)
    assert h.layers[1]["n_segments"] > 0 and h.layers[1]["length"] == 0 and h.layers[0]["length"] > 0 and h.stats["zero_length"] == 0
    alone = small_layer_alone(c)
    assert S.exponent(alone.xy) == -100
    al, ay = S.measures(alone)
    want = np.array([(2 * (0.07 + 0.001 * (2 * i + 25))) ** 2 for i in range(8)]) * 2.0 ** -200
    assert np.allclose(al["area"], want, rtol=1e-5, atol=0) and ay[0]["area"] > 0      # its true area: e is the handle's, not the loop's
    ha = H.hatch(alone, length(MIXED_SPACING, -100), d[1:], 0.0)             # at its own scale: lines 0.05 apart across every small loop
    assert ha.stats["n_segments"] > 8 * 4 and ha.stats["length"] > 0


def refusal_cases(e):
    """The circle of tests/test_gpu_hatch.py::test_argument_errors (e = 4) at exponent e: [(spacing, offset, refused)] at the boundary
    (2^(e+1) + |offset|) / spacing = 2^29. With offset 0 the boundary is spacing = 2^(e-28): refused, and the smallest spacing that is
    admitted (the next float32) would make 0.6 x 2^29 lines of the circle -- gigabytes; so acceptance is asked where the offset makes
    the numerator 2^(e+20) exactly (offset = 2^(e+20) - 2^(e+1)): admitted one float32 above 2^(e-9), where the circle has 640
    lines, and refused at 2^(e-9), the next smaller power of two."""
    off = F(math.ldexp(1.0, e + 20) - math.ldexp(1.0, e + 1))
    assert float(off) + math.ldexp(1.0, e + 1) == math.ldexp(1.0, e + 20)
    edge = F(math.ldexp(1.0, e - 9))
    return [(F(math.ldexp(1.0, e - 28)), F(0), True), (np.nextafter(edge, F(np.inf)), off, False), (edge, off, True),
            (np.nextafter(edge, F(np.inf)), F(-off), False), (edge, F(-off), True)]


def refusal_circle(e):
    c = S.pack([S.circle(40)])
    return stack_at(c, e)[0]


@pytest.mark.parametrize("e", [100, -100])
def test_the_refusal_boundary_is_scale_free(e):
    c = refusal_circle(e)
    assert S.exponent(c.xy) == e
    for sp, off, refused in refusal_cases(e):
        if refused:
            with pytest.raises(ValueError, match="spacing is too small for these coordinates"):
                H.check_arguments(c, sp, [(1.0, 0.0)], off)
        else:
            h = H.hatch(c, sp, [(1.0, 0.0)], off)
            assert 600 < h.stats["n_lines"] < 680 and abs(int(h.line[0])) > 2 ** 28
    # the smallest spacing admitted at offset 0 is the next float32 above the refused power of two
    assert H.check_arguments(c, np.nextafter(F(math.ldexp(1.0, e - 28)), F(np.inf)), [(1.0, 0.0)], 0.0)[3] == e


# ---- the tracer -------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def outline_base():
    """name -> (res, contour of the oracle) at u = 1, for scaled_corpus.shapes2d."""
    out = {}
    for name, sh in SC.shapes2d(Builder(), 1.0)[1]:
        res = res_for(sh.Bounds(), OUTLINE_DIV)
        out[name] = (res, contourref.of_oracle(sh.tree(), res))
    return out


def slice_setup(sh, res0, u):
    """(res, the four heights) of a mesh shape built at unit u; res0: the base rung's diagonal / 32."""
    bb = sh.Bounds()
    return F(res0 * F(u)), contourref.layer_heights(bb, F(F(bb[5] - bb[2]) / F(4)))


@functools.lru_cache(maxsize=None)
def slices_base():
    out = {}
    shapes = dict(SC.mesh_shapes(Builder(), 1.0)[1])
    for name in SLICE_SHAPES:
        res0 = F(float(shapes[name].Diagonal()) / 32)
        res, z = slice_setup(shapes[name], res0, 1.0)
        assert len(z) == 4
        out[name] = (res0, z, contourref.of_oracle(shapes[name].tree(), res, z))
    return out


def contour_differ(base, got, k):
    """Two traced contours (twin or device handle): the integer statistics where both are twins, the arrays."""
    bad = loops_differ(base, got, k)
    if isinstance(getattr(base, "stats", None), dict) and isinstance(getattr(got, "stats", None), dict):
        bad += [f for f in base.stats if base.stats[f] != got.stats[f]]
    return bad


@pytest.mark.parametrize("k", RUNGS)
def test_outlines_are_covariant(k):
    u = SC.unit(k)
    base = outline_base()
    n = 0
    for name, sh in SC.shapes2d(Builder(), u)[1]:
        if k not in rungs_of(name):
            continue
        res0, c0 = base[name]
        c = contourref.of_oracle(sh.tree(), F(res0 * F(u)))
        assert contour_differ(c0, c, k) == [], (name, k)
        n += 1
    assert k in TRACER_COVARIANT and n >= 37


@pytest.mark.parametrize("k", MESH_RUNGS)
def test_slices_are_covariant(k):
    u = SC.unit(k)
    shapes = dict(SC.mesh_shapes(Builder(), u)[1])
    for name in SLICE_SHAPES:
        res0, z0, c0 = slices_base()[name]
        res, z = slice_setup(shapes[name], res0, u)
        assert z.tobytes() == times(z0, k).tobytes(), (name, k)
        assert contour_differ(c0, contourref.of_oracle(shapes[name].tree(), res, z), k) == [], (name, k)
    assert k in SLICES_COVARIANT


def test_the_chain_shapes_are_what_they_are_named_for():
    base = outline_base()
    holes, several, poly = (base[n][1] for n in CHAIN_SHAPES)
    assert (holes.areas() < 0).any() and (holes.areas() > 0).any()
    assert len(several.loop_layer) == 8 and (several.areas() > 0).all()
    assert len(poly.loop_layer) == 1
    per_layer = [int((slices_base()[n][2].loop_layer == l).sum()) for n in SLICE_SHAPES for l in range(4)]
    assert per_layer == [1, 1, 1, 1, 4, 4, 4, 4]


def chain_args(res):
    """What the chain on a traced handle is run with: simplify's tol, the hatch's spacing and directions. All from res, so scaled."""
    return F(res / F(8)), F(F(4) * res), H.directions((45.0, 135.0))


@pytest.mark.parametrize("k", RUNGS)
def test_the_chain_on_traced_loops_is_covariant(k):
    """simplify -> measures -> sections -> hatch (-> skin for slices) on the twin's traced loops: the coordinates are of order u, far
    inside STACK_COVARIANT's range, so the chain inherits the tracer's covariance."""
    u = SC.unit(k)
    d2 = dict(SC.shapes2d(Builder(), u)[1])
    d3 = dict(SC.mesh_shapes(Builder(), u)[1])
    cases = [(outline_base()[n][1], contourref.of_oracle(d2[n].tree(), F(outline_base()[n][0] * F(u))), outline_base()[n][0]) for n in CHAIN_SHAPES if k in rungs_of(n)]
    for n in SLICE_SHAPES if k in MESH_RUNGS else ():
        res0, _, c0 = slices_base()[n]
        cases.append((c0, contourref.of_oracle(d3[n].tree(), *slice_setup(d3[n], res0, u)), res0))
    for c0, c, res0 in cases:
        out = []
        for cc, res in ((S.Loops.of(c0), res0), (S.Loops.of(c), F(res0 * F(u)))):
            tol, sp, d = chain_args(res)
            simple, st = S.simplify(cc, tol, 8, 2)
            out.append((simple, st, S.measures(simple), M.sections(simple.xy, simple.loop_start, simple.loop_layer, simple.n_layers)[:2], H.hatch(simple, sp, d),
                        skinref.skin(simple, sp, d, 1, 1)))
        (s0, st0, m0, q0, h0, k0), (s1, st1, m1, q1, h1, k1) = out
        assert loops_differ(s0, s1, k) + simplify_stats_differ(st0, st1, k) + measures_differ(m0, m1, k) + sections_differ(q0, q1, k) + hatch_differ(h0, h1, k) + hatch_differ(k0, k1, k) == []


# ---- indexed meshes ---------------------------------------------------------------------------------------------------------------------
def mesh_at(v, top):
    """Vertices with the largest finite |coordinate| moved into [2^(top-1), 2^top): (verts, k, exact)."""
    k = top - T.exponent_of(v)
    return times(v, k), k, is_exact(v, k)


def array_meshes():
    """name -> (verts, idx, cell, tol of simplify_adaptive): base values."""
    from test_gpu_clean import contended_soup
    sv, si = M.sphere(12, 16)
    bv, bi = M.box((1, 2, 3), (5, 6, 7))
    cv, ci = contended_soup()
    return {"sphere": (sv, si, 0.3, 0.1), "box": (bv, bi, 3.0, 0.5), "soup": (cv, ci, 0.5, 0.05)}


ADAPTIVE_LEVELS = 4
CLEAN_FLAGS = K.MERGE_POSITIONS | K.FACES


def mesh_differ(base, got, k):
    """(verts, idx, keys, ...) of two results: faces and keys equal, vertices times 2^k."""
    return ["idx"] * (not _eq(base[1], got[1])) + ["keys"] * (not _eq(base[2], got[2])) + ["verts"] * (not _f32(base[0], got[0], k))


@pytest.mark.parametrize("name", ["sphere", "box", "soup"])
def test_adaptive_and_clean_on_arrays_at_the_ends_of_the_exponent_range(name):
    v, i, cell, tol = array_meshes()[name]
    a0 = A.simplify(v, i, F(cell), F(tol), ADAPTIVE_LEVELS)
    c0 = K.clean(v, i, None, None, CLEAN_FLAGS)
    assert a0[3]["n_tris"] > 0 and c0[4]["n_tris"] > 0
    for top in ARRAY_TOPS:
        s, k, exact = mesh_at(v, top)
        assert T.exponent_of(s) == top and exact == (top == 128 or name == "box"), (name, top)
        a = A.simplify(s, i, length(cell, k), length(tol, k), ADAPTIVE_LEVELS)
        c = K.clean(s, i, None, None, CLEAN_FLAGS)
        assert a[3]["exponent"] == top and np.isfinite(a[0]).all() and math.isfinite(a[3]["max_err"]), (name, top)
        assert np.isfinite(c[0][np.isfinite(c[0])]).all() and c[4]["n_tris"] == c0[4]["n_tris"], (name, top)
        if top == 128:
            assert mesh_differ(a0, a, k) == [] and a[3]["max_err"] == math.ldexp(a0[3]["max_err"], k) and mesh_differ(c0, c, k) == [], (name, top)
        else:
            want_a, want_c = ARRAYS_COVARIANT_LOW[name]
            if want_a is not None:
                assert (mesh_differ(a0, a, k) == [], mesh_differ(c0, c, k) == []) == (want_a, want_c), (name, top)


def indexed_opts(res):
    """The options the indexed chain is run with at a resolution: every length derives from res, so it scales with it."""
    return {"adaptive": dict(cell=res, tol=F(res / F(4)), levels=4),
            "project": dict(step=F(res / F(4)), tol=F(res / F(1024)), max_move=F(F(4) * res), max_iters=8),
            "rays": dict(tmax=F(F(64) * res), tol=F(res / F(1024)), max_steps=96, refine=8, thin=F(F(16) * res)),
            "thickness": dict(step=F(res / F(4)), t0=F(res / F(4)), tmax=F(F(64) * res), tol=F(res / F(1024)), max_steps=128, refine=8, thin=F(F(2) * res))}


def corner_rays(bb, n=300, seed=61):
    """tests/test_gpu_ray.py's corner rays of the BASE bounds: origins (lengths: scaled by the caller) and directions (ratios of
    lengths: the same on every rung, so that t is a length)."""
    from test_gpu_ray import corner_rays as make
    o, r = make(bb, n, seed)
    return o, (r / np.linalg.norm(r.astype(np.float64), axis=1)[:, None]).astype(F)


@functools.lru_cache(maxsize=None)
def indexed_base():
    """name -> (res, verts of the oracle's octree mesh, project / raycast / thickness of the twins over the oracle) at u = 1."""
    out = {}
    shapes = dict(SC.mesh_shapes(Builder(), 1.0)[1])
    for name in INDEXED_SHAPES:
        sh = shapes[name]
        cpu = OracleSDF(sh.tree())
        res = F(float(sh.Diagonal()) / 32)
        v = np.unique(cpu.render_octree(res, 4096, True).tris.reshape(-1, 3), axis=0)
        o = indexed_opts(res)
        rays = corner_rays(sh.Bounds())
        out[name] = (res, v, rays, P.project(cpu.Evaluate, v, **o["project"]), R.raycast(cpu.Evaluate, *rays, **o["rays"]), R.thickness(cpu.Evaluate, v, **o["thickness"]))
    return out


def project_differ(base, got, k):
    """(positions, d_before, d_after, status, ...) of two projections."""
    return [n for j, n in enumerate(("positions", "d_before", "d_after")) if not _f32(base[j], got[j], k)] + ["status"] * (not _eq(base[3], got[3]))


def rays_differ(base, got, k):
    """(t, d, status, steps, ...) of two raycasts."""
    return [n for j, n in enumerate(("t", "d")) if not _f32(base[j], got[j], k)] + [n for j, n in ((2, "status"), (3, "steps")) if not _eq(base[j], got[j])]


def thickness_differ(base, got, k):
    return ["thickness"] * (not _f32(base[0], got[0], k)) + ["status"] * (not _eq(base[1], got[1]))


def indexed_twins_at(name, k):
    res0, v0, (o0, r0), _, _, _ = indexed_base()[name]
    u = SC.unit(k)
    cpu = OracleSDF(dict(SC.mesh_shapes(Builder(), u)[1])[name].tree())
    o = indexed_opts(F(res0 * F(u)))
    v = times(v0, k)
    return P.project(cpu.Evaluate, v, **o["project"]), R.raycast(cpu.Evaluate, times(o0, k), r0, **o["rays"]), R.thickness(cpu.Evaluate, v, **o["thickness"])


def indexed_differ(name, k):
    _, _, _, p0, r0, t0 = indexed_base()[name]
    p, r, t = indexed_twins_at(name, k)
    bad = project_differ(p0, p, k) + rays_differ(r0, r, k) + thickness_differ(t0, t, k)
    return bad + ["evals"] * ((p[4]["evals"], r[4]["evals"], t[2]["evals"]) != (p0[4]["evals"], r0[4]["evals"], t0[2]["evals"]))


@pytest.mark.parametrize("k", RUNGS)
def test_projection_and_rays_are_covariant(k):
    for name in INDEXED_SHAPES:
        _, v0, _, p0, r0, t0 = indexed_base()[name]
        assert len(v0) > 3000 and p0[4]["count"][P.CONVERGED] > 300 and r0[4]["count"][R.HIT] + r0[4]["count"][R.CROSSED] > 100 and t0[2]["count"][R.HIT] > 3000
        assert indexed_differ(name, k) == [], (name, k)
    assert set(INDEXED_COVARIANT) <= set(RUNGS)


def mass_differ(base, got, k):
    """Two gsdf_mass records (massref.MASS_DTYPE) of one shell or of the whole mesh."""
    bad = [f for f, p in (("volume", 3), ("first", 4), ("second", 5), ("centroid", 1), ("inertia", 5)) if not _f64(base[f], got[f], p, k)]
    return bad + ["exponent"] * (int(got["exponent"]) != int(base["exponent"]) + k) + ["label"] * (int(got["label"]) != int(base["label"]))


def mesh_twins(v, i, keys, res, origin):
    """adaptiveref, cleanref and massref on one indexed mesh, with indexed_opts(res): what the device is asked for on the same arrays."""
    o = indexed_opts(res)["adaptive"]
    return A.simplify(v, i, o["cell"], o["tol"], o["levels"], origin, keys), K.clean(v, i, keys, None, CLEAN_FLAGS), M.mesh_mass(v, i)


def mesh_twins_differ(base, got, k):
    (a0, c0, m0), (a, c, m) = base, got
    bad = [("adaptive", x) for x in mesh_differ(a0, a, k)] + [("adaptive", "max_err")] * (math.ldexp(a0[3]["max_err"], k) != a[3]["max_err"])
    bad += [("adaptive", f) for f in a0[3] if f not in ("max_err", "exponent") and a0[3][f] != a[3][f]] + [("adaptive", "exponent")] * (a[3]["exponent"] != a0[3]["exponent"] + k)
    bad += [("clean", x) for x in mesh_differ(c0, c, k)] + [("clean", f) for f in c0[4] if c0[4][f] != c[4][f]]
    bad += [("mass", x) for x in mass_differ(m0[0], m[0], k)] + [("mass", "shells")] * (len(m0[1]) != len(m[1]))
    return bad + [("mass", "shell", x) for b, g in zip(m0[1], m[1]) for x in mass_differ(b, g, k)]


@functools.lru_cache(maxsize=None)
def oracle_meshes():
    """name -> (res, origin, verts, idx) at u = 1: the oracle's octree mesh as an indexed mesh (np.unique over its corners, so with
    exact duplicates joined and nothing else), the lattice origin half a cell off the bounds' corner."""
    out = {}
    for name in INDEXED_SHAPES:
        sh = dict(SC.mesh_shapes(Builder(), 1.0)[1])[name]
        res = F(float(sh.Diagonal()) / 32)
        v, inv = np.unique(OracleSDF(sh.tree()).render_octree(res, 4096, True).tris.reshape(-1, 3), axis=0, return_inverse=True)
        out[name] = (res, tuple(F(x) - F(0.5) * res for x in sh.Bounds()[:3]), np.ascontiguousarray(v, F), np.ascontiguousarray(inv.reshape(-1, 3), np.uint32))
    return out


@pytest.mark.parametrize("k", MC_RUNGS)
def test_adaptive_clean_and_mass_are_covariant_on_exactly_scaled_arrays(k):
    """A mesh whose vertices are the base rung's times u: the form in which the GPU file compares rungs (two welds of one tree differ
    in their last bits, so two RUNS are not comparable byte for byte; the arrays of one run, scaled, are)."""
    for name in INDEXED_SHAPES:
        res, origin, v, i = oracle_meshes()[name]
        base = mesh_twins(v, i, None, res, origin)
        assert base[0][3]["n_tris"] < len(i) and sum(base[0][3]["chosen"][1:]) > 0 and base[1][4]["n_tris"] > 1000, (name, base[0][3])
        got = mesh_twins(times(v, k), i, None, F(res * F(SC.unit(k))), tuple(length(x, k) for x in origin))
        assert mesh_twins_differ(base, got, k) == [], (name, k)


def test_the_central_difference_normalisation_ends_where_it_is_said_to():
    lo, hi = NORMALISATION_END["holds"]
    assert indexed_differ("diff", lo) == [] and indexed_differ("diff", hi) == []
    bad = indexed_differ("diff", NORMALISATION_END["fails"][0])
    assert "positions" in bad and "thickness" in bad and "t" not in bad          # the gradient's square, not the march
