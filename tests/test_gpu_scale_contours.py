"""Contours, fills and loop measures on the device across float32 magnitudes: every entry point that derives an exponent
e = max(biased exponent, 1) - 126 from its handle and scales by 2^(61-2e), 2^(60-e), 2^(62-3e), 2^(62-4e), 2^(58-e) -- measures,
sections, simplify, hatch, skin -- and the tracer that feeds them, away from the e = 3 .. 10 where the rest of the suite lives.

Everything is held as bytes to the twin of its contract through the neighbouring files' own helpers (test_gpu_contour.same,
test_gpu_contour_simplify.check / check_measures, test_gpu_mass.check_sections, test_gpu_hatch.check, test_gpu_skin.check: dry runs
included); no tolerance anywhere. Where tests/test_scale_late_ref.py's literals say the TWIN is covariant, the device's result is also
held to this module's own base rung times 2^(p k), bit for bit -- a yardstick that does not pass through the twin.

  (a) array stacks (hand loops, 8 810 mixed vertices, the 40-tooth comb, the pyramid) with their exponent at 128, 104, 44, 12, -4, -36,
      -96, -120, -125 and with a subnormal largest coordinate: measures, sections, simplify (two passes) and its measures, hatch over
      three directions, the reversed directions, skin with one layer below and above; covariance on STACK_COVARIANT;
  (b) the hatch's refusal (2^(e+1) + |offset|) / spacing >= 2^29 at e = 100 and e = -100, at the float32 either side of the boundary;
  (c) one stack whose loops alternate between 2^100 and 2^-100 inside every wave, and its small layer alone;
  (d) outlines of every scaled_corpus.shapes2d shape on RUNGS and four slices of two mesh shapes on MESH_RUNGS against the tracer's
      twin over the oracle, with the whole chain simplify -> measures -> sections -> hatch (-> skin) on three outlines and both stacks
      of slices per rung; through the interpreter, and on the two extreme rungs through specialize() too (builds side by side).

Time, one run on one MI355X machine: this file 7 s (33 cases) beside tests/test_gpu_scale_indexed.py's 1.5 s (18 cases). Per case: a
rung of (a) 0.07 s (four stacks, seven entry points each with its twin and dry run; the first also loads the libraries and makes the
base rung, 1.9 s); (b) and (c) 0.01 s; a rung of outlines 0.07 s (42 shapes traced, three chains), of slices 0.02 s; five per-tree
builds side by side 1.2 s, the slowest.

Sensitivity, tried once on scratch copies of the kernels (none committed); the neighbouring files (test_gpu_contour,
_contour_simplify, _hatch, _skin, _mass) passed with every one of them:
  cmeas_pow2 built in the float32 exponent field (right for |x| <= 126 only)    (a) at 128, 104, -36 .. -129, (b) at -100, (c), (d) from 2^-20 down
  hatch_length_kernel without the `biased > 1u` clamp                           (a) at -129 alone (layers' lengths twice the twin's)
  HATCH_K_LIMIT at 2^28 + 64                                                    (b), both exponents
  hatch_emit_kernel flushing a subnormal (float) crossing to 0                  (a) at -120, -125, -129
  an absolute `|d_lo - d_hi| < 1e-12 -> t = 0.5` in the tracer's vertex         (d) outlines from 2^-10 down, slices at 2^-40, the per-tree builds
"""
import numpy as np
import pytest

import contourref
import contoursimpref as S
import hatchref as H
import par
import scaled_corpus as SC
import test_scale_late_ref as L
from scaffold.builder import Builder
from test_gpu_contour import same as same_trace
from test_gpu_contour_simplify import check as simplify_check
from test_gpu_contour_simplify import check_measures
from test_gpu_hatch import check as hatch_check
from test_gpu_hatch import code, upload
from test_gpu_mass import check_sections
from test_gpu_skin import check as skin_check
from test_scale_ref import MESH_RUNGS, RUNGS, rungs_of

pytestmark = pytest.mark.gpu
F = np.float32
BAD_ARGUMENT = -3


def hatch_stats_differ(base, got, k):
    """HatchStats / SkinStats of two device runs: the counts equal, the lengths times 2^k."""
    bad = [f for f in ("n_segments", "n_crossings", "n_lines", "max_line_crossings", "zero_length", "n_layers") if getattr(base, f) != getattr(got, f)]
    bl, gl = (np.array(x.length, np.float64).reshape(-1) for x in (base, got))
    return bad + ["length"] * (np.ldexp(bl, k).tobytes() != gl.tobytes())


def device_stack(gpu, c, spacing, offset, tol, what):
    """Every entry point on one handle of the loops c, each against its twin; what the covariance is read off."""
    dev = upload(gpu, c)
    assert dev.xy.tobytes() == c.xy.tobytes() and S.exponent(dev.xy) == S.exponent(c.xy)
    check_measures(dev, c, what)
    sections = check_sections(gpu, c.xy, c.loop_start, c.loop_layer, c.n_layers, what, dev)
    simple, want, _ = simplify_check(gpu, dev, c, tol, 8, 2, what)
    check_measures(simple, want, (what, "simplified"))
    d = L.stack_dirs()
    out = {"measures": dev.measures(), "sections": sections, "simplify": simple, "simplified measures": simple.measures()}
    for name, dirs, off in (("hatch", d, offset), ("reversed", -d, -offset)):
        out[name], tw = hatch_check(gpu, dev, c, spacing, dirs, off, (what, name))
        assert out[name].stats.zero_length == tw.stats["zero_length"]
    out["skin"], tw = skin_check(gpu, dev, c, spacing, d, 1, 1, offset, (what, "skin"))
    assert out["skin"].stats.zero_length == tw.stats["zero_length"] and list(out["skin"].stats.n_class) == tw.stats["n_class"]
    return out


def device_stack_differ(base, got, k):
    bad = [("measures", x) for x in L.measures_differ(base["measures"], got["measures"], k)] + [("sections", x) for x in L.sections_differ(base["sections"], got["sections"], k)]
    bad += [("simplify", x) for x in L.loops_differ(base["simplify"], got["simplify"], k)]
    bad += [("simplified measures", x) for x in L.measures_differ(base["simplified measures"], got["simplified measures"], k)]
    for w in ("hatch", "reversed", "skin"):
        bad += [(w, x) for x in L.hatch_differ(base[w], got[w], k) + hatch_stats_differ(base[w].stats, got[w].stats, k)]
    return bad


# ---- (a) array stacks on the exponent ladder
@pytest.fixture(scope="module")
def stack_base(gpu):
    out = {}
    for name, (make, sp, off, tol) in L.STACKS.items():
        c = make()
        out[name] = (c, device_stack(gpu, c, F(sp), F(off), F(tol), (name, "base")))
    return out


@pytest.mark.parametrize("top", L.STACK_TOPS + (L.SUBNORMAL_TOP,))
def test_array_stacks_on_the_exponent_ladder(gpu, stack_base, top):
    for name, (_, sp, off, tol) in L.STACKS.items():
        c, base = stack_base[name]
        cs, k, exact = L.stack_at(c, top)
        got = device_stack(gpu, cs, L.length(sp, k), L.length(off, k), L.length(tol, k), (name, top))
        assert S.exponent(cs.xy) == max(top, -125), (name, top)
        if top in L.STACK_COVARIANT:
            assert exact and S.exponent(cs.xy) == S.exponent(c.xy) + k, (name, top)
            assert device_stack_differ(base, got, k) == [], (name, top)
        else:
            assert exact == L.STACK_INPUT_EXACT[name], (name, top)


# ---- (b) the refusal boundary
@pytest.mark.parametrize("e", [100, -100])
def test_the_refusal_boundary_is_scale_free(gpu, e):
    c = L.refusal_circle(e)
    dev = upload(gpu, c)
    d = [(1.0, 0.0)]
    for sp, off, refused in L.refusal_cases(e):
        if refused:
            with pytest.raises(ValueError) as twin:
                H.check_arguments(c, sp, d, off)
            for fn in (lambda: dev.hatch_dirs(sp, d, off), lambda: dev.hatch_dirs(sp, d, off, dry=True), lambda: dev.skin_dirs(sp, d, 1, 1, off)):
                rc, msg = code(gpu, fn)
                assert rc == BAD_ARGUMENT and str(twin.value) in msg, (e, float(sp), float(off), msg)
        else:
            got, _ = hatch_check(gpu, dev, c, sp, d, off, (e, float(sp), float(off)))
            assert 600 < got.stats.n_lines < 680
            skin_check(gpu, dev, c, sp, d, 1, 1, off, (e, "skin"))


# ---- (c) mixed magnitudes inside one wave
def test_mixed_magnitudes_inside_one_wave(gpu):
    c = L.mixed_magnitudes()
    dev = upload(gpu, c)
    check_measures(dev, c, "mixed magnitudes")
    loops, layers = check_sections(gpu, c.xy, c.loop_start, c.loop_layer, c.n_layers, "mixed magnitudes", dev)
    d = H.directions(L.MIXED_ANGLES)
    got, _ = hatch_check(gpu, dev, c, L.length(L.MIXED_SPACING, 100), d, 0.0, "mixed magnitudes")
    small = np.arange(64) % 2 == 1
    m, my = dev.measures()
    assert (m["area"][:64][small] == 0).all() and (m["area"][:64][~small] > 0).all() and (m["area"][64:] == 0).all() and my[1]["area"] == 0
    assert (loops["area"][:64][small] == 0).all() and layers[1]["area"] == 0
    assert got.layers[1]["n_segments"] > 0 and got.layers[1]["length"] == 0 and got.layers[0]["length"] > 0
    # the small layer in a handle of its own: e = -100, and its true areas
    alone = L.small_layer_alone(c)
    da = upload(gpu, alone)
    check_measures(da, alone, "small layer alone")
    al, ay = check_sections(gpu, alone.xy, alone.loop_start, alone.loop_layer, alone.n_layers, "small layer alone", da)
    ha, _ = hatch_check(gpu, da, alone, L.length(L.MIXED_SPACING, -100), d[1:], 0.0, "small layer alone")
    want = np.array([(2 * (0.07 + 0.001 * (2 * i + 25))) ** 2 for i in range(8)]) * 2.0 ** -200
    assert np.allclose(da.measures()[0]["area"], want, rtol=1e-5, atol=0) and np.allclose(al["area"], want, rtol=1e-5, atol=0) and ay[0]["area"] > 0
    assert ha.n_segments > 8 * 4 and ha.stats.length > 0


# ---- (d) traced handles
def chain(gpu, dev, res, what, skin):
    """simplify -> measures -> sections -> hatch (two directions) (-> skin) on a traced handle, each step against its twin."""
    tol, sp, d = L.chain_args(res)
    simple, want, _ = simplify_check(gpu, dev, S.Loops.of(dev), tol, 8, 2, what)
    check_measures(simple, want, what)
    sections = check_sections(gpu, want.xy, want.loop_start, want.loop_layer, want.n_layers, what, simple)
    hatch, tw = hatch_check(gpu, simple, want, sp, d, 0.0, what)
    assert tw.stats["n_segments"] > 0, what
    return simple, simple.measures(), sections, hatch, (skin_check(gpu, simple, want, sp, d, 1, 1, 0.0, what)[0] if skin else None)


def chain_differ(base, got, k):
    bad = L.loops_differ(base[0], got[0], k) + L.measures_differ(base[1], got[1], k) + L.sections_differ(base[2], got[2], k)
    for b, g in zip(base[3:], got[3:]):
        if b is not None:
            bad += L.hatch_differ(b, g, k) + hatch_stats_differ(b.stats, g.stats, k)
    return bad


def outlines(gpu, k, names=None, specialise=False):
    """name -> (handle, chain or None) of scaled_corpus.shapes2d at u = 2^k, each outline against the tracer's twin over the oracle."""
    u = SC.unit(k)
    out = {}
    for name, sh in SC.shapes2d(Builder(), u)[1]:
        if (k != 0 and k not in rungs_of(name)) or (names is not None and name not in names):
            continue
        res = F(L.outline_base()[name][0] * F(u))
        sdf = gpu.SDF2HIP(sh)
        if specialise:
            sdf.specialize()
            assert sdf.info()["specialized"]
        dev = gpu.ContourHIP.outline(sdf, res)
        same_trace(dev, contourref.of_oracle(sh.tree(), res), (name, k))
        out[name] = (dev, chain(gpu, dev, res, (name, k, "chain"), False) if name in L.CHAIN_SHAPES else None)
    return out


def slices(gpu, k, names=L.SLICE_SHAPES, specialise=False):
    u = SC.unit(k)
    shapes = dict(SC.mesh_shapes(Builder(), u)[1])
    out = {}
    for name in names:
        res, z = L.slice_setup(shapes[name], L.slices_base()[name][0], u)
        sdf = gpu.SDF3HIP(shapes[name])
        if specialise:
            sdf.specialize()
            assert sdf.info()["specialized"]
        dev = gpu.ContourHIP.slices(sdf, res, z)
        same_trace(dev, contourref.of_oracle(shapes[name].tree(), res, z), (name, k))
        out[name] = (dev, chain(gpu, dev, res, (name, k, "chain"), True))
    return out


@pytest.fixture(scope="module")
def traced_base(gpu):
    return outlines(gpu, 0), slices(gpu, 0)


@pytest.mark.parametrize("k", RUNGS)
def test_outlines_on_the_ladder(gpu, traced_base, k):
    got = outlines(gpu, k)
    assert len(got) >= 41 and k in L.TRACER_COVARIANT
    for name, (dev, ch) in got.items():
        dev0, ch0 = traced_base[0][name]
        assert L.contour_differ(dev0, dev, k) == [], (name, k)
        if ch is not None:
            assert chain_differ(ch0, ch, k) == [], (name, k)


@pytest.mark.parametrize("k", MESH_RUNGS)
def test_slices_on_the_ladder(gpu, traced_base, k):
    assert k in L.SLICES_COVARIANT
    for name, (dev, ch) in slices(gpu, k).items():
        dev0, ch0 = traced_base[1][name]
        assert dev.n_layers == 4 and L.contour_differ(dev0, dev, k) == [], (name, k)
        assert chain_differ(ch0, ch, k) == [], (name, k)
        assert len(set(ch[4].cls.tolist())) > 1, (name, k)


@pytest.mark.parametrize("which", ["lowest", "highest"])
def test_per_tree_builds_on_the_extreme_rungs(gpu, traced_base, which):
    """The chain shapes and the slices through specialize(), five builds side by side (tests/par.py): the same bytes as the twins, and
    covariant with the interpreter's base rung."""
    k = RUNGS[0] if which == "lowest" else RUNGS[-1]

    def one(name):
        if name in L.SLICE_SHAPES:
            return 1, name, slices(gpu, k, (name,), specialise=True)[name]
        return 0, name, outlines(gpu, k, (name,), specialise=True).get(name)

    done = 0
    for dim, name, r in par.pmap(one, list(L.CHAIN_SHAPES + L.SLICE_SHAPES), workers=5):
        if r is None:                       # (a shape whose oracle ladder ends before this rung: RANGE in tests/test_scale_ref.py)
            assert k not in rungs_of(name)
            continue
        dev0, ch0 = traced_base[dim][name]
        assert L.contour_differ(dev0, r[0], k) == [] and chain_differ(ch0, r[1], k) == [], (name, k)
        done += 1
    assert done >= 4
