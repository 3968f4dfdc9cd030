"""The reference's evaluators and renderers across units, oracle only: what holds on the CPU before the device is asked for it.

tests/scaled_corpus.py rebuilds the corpus with every length multiplied by u = 2^k. The reference's arithmetic is float32 with no
absolute constant in nearly every node, so evaluating the scaled tree at u p gives u times the base distance BIT FOR BIT, and the
renderers produce u times the base triangles. Each ladder below is a literal: the rungs over which the ORACLE passes, found here, with
the cause of each end that falls short of +-40. tests/test_gpu_scale.py holds the device to the oracle on the same rungs.
"""
import numpy as np
import pytest

import corpus
import dcref
import scaled_corpus as SC
from gsdf_amd import hip
from oracle.oracle import OracleSDF
from scaffold.builder import Builder, NutHex
from test_lowering import decode

F = np.float32

# k of u = 2^k: steps of at most 10 from -40 to 40 (0 is the base rung, tests/corpus.py itself), and +-8: a unit near millimetres or
# inches against metres (2^8 = 256, 2^-8 = 0.004), the scaling ordinary CAD input has
RUNGS = (-40, -30, -20, -10, -8, 8, 10, 20, 30, 40)
# shapes with a shorter range: (lowest, highest) rung of RUNGS at which the oracle is homogeneous
#   line         NewLine2D turns a line shorter than epstol = 6e-7 (an absolute length; the reference's primitives2d.go:24, gsdf.go:24)
#                into a circle: 1.1 * 2^-30 is shorter, 1.1 * 2^-20 is not
#   lines        the polyline starts its minimum over squared distances at 1e23 (cpu_evaluators.go:1145-1160): at u = 2^40 the squares
#                are of order 2^80 > 1e23 and the start value wins; 2^60 at u = 2^30 does not reach it
#   union_lines  holds both
RANGE = {"line": (-20, 40), "lines": (-40, 30), "union_lines": (-20, 30)}

# the renderers (resolution: base diagonal / 32, times u)
#   octree, flat: marching cubes snaps a corner distance closer than 1e-12 to the iso level onto it (marchcubes.go:84-90, mcInterpolate;
#                 oracle/orc_render.c: `eps = 1e-12f`), an absolute length: at u = 2^-30 corner distances of 1e-3 cell are below it and
#                 the vertices move (same triangle count, other bits); from 2^-20 up nothing is that close
#   dual contour: which cubes, which quads, their order and keys are decided by signs and by |d| >= 2 res: covariant at every rung.
#                 The vertex positions are not: the normals are central differences over an absolute step (2e-8, chiseled 1e-4) and the
#                 QR's rank tests compare against 1e-14 (dual_contour_vertexplacement.go), so a vertex whose cube touches a coordinate
#                 plane (not chiseled) or any vertex (chiseled) depends on the unit. Not chiseled, six of the seven shapes have no such
#                 vertex at this resolution and are covariant bit for bit at every rung; the smooth union has six of 1704.
MESH_RUNGS = (-40, -30, -20, -8, 8, 20, 30, 40)
MC_RUNGS = (-20, -8, 8, 20, 30, 40)
DC_VERTS_COVARIANT = ("diff", "twist", "screw_iso_ext", "circarray0", "extrude_poly", "array")


# what the lowering decides per rung (compile.cpp: recip_for grants RN(1 / d) for |d| in [2^-30, 2^30] only): k -> (the smooth combines'
# blend width and the screw's pitch, both 0.1 u: out of range at 2^40 and from 2^-30 down; the octagon, |e|^2 = 0.586 u^2: out of
# range from 2^+-20 outwards). Literal: it says which form each rung is meant to run; the CPU test reads the lowered program, the GPU
# test (tests/test_gpu_scale.py) what the handle reports.
LOWERING = {-40: ("declined", "poly_plain"), -30: ("declined", "poly_plain"), -20: ("recip", "poly_plain"), -10: ("recip", "poly_recip"),
            -8: ("recip", "poly_recip"), 0: ("recip", "poly_recip"), 8: ("recip", "poly_recip"), 10: ("recip", "poly_recip"),
            20: ("recip", "poly_plain"), 30: ("recip", "poly_plain"), 40: ("declined", "poly_plain")}


def rungs_of(name):
    lo, hi = RANGE.get(name, (-40, 40))
    return tuple(k for k in RUNGS if lo <= k <= hi)


def recip_census(code):
    """What the lowering decided about exact-reciprocal division (compile.cpp: recip_for, the polygon's bit 31), read off a lowered
    program: nodes that carry RN(1 / d), nodes it declined (word 0), polygons with and without the flag."""
    c = {"recip": 0, "declined": 0, "poly_recip": 0, "poly_plain": 0}
    for name, _, _, _, pc in decode(code):
        if name in ("D_COMBINE_SUNION", "D_COMBINE_SDIFF", "D_COMBINE_SINTER"):
            c["recip" if code[pc + 2] != 0 else "declined"] += 1
        elif name == "D_SCREW_PRE":
            c["recip" if code[pc + 6] != 0 else "declined"] += 1
        elif name == "D_POLY2D":
            c["poly_recip" if int(code[pc + 1]) >> 31 else "poly_plain"] += 1
    return c


def test_the_base_rung_is_the_corpus():
    """u = 1: the same lowered program, slot count and bounds as tests/corpus.py's shape of that name, for every shape kept."""
    for fn in ("shapes3d", "shapes2d", "bezier2d"):
        base = dict(getattr(corpus, fn)(Builder())[1])
        mine = dict(getattr(SC, fn)(Builder(), 1.0)[1])
        assert [n for n in base if n not in mine] == (list(SC.LEFT_OUT_3D) if fn == "shapes3d" else [])
        for name, sh in mine.items():
            (c0, s0), (c1, s1) = hip.lower(base[name]), hip.lower(sh)
            assert s0 == s1 and c0.tobytes() == c1.tobytes() and base[name].Bounds().tobytes() == sh.Bounds().tobytes(), name


def test_the_shell_is_left_out_because_its_thickness_is_also_a_zoom():
    """Shell(s, t)(p) = t (|s(p / t)| - t): with s a sphere of radius r that is t (| |p| / t - r | - t) -- homogeneous under no scaling
    of r and t. The oracle restates it that way (operations.go:749-754); so the node stays out of the ladder rather than in it wrong."""
    p = F([[0.5, 0, 0], [2.0, 0, 0], [0, 3.0, 0]])
    b = Builder()
    d = OracleSDF(b.Shell(b.NewSphere(2.0), 0.25).tree()).Evaluate(p)
    want = F(0.25) * (np.abs(np.linalg.norm(p / F(0.25), axis=1).astype(F) - F(2.0)) - F(0.25))
    assert np.array_equal(d, want.astype(F))
    d2 = OracleSDF(b.Shell(b.NewSphere(4.0), 0.5).tree()).Evaluate(p * F(2))
    assert not np.array_equal(d2, d * F(2))


def test_the_nut_is_left_out_because_its_hex_comes_from_a_table():
    """threads.ISO picks the flat-to-flat distance from a table of millimetre sizes (threads.go:225-251): the bounds of the nut of an
    eight times larger thread are not eight times the bounds."""
    b = Builder()
    assert not np.array_equal(b.NutISO(24, 4.0, False, NutHex).Bounds(), b.NutISO(3, 0.5, False, NutHex).Bounds() * F(8))


@pytest.mark.parametrize("fn", ["shapes3d", "shapes2d", "bezier2d"])
def test_evaluate_is_homogeneous(fn):
    base = getattr(SC, fn)(Builder(), 1.0)[1]
    ref = {}
    for name, sh in base:
        p = corpus.sample_points(sh, n_grid=7, n_rand=1000)
        d = OracleSDF(sh.tree()).Evaluate(p)
        ref[name] = (p, d)
    for k in RUNGS:
        u = SC.unit(k)
        for name, sh in getattr(SC, fn)(Builder(), u)[1]:
            if k not in rungs_of(name):
                continue
            p, d = ref[name]
            got = OracleSDF(sh.tree()).Evaluate(SC.scaled_points(p, u))
            want = d * F(u)
            bad = int(((got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))).sum())
            assert bad == 0 and int(np.isnan(got).sum()) == int(np.isnan(d).sum()) and np.isfinite(got[~np.isnan(got)]).all(), (name, k, bad)


def test_the_short_ranges_end_where_they_are_said_to():
    """The rung past each literal end fails in the oracle: the ladder is not shorter than it has to be."""
    for name, k in (("line", -30), ("lines", 40), ("union_lines", -30), ("union_lines", 40)):
        sh0 = dict(SC.shapes2d(Builder(), 1.0)[1])[name]
        p = corpus.sample_points(sh0, n_grid=7, n_rand=300)
        d = OracleSDF(sh0.tree()).Evaluate(p)
        u = SC.unit(k)
        got = OracleSDF(dict(SC.shapes2d(Builder(), u)[1])[name].tree()).Evaluate(SC.scaled_points(p, u))
        assert not np.array_equal(got, d * F(u)), (name, k)


def _sorted(t):
    t = np.ascontiguousarray(t, np.float32).reshape(-1, 9)
    return t[np.lexsort(t.view(np.uint32).T[::-1])]


def base_meshes():
    """name -> (res, octree MeshResult, flat MeshResult, [dcref.mesh(...)[:3] not chiseled, chiseled]) at u = 1."""
    out = {}
    for name, sh in SC.mesh_shapes(Builder(), 1.0)[1]:
        cpu = OracleSDF(sh.tree())
        res = F(float(sh.Diagonal()) / 32)
        out[name] = (res, cpu.render_octree(res, 4096, True), cpu.render_flat(res, 4096, 2), [dcref.mesh(cpu, res, ch)[:3] for ch in (False, True)])
    return out


@pytest.fixture(scope="module")
def meshes():
    return base_meshes()


@pytest.mark.parametrize("k", MESH_RUNGS)
def test_renderers_are_covariant(meshes, k):
    u = SC.unit(k)
    fu = F(u)
    for name, sh in SC.mesh_shapes(Builder(), u)[1]:
        res, oc, fl, dc = meshes[name]
        assert oc.n_tris > 1000, name
        cpu = OracleSDF(sh.tree())
        r = F(res * fu)
        o2, f2 = cpu.render_octree(r, 4096, True), cpu.render_flat(r, 4096, 2)
        assert (o2.n_tris, o2.pruned) == (oc.n_tris, oc.pruned) and (f2.n_tris, f2.evals) == (fl.n_tris, fl.evals), (name, k)
        if k in MC_RUNGS:
            assert _sorted(o2.tris).tobytes() == _sorted(oc.tris * fu).tobytes(), (name, k, "octree")
            assert _sorted(f2.tris).tobytes() == _sorted(fl.tris * fu).tobytes(), (name, k, "flat")
        for ci, ch in enumerate((False, True)):
            v, i, key = dcref.mesh(cpu, r, ch)[:3]
            v0, i0, key0 = dc[ci]
            assert key.tobytes() == key0.tobytes() and i.tobytes() == i0.tobytes(), (name, k, "dual contouring", ch)
            if not ch and name in DC_VERTS_COVARIANT:
                assert v.tobytes() == (v0 * fu).astype(F).tobytes(), (name, k, "dual contouring vertices")


def test_the_ladder_reaches_the_other_lowering():
    """recip_for grants RN(1 / d) for d in [2^-30, 2^30] only, and a polygon keeps its flag only if every |e|^2 is in that range: the
    base rung takes the exact-reciprocal forms everywhere, the far rungs must not."""
    def census(k):
        u = SC.unit(k)
        d3, d2 = dict(SC.shapes3d(Builder(), u)[1]), dict(SC.shapes2d(Builder(), u)[1])
        return {n: recip_census(hip.lower(s)[0]) for n, s in list(d3.items()) + list(d2.items())}
    base = census(0)
    assert base["smoothunion"] == {"recip": 1, "declined": 0, "poly_recip": 0, "poly_plain": 0}
    assert base["screw_iso_ext"]["recip"] == 1 and base["screw_iso_ext"]["poly_recip"] == 1
    assert base["poly"] == {"recip": 0, "declined": 0, "poly_recip": 1, "poly_plain": 0}
    assert sum(c["declined"] + c["poly_plain"] for c in base.values()) == 0
    for k, (smooth, poly) in LOWERING.items():
        if k == 0:
            continue
        c = census(k)
        for n in ("smoothunion", "smoothdiff", "smoothintersect"):
            assert c[n][smooth] == 1 and c[n]["recip"] + c[n]["declined"] == 1, (k, n, c[n])
        assert c["screw_iso_ext"][smooth] == 1, (k, c["screw_iso_ext"])
        assert c["poly"][poly] == 1 and c["poly"]["poly_recip"] + c["poly"]["poly_plain"] == 1, (k, c["poly"])
