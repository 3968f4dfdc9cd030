"""The device against the oracle across float32 magnitudes: parts in other units, and positions far from and deep inside a part.

The rest of the suite lives at dimensions and coordinates of order 1. There every divisor is inside recip_for's [2^-30, 2^30], every
polygon keeps its reciprocal flag, every wave vote with a range guard (div_uniform_k, sqrt_k, atan2_shared, cossin_voted, hypot_k,
smooth_h) sees waves that are uniformly in range, and every margin written around order-1 numbers (gate_far, poly_cull, region_lb_zcyl,
smooth_h's 1.001, GSDF_LIP_BIG) is padding around order-1 numbers. Here:

  (a) tests/scaled_corpus.py's shapes, every length times u = 2^k, on the rungs over which the ORACLE is homogeneous
      (tests/test_scale_ref.py: RUNGS, RANGE): Evaluate of host buffers and of device buffers against the oracle of the scaled tree, bit
      for bit, and what the lowering decided about division on every rung (info()["recip"]) against a literal table -- the ladder
      reaches the IEEE-division form of the smooth combines and the screw and the polygon without its flag;
  (b) eight shapes -- one per vote, the polygon, the circular array -- through specialize() at the base rung and at both ends;
  (c) the meshers, normals and render3 on seven shapes per rung, against the oracle's meshes of the scaled tree; the welded mesh,
      its report and its simplification against the twins of their contracts and, in order-free form, against the BASE rung's;
  (d) every shape of tests/corpus.py, unit scale, at sample positions times 2^k, k from -70 to 40: rung by rung (whole waves in one
      regime) and as one batch with the rungs interleaved by a fixed permutation (the lanes of a wave straddle every guard), through
      the interpreter and through the per-tree builds of (b).

Bit for bit wherever the oracle is a number (_mismatch_ref); the quadratic bezier within REL_TOL, its absolute floor scaled with u.

Time, one run on one MI355X machine: this file 21 s (36 cases) and tests/test_gpu_math.py 2.8 s (27 cases); the whole GPU suite
with them 768 s (471 cases), so the rest, which is the parent commit's suite (408 cases), about 744 s. Per case: a rung of (a) 0.08-0.22 s
(33 or 45 trees, an oracle and two device evaluations each; the first case also loads the libraries, 1.4 s); the position ladder
of (d) 0.15 s per dimension; eight per-tree builds side by side 4.4-4.5 s (each build a compiler run of 1-4 s), the slowest; a
rung of (c) 0.2-0.3 s (seven shapes, every mesher, the chain with its three twins).
"""
import numpy as np
import pytest

import corpus
import dcref
import par
import scaled_corpus as SC
import viewref
from oracle.oracle import OracleSDF
from scaffold.builder import Builder
from test_gpu_eval import REL_TOL
from test_gpu_simplify import check as simplify_against_twin
from test_gpu_topo import check_against_twin as report_against_twin
from test_gpu_variants import _mismatch, _mismatch_ref, _points, _same_tris
from test_gpu_view import _same as same_frame
from test_gpu_weld import check_against_twin as weld_against_twin
from test_scale_ref import LOWERING, MC_RUNGS, MESH_RUNGS, RUNGS, rungs_of

pytestmark = pytest.mark.gpu
F = np.float32

# the points of a shape: test_gpu_variants._points over the BASE shape's bounds (seed = the shape's place in its list), times u.
# At how many of them the oracle is NaN: none, but the ellipse's l = 0 on an axis (0 / 0), on every rung alike.
NAN_POINTS = {"ellipse": 2}


def _close(got, want, floor):
    """Largest relative difference (the bezier's tolerance test); NaN if the device gives a NaN or an infinity, which then fails."""
    return float(np.max(np.abs(got - want) / np.maximum(np.abs(want), floor)))


def _eval_both(sdf, pos):
    """Host-buffer Evaluate and evaluate_dev of the same points (the handle's own kernel on device tensors)."""
    import torch
    host = sdf.Evaluate(pos)
    tp = torch.from_numpy(pos).cuda()
    td = torch.full((len(pos) + 1,), float("nan"), device="cuda")
    torch.cuda.synchronize()
    sdf.evaluate_dev(tp.data_ptr(), 4 * pos.shape[1], td.data_ptr(), len(pos))
    torch.cuda.synchronize()
    dev = td.cpu().numpy()
    assert np.isnan(dev[-1]), "wrote past n"
    return host, dev[:-1]


def _compare(sdf, pos, want, floor=None):
    """[(how, number of differing points)] that differ; floor: the bezier's tolerance instead of bits."""
    out = []
    for how, got in zip(("host buffer", "device buffer"), _eval_both(sdf, pos)):
        if floor is not None:
            worst = _close(got, want, floor)
            if not worst <= REL_TOL:
                out.append((how, worst))
        elif _mismatch_ref(got, want):
            k = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)) & ~np.isnan(want))
            out.append((how, len(k), pos[k[:2]].tolist(), got[k[:2]].tolist(), want[k[:2]].tolist()))
    return out


def _scaled(dim, u):
    b = Builder()
    return SC.shapes3d(b, u)[1] if dim == 3 else SC.shapes2d(b, u)[1] + SC.bezier2d(b, u)[1]


# ---- (a) every shape on every rung the oracle passes

@pytest.mark.parametrize("k", (0,) + RUNGS)
@pytest.mark.parametrize("dim", [3, 2])
def test_evaluate_on_the_ladder(gpu, dim, k):
    u = SC.unit(k)
    base = dict(_scaled(dim, 1.0))
    bad, census = [], {}
    for j, (name, sh) in enumerate(_scaled(dim, u)):
        if k != 0 and k not in rungs_of(name):
            continue
        sdf = gpu.SDFHIP(sh)
        census[name] = sdf.info()["recip"]
        pos = SC.scaled_points(_points(base[name], j), u)
        want = OracleSDF(sh.tree()).Evaluate(pos)
        assert int(np.isnan(want).sum()) == NAN_POINTS.get(name, 0) and np.isfinite(want[~np.isnan(want)]).all(), (name, k, int(np.isnan(want).sum()))
        bad += [(name, k) + d for d in _compare(sdf, pos, want, floor=1e-3 * u if name == "quadbezier" else None)]
    print("rung", k, "dim", dim, "shapes", len(census), "differing", bad)
    smooth, poly = LOWERING[k]
    if dim == 3:
        for n in ("smoothunion", "smoothdiff", "smoothintersect"):
            assert census[n][smooth] == 1 and census[n]["recip"] + census[n]["declined"] == 1, (k, n, census[n])
        assert census["screw_iso_ext"][smooth] == 1, (k, census["screw_iso_ext"])   # (the pitch)
    else:
        assert census["poly"][poly] == 1 and census["poly"]["poly_recip"] + census["poly"]["poly_plain"] == 1, (k, census["poly"])
    assert not bad, bad


# ---- (b), (d) per-tree builds; the position ladder

POSITION_RUNGS = (-70, -64, -50, -40, -20, 0, 10, 20, 28, 40)
ELLIPSE_RUNGS = tuple(k for k in POSITION_RUNGS if k < 28)     # from 2^28 on the oracle's ellipse is NaN at 2046 of 2049 points: left out, not masked
# one per vote with a range guard -- div_uniform_k (smooth union: the blend width; the screw: the pitch), smooth_h (smooth difference),
# atan2_shared (the screw), cossin_voted (the twist), hypot_k (the rounded cylinder), sqrt_k (the polyline, the polygon) -- plus the
# polygon and the circular array
PER_TREE = [(3, "smoothunion"), (3, "smoothdiff"), (3, "screw_iso_ext"), (3, "twist"), (3, "cylr"), (3, "circarray0"), (2, "lines"), (2, "poly")]


def _ladder_check(sdf, cpu, pos0, name):
    """(d) for one handle: rung by rung, then one interleaved batch. Returns what differs."""
    rungs = ELLIPSE_RUNGS if name == "ellipse" else POSITION_RUNGS
    floor = 1e-3 if name == "quadbezier" else None
    bad, ps, ws = [], [], []
    for k in rungs:
        pos = SC.scaled_points(pos0, SC.unit(k))
        want = cpu.Evaluate(pos)
        nan = int(np.isnan(want).sum())
        assert nan == (NAN_POINTS.get(name, 0) if k == 0 else 0) and np.isfinite(want[~np.isnan(want)]).all(), (name, k, nan)
        got = sdf.Evaluate(pos)
        if floor is not None:
            if not _close(got, want, floor) <= REL_TOL:
                bad.append((name, k, _close(got, want, floor)))
        elif _mismatch_ref(got, want):
            i = np.flatnonzero((got.view(np.uint32) != want.view(np.uint32)) & ~np.isnan(want))
            bad.append((name, k, len(i), pos[i[:2]].tolist(), got[i[:2]].tolist(), want[i[:2]].tolist()))
        ps.append(pos)
        ws.append(want)
    perm = np.random.default_rng(5).permutation(len(rungs) * len(pos0))     # fixed: neighbouring lanes come from different rungs
    pos, want = np.ascontiguousarray(np.concatenate(ps)[perm]), np.concatenate(ws)[perm]
    bad += [(name, "interleaved") + d for d in _compare(sdf, pos, want, floor)]
    return bad


@pytest.mark.parametrize("dim", [3, 2])
def test_positions_far_from_and_deep_inside_a_unit_tree(gpu, dim):
    b = Builder()
    shapes = corpus.shapes3d(b)[1] if dim == 3 else corpus.shapes2d(b)[1] + corpus.bezier2d(b)[1]
    bad = []
    for j, (name, sh) in enumerate(shapes):
        bad += _ladder_check(gpu.SDFHIP(sh), OracleSDF(sh.tree()), _points(sh, j), name)
    print("position ladder, dim", dim, "shapes", len(shapes), "differing", bad)
    assert not bad, bad


@pytest.mark.parametrize("which", ["base", "lowest", "highest"])
def test_per_tree_builds_on_the_ladder(gpu, which):
    """Eight builds side by side (tests/par.py). At the base rung the handles also climb the position ladder of (d)."""
    def check(item):
        j, (dim, name) = item
        ks = rungs_of(name)
        k = {"base": 0, "lowest": ks[0], "highest": ks[-1]}[which]
        u = SC.unit(k)
        base, sh = dict(_scaled(dim, 1.0))[name], dict(_scaled(dim, u))[name]
        sdf = gpu.SDFHIP(sh).specialize()
        info = sdf.info()
        assert info["specialized"] and info["kernels"]["eval"].endswith(":specialised"), (name, k, info["kernels"])
        pos = SC.scaled_points(_points(base, j), u)
        cpu = OracleSDF(sh.tree())
        bad = [(name, k, "specialised") + d for d in _compare(sdf, pos, cpu.Evaluate(pos))]
        if which == "base":
            bad += [("specialised",) + d for d in _ladder_check(sdf, cpu, _points(base, j), name)]
        return bad
    bad = [d for r in par.pmap(check, list(enumerate(PER_TREE)), workers=8) for d in r]
    print("per-tree builds,", which, "differing", bad)
    assert not bad, bad


# ---- (c) meshers, normals, render3, the indexed chain

# The welded mesh is a function of the mesher's records IN THEIR ORDER, and that order differs from run to run (gsdf_hip.h, "simplify":
# "floats whose last bits depend on which leaf's copy the weld kept, i.e. on the mesher's record order"). So idx, keys and verts of two
# runs -- of one tree, let alone of two rungs -- are not equal byte for byte, and the chain is held in two ways: every rung's weld, report
# and simplification against the twins of their contracts on that run's own records (weldref, toporef, simplifyref: exact), and against
# the BASE rung in the form the contract makes run-independent: the set of keyed vertices and of faces over keys, the counts, edge
# classes, shells and Euler number, the exponent shifted by k; positions within 2^-19 M, M the largest coordinate -- a copy of a vertex
# is origin + res * i (two float32 roundings) and an interpolation a + t (b - a) (three more), each at most half an ulp of a value
# below M, that is 2^-23 M: five per copy, two copies, 10 * 2^-23 M, rounded up to 16 (the t of two copies differ by ulps of distances
# below res, far less); about 4e-5 res at this resolution, where a misplaced lattice index would be 1 res -- and the measures times
# u^2, u^3, u within 1e-4 (they are sums over positions that differ by the above).

def _keyed(v, i, key):
    """Order-free form of an indexed mesh with distinct keys: (keys sorted, verts in that order, faces over keys, rotated to start at
    their smallest key, sorted)."""
    o = np.argsort(key, kind="stable")
    f = key[i]
    r = np.argmin(f, axis=1)
    f = np.stack([f[np.arange(len(f)), (r + c) % 3] for c in range(3)], axis=1)
    return key[o], v[o], f[np.lexsort(f.T[::-1])]


def _chain(gpu, sh, res, what):
    """Weld, report and simplify of one tree, each against its twin; returns the order-free forms and the report."""
    v, i, key = weld_against_twin(gpu, sh, res)
    oc = gpu.OctreeHIP(gpu.SDF3HIP(sh), res, payload=gpu.PAYLOAD_RECORDS)
    ix = oc.weld()
    v, i, key = ix.read()
    assert len(np.unique(key)) == len(key), what
    rep, _ = report_against_twin(ix, v, i)
    origin = np.array(oc.stats.origin[:], np.float32) - F(res / F(2))       # off the lattice planes, as the contract advises
    simp, _, _ = simplify_against_twin(gpu, ix, v, i, F(res * F(3)), tuple(origin))
    return _keyed(v, i, key), rep, _keyed(*simp.read())


@pytest.fixture(scope="module")
def base_rung(gpu):
    out = {}
    for name, sh in SC.mesh_shapes(Builder(), 1.0)[1]:
        res = F(float(sh.Diagonal()) / 32)
        out[name] = (res, _chain(gpu, sh, res, (name, "base")))
    return out


COUNTS = ("n_verts", "n_tris", "degenerate", "nonfinite", "used_verts", "edges", "boundary_edges", "nonmanifold_edges", "misoriented_edges",
          "n_shells", "euler", "closed_oriented")


@pytest.mark.parametrize("k", (0,) + MESH_RUNGS)
def test_meshers_on_the_ladder(gpu, base_rung, k):
    u = SC.unit(k)
    for name, sh in SC.mesh_shapes(Builder(), u)[1]:
        what = (name, k)
        res0 = base_rung[name][0]
        res = F(res0 * F(u))
        sdf, cpu = gpu.SDF3HIP(sh), OracleSDF(sh.tree())
        m = cpu.render_octree(res, 4096, True)
        assert m.n_tris > 1000, what
        meshes = {}
        for kw in ({}, {"prune": False}, {"share_corners": 1}, {"share_corners": 2}):
            oc = gpu.OctreeHIP(sdf, res, **kw)
            meshes[tuple(kw)] = oc.RenderAll()
            _same_tris(meshes[tuple(kw)], m.tris, (what, "octree", kw))
            if "prune" not in kw:
                assert oc.TotalPruned() == m.pruned, (what, kw, oc.TotalPruned(), m.pruned)
        _same_tris(meshes[()], meshes[("prune",)], (what, "pruned against unpruned"))
        ma = cpu.render_octree(res, 4096, True, assume_sdf=True)
        oa = gpu.OctreeHIP(sdf, res, assume_sdf=True)
        assert oa.TotalPruned() == ma.pruned, (what, "assume_sdf", oa.TotalPruned(), ma.pruned)
        _same_tris(oa.RenderAll(), ma.tris, (what, "octree, assume_sdf"))
        fl, mf = gpu.FlatHIP(sdf, res), cpu.render_flat(res, 4096, 2)
        assert fl.Evaluations() == mf.evals and fl.n_tris() == mf.n_tris, (what, "flat", fl.Evaluations(), mf.evals, fl.n_tris(), mf.n_tris)
        _same_tris(fl.RenderAll(), mf.tris, (what, "flat"))
        tv, ti, tk, _, _, ref = dcref.mesh(cpu, res, False)
        _same_tris(gpu.DualContourHIP(sdf, res).RenderAll(), ref.tris, (what, "dual contouring"))
        v, i, key = gpu.IndexedHIP.dual_contour(sdf, res).read()
        assert (key.tobytes(), i.tobytes(), v.tobytes()) == (tk.tobytes(), ti.tobytes(), tv.tobytes()), (what, "dual contouring, indexed")
        pos = SC.scaled_points(corpus.sample_points(dict(SC.mesh_shapes(Builder(), 1.0)[1])[name], n_grid=4, n_rand=500), u)
        step = F(1e-3 * u)
        assert _mismatch(sdf.normals(pos, step).ravel(), cpu.normals_central_diff(pos, step).ravel()) == 0, (what, "normals")
        view = gpu.view_orbit(sh.Bounds(), 0.6, 0.35)
        same_frame(sdf.render3(view, 32, 24), viewref.render(cpu.Evaluate, view, 32, 24), (what, "render3"))
        if k in MC_RUNGS:      # where the reference's marching cubes is covariant (test_scale_ref.py): the chain against the base rung's
            (key0, v0, f0), rep0, (skey0, _, sf0) = base_rung[name][1]
            (key, v, f), rep, (skey, _, sf) = _chain(gpu, sh, res, what)
            assert key.tobytes() == key0.tobytes() and f.tobytes() == f0.tobytes(), (what, "weld: keyed vertices, faces over keys")
            worst = float(np.abs(v.astype(np.float64) - v0.astype(np.float64) * u).max())
            bound = 2.0 ** -19 * float(np.abs(v0).max()) * u
            print(what, "largest |vertex - u * base vertex| / res:", worst / float(res), "bound / res:", bound / float(res))
            assert worst <= bound, (what, "weld: positions", worst / float(res), bound / float(res))
            assert [getattr(rep, c) for c in COUNTS] == [getattr(rep0, c) for c in COUNTS], (what, "report: counts")
            assert rep.exponent == rep0.exponent + k, (what, rep.exponent, rep0.exponent)
            for got, want in [(rep.area, rep0.area * u * u), (rep.volume, rep0.volume * u * u * u)] + [(g, c * u) for g, c in zip(rep.centroid, rep0.centroid)]:
                assert abs(got - want) <= 1e-4 * max(abs(want), float(np.abs(v0).max()) * u * 1e-2), (what, "report: measures", got, want)
            assert skey.tobytes() == skey0.tobytes() and sf.tobytes() == sf0.tobytes(), (what, "simplify: keyed vertices, faces over keys")
