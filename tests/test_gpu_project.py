"""gsdf_hip_indexed_project on the device against the numpy twin of its contract (tests/projectref.py) over the oracle's evaluator:
positions, d_before and d_after equal BIT FOR BIT, the status bytes and the stats' leading block equal as bytes, and the program's
evaluation counter grows by exactly st.evals. The twin sees the vertices and the options, and no device result."""
import ctypes as C

import numpy as np
import pytest

import projectref as P
import toporef as T
from corpus import shapes3d
from oracle.oracle import OracleSDF
from scaffold.builder import Builder
from test_gpu_nan import degenerate_trees, relation
from test_gpu_simplify import small
from test_gpu_topo import check_against_twin as check_report
from test_gpu_weld import SMALL

pytestmark = pytest.mark.gpu
F = np.float32


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def opts_for(res, max_iters=8):
    return dict(step=F(res / F(4)), tol=F(res / F(1024)), max_move=F(F(4) * res), max_iters=max_iters)


def same_bits(a, b, what):
    bad = np.flatnonzero((u32(a) != u32(b)).reshape(len(a), -1).any(axis=1))
    assert bad.size == 0, (what, bad.size, bad[:6].tolist(), np.asarray(a)[bad[:3]].tolist(), np.asarray(b)[bad[:3]].tolist())


def check(ix, sdf, fn, v, what="", **o):
    """Device projection of handle `ix` (vertices v) through program `sdf` against the twin's over the distance function `fn`: the
    result, the fit, the stats, the evaluation counter and the dry run. Returns (device mesh, device stats, twin result)."""
    e0 = sdf.Evaluations()
    dev, st = ix.project(sdf, **o)
    assert sdf.Evaluations() - e0 == st.evals, (what, sdf.Evaluations() - e0, st.evals)
    counted = P.CountingSDF(fn)
    pos, db, da, status, ts = P.project(counted, v, **o)
    got = {"n_verts": st.n_verts, "count": list(st.count), "evals": st.evals, "over": (st.over_tol_before, st.over_tol_after),
           "max": (st.max_abs_before, st.max_abs_after), "steps_max": st.steps_max}
    want = {"n_verts": ts["n_verts"], "count": ts["count"].tolist(), "evals": ts["evals"], "over": (ts["over_tol_before"], ts["over_tol_after"]),
            "max": (float(ts["max_abs_before"]), float(ts["max_abs_after"])), "steps_max": ts["steps_max"]}
    print(what, o["max_iters"], {P.STATUS[k]: c for k, c in enumerate(got["count"]) if c}, "evals", st.evals, "max |d|", got["max"], "steps_max", st.steps_max,
          "ms", st.ms_device)
    assert got == want, (what, got, want)
    assert st.result_bytes() == P.stats_bytes(ts) and counted.count == st.evals
    v2, _, _ = dev.read()
    b2, a2, s2 = dev.fit()
    assert s2.tobytes() == status.tobytes(), (what, np.flatnonzero(s2 != status)[:8].tolist())
    same_bits(v2, pos, (what, "positions"))
    same_bits(b2, db, (what, "d_before"))
    same_bits(a2, da, (what, "d_after"))
    none, dry = ix.project(sdf, dry=True, **o)
    assert none is None and dry.result_bytes() == st.result_bytes()
    return dev, st, (pos, db, da, status, ts)


@pytest.mark.parametrize("name", sorted(T.hand_meshes()))
def test_hand_meshes(gpu, name):
    """Against a sphere of radius 5 about the origin: unused vertices, degenerate faces, a NaN vertex (tet-nan: SKIPPED), the vertex
    at the very centre (the six taps cancel: FLAT), V of 4 .. 16."""
    v, i = T.hand_meshes()[name]
    shape = Builder().NewSphere(5)
    sdf, cpu = gpu.SDF3HIP(shape), OracleSDF(shape.tree())
    ix = gpu.IndexedHIP.from_arrays(v, i)
    for o in (dict(step=0.25, tol=1e-4, max_move=30.0, max_iters=8), dict(step=0.25, tol=1e-4, max_move=0.5, max_iters=2)):
        dev, st, tw = check(ix, sdf, cpu.Evaluate, v, name, **o)
        _, i2, k2 = dev.read()
        assert (i2 == i).all() and (k2 == 0).all()
    assert st.count[P.SKIPPED] == (1 if name == "tet-nan" else 0)
    if name == "tet":
        assert tw[3][0] == P.FLAT and st.count[P.CLAMPED] > 0


_simplified = {}


def simplified(gpu, name):
    """(clustered handle, its verts, idx, keys, res) of a SMALL shape at resdiv 48 welded, then simplified at 4 res; made once."""
    if name not in _simplified:
        ix, _, _, _, res, origin = small(gpu, name)
        sx, _ = ix.simplify(F(4) * res, tuple(F(o) - F(0.5) * res for o in origin))
        _simplified[name] = (sx,) + sx.read() + (res,)
    return _simplified[name]


@pytest.mark.parametrize("name", SMALL)
def test_small_shapes(gpu, name):
    sx, v, i, k, res = simplified(gpu, name)
    shape = dict(shapes3d()[1])[name]
    cpu = OracleSDF(shape.tree())
    interp, spec = gpu.SDF3HIP(shape), gpu.SDF3HIP(shape).specialize()
    for iters in (0, 1, 8):
        a, sa, tw = check(sx, interp, cpu.Evaluate, v, (name, "interpreter"), **opts_for(res, iters))
        b, sb, _ = check(sx, spec, cpu.Evaluate, v, (name, "specialised"), **opts_for(res, iters))
        assert sa.result_bytes() == sb.result_bytes() and [x.tobytes() for x in a.read() + a.fit()] == [x.tobytes() for x in b.read() + b.fit()]
    assert spec.info()["kernels"]["project"] == "project_kernel:specialised", spec.info()["kernels"]
    assert interp.info()["kernels"]["project"] == "project_kernel:interpreter", interp.info()["kernels"]
    # the result: the input's faces and keys, no normals, and an ordinary handle whose report is the twin's of the twin's positions
    v2, i2, k2 = a.read()
    assert i2.tobytes() == i.tobytes() and k2.tobytes() == k.tobytes() and a.stats.has_normals == 0 and (a.n_verts, a.n_tris) == (sx.n_verts, sx.n_tris)
    check_report(a, tw[0], i)
    if name in ("sphere", "torus"):
        assert set(np.unique(tw[3])) <= {P.ON, P.CONVERGED} and sa.over_tol_after == 0


def test_dry_run_and_deviation(gpu):
    sx, v, i, _, res = simplified(gpu, "torus")
    shape = dict(shapes3d()[1])["torus"]
    sdf = gpu.SDF3HIP(shape)
    o = opts_for(res)
    full, st = sx.project(sdf, **o)
    e0 = sdf.Evaluations()
    none, dry = sx.project(sdf, dry=True, **o)
    assert none is None and dry.result_bytes() == st.result_bytes() and sdf.Evaluations() - e0 == st.evals
    e0 = sdf.Evaluations()
    dv = sx.deviation(sdf, o["tol"])
    _, zero = sx.project(sdf, **opts_for(res, 0))
    assert dv.result_bytes() == zero.result_bytes() and sdf.Evaluations() - e0 == 2 * len(v) and dv.evals == len(v)
    assert dv.max_abs_before == dv.max_abs_after == st.max_abs_before and dv.count[P.ITERS] == dv.over_tol_before == st.over_tol_before
    po = gpu.ProjectOpts(step=o["step"], tol=o["tol"], max_move=o["max_move"], max_iters=8)
    assert gpu.lib().gsdf_hip_indexed_project(sx._h, sdf._h, C.byref(po), None, None) == -3      # neither a handle nor stats asked for
    # extract and simplify of the result carry no fit
    for other in (full.extract(), full.simplify(res * F(2.0 ** -12))[0], sx):
        with pytest.raises(gpu.HipError) as e:
            other.fit()
        assert e.value.code == -3 and "gsdf_hip_indexed_project" in e.value.msg
    a = np.empty(len(v), F)
    assert gpu.lib().gsdf_hip_indexed_read_fit(full._h, None, a.ctypes.data, None) == 0 and (u32(a) == u32(full.fit()[1])).all()   # each output optional


def test_non_finite_vertices_are_skipped(gpu):
    sx, v, i, k, res = simplified(gpu, "sphere")
    shape = dict(shapes3d()[1])["sphere"]
    sdf, cpu = gpu.SDF3HIP(shape), OracleSDF(shape.tree())
    vn = v.copy()
    bad = np.arange(3, len(v), 7)
    vn[bad, np.arange(len(bad)) % 3] = np.resize(np.array([np.nan, np.inf, -np.inf], F), len(bad))
    ix = gpu.IndexedHIP.from_arrays(vn, i, k)
    dev, st, tw = check(ix, sdf, cpu.Evaluate, vn, "non-finite vertices", **opts_for(res))
    assert st.count[P.SKIPPED] == len(bad) and (tw[3][bad] == P.SKIPPED).all() and st.evals == tw[4]["evals"]
    v2 = dev.read()[0]
    assert (u32(v2[bad]) == u32(vn[bad])).all() and (u32(dev.fit()[0][bad]) == 0x7fc00000).all()


def test_degenerate_fields(gpu):
    """Trees whose distance is NaN or infinite in places (tests/test_gpu_nan.py). Where the reference's distance is NaN the device
    returns NaN or a stand-in (the relation that file states), so the device is held to the oracle through d_before, by that relation;
    the projection itself -- positions, statuses, stats, every bit -- is held to the twin over the device's own evaluator."""
    rng = np.random.default_rng(47)
    seen = np.zeros(8, np.int64)
    for name, t in degenerate_trees():
        bb = np.array(t.bb[:], F)
        c, hs = (bb[:3] + bb[3:]) / 2, np.maximum((bb[3:] - bb[:3]) / 2, 0.25) * F(1.2)
        v = np.concatenate([(c + (rng.random((700, 3), F) * 2 - 1) * hs).astype(F), F(0.25) * rng.integers(-6, 7, (300, 3)).astype(F)])
        i = rng.integers(0, len(v), (500, 3)).astype(np.uint32)
        sdf = gpu.SDFHIP(t)
        ix = gpu.IndexedHIP.from_arrays(v, i)
        res = F(np.linalg.norm(bb[3:] - bb[:3]) / 48)
        o = dict(step=F(res / F(4)), tol=F(res / F(1024)), max_move=F(F(8) * res), max_iters=6)
        e0 = sdf.Evaluations()
        dev, st = ix.project(sdf, **o)
        assert sdf.Evaluations() - e0 == st.evals
        b2, a2, s2 = dev.fit()
        relation(b2, OracleSDF(t).Evaluate(v), (name, "d_before"))
        pos, db, da, status, ts = P.project(lambda p: sdf.Evaluate(p), v, **o)
        assert s2.tobytes() == status.tobytes(), (name, np.flatnonzero(s2 != status)[:8].tolist(), s2[s2 != status][:8], status[s2 != status][:8])
        same_bits(dev.read()[0], pos, (name, "positions"))
        for got, want in ((b2, db), (a2, da)):
            nan = np.isnan(want)
            assert (np.isnan(got) == nan).all() and (u32(got)[~nan] == u32(want)[~nan]).all(), name
        assert st.result_bytes() == P.stats_bytes(ts), (name, list(st.count), ts["count"].tolist())
        with np.errstate(invalid="ignore"):
            assert not (np.abs(a2) > np.abs(b2)).any()
        seen += ts["count"]
        print(name, {P.STATUS[k]: int(n) for k, n in enumerate(ts["count"]) if n})
    # a NaN reaches the root where no min / max / clamp stands behind it (shell-zero: 0 x inf): NONFINITE on the device itself; FLAT and
    # REVERTED are forced on the device by test_flat_and_reverted_on_an_ordinary_field
    assert seen[P.NONFINITE] > 0, seen.tolist()


def test_flat_and_reverted_on_an_ordinary_field(gpu):
    """A unit sphere, bit for bit against the twin over the oracle. The centre: the six taps cancel, FLAT. A point h / 10 from the centre:
    g.x = 2 x, so the one step lands about h / x = 10 radii out, |d| grows from 1 to 9, and with one trip it ends there: REVERTED.
    With more trips the same vertex comes back from there and converges."""
    shape = Builder().NewSphere(1)
    sdf, cpu = gpu.SDF3HIP(shape), OracleSDF(shape.tree())
    h = F(F(0.01) * F(0.5))
    v = np.array([[h / F(10), 0, 0], [0, 0, 0], [0.3, 0.2, 0.1], [0, h / F(10), 0]], F)
    ix = gpu.IndexedHIP.from_arrays(v, np.array([[0, 1, 2], [1, 2, 3]], np.uint32))
    for form in ("interpreter", "specialised"):
        dev, st, tw = check(ix, sdf, cpu.Evaluate, v, ("sphere", form), step=F(0.01), tol=F(1e-5), max_move=F(100), max_iters=1)
        assert tw[3].tolist() == [P.REVERTED, P.FLAT, P.ITERS, P.REVERTED] and st.steps_max == 1
        b2, a2, s2 = dev.fit()
        assert s2.tolist() == tw[3].tolist() and (u32(dev.read()[0]) == u32(v))[[0, 1, 3]].all() and (u32(a2) == u32(b2))[[0, 1, 3]].all()
        _, st8, tw8 = check(ix, sdf, cpu.Evaluate, v, ("sphere", form), step=F(0.01), tol=F(1e-5), max_move=F(100), max_iters=8)
        assert tw8[3].tolist() == [P.CONVERGED, P.FLAT, P.CONVERGED, P.CONVERGED]
        sdf.specialize()


def test_max_move_zero_moves_nothing(gpu):
    sx, v, i, _, res = simplified(gpu, "sphere")
    shape = dict(shapes3d()[1])["sphere"]
    sdf, cpu = gpu.SDF3HIP(shape), OracleSDF(shape.tree())
    o = dict(opts_for(res), max_move=F(0))
    dev, st, tw = check(sx, sdf, cpu.Evaluate, v, "max_move 0", **o)
    assert (u32(dev.read()[0]) == u32(v)).all() and st.steps_max == 0
    assert st.over_tol_before > 0 and st.count[P.CLAMPED] == st.over_tol_before == st.over_tol_after and st.count[P.ON] == len(v) - st.over_tol_before


def test_errors(gpu):
    v, i = T.hand_meshes()["tet"]
    ix = gpu.IndexedHIP.from_arrays(v, i)
    b = Builder()
    sdf = gpu.SDF3HIP(b.NewSphere(5))
    good = dict(step=0.25, tol=1e-4, max_move=1.0, max_iters=8)
    for bad in (dict(step=0.0), dict(step=-1.0), dict(step=float("inf")), dict(step=float("nan")), dict(tol=-1e-3), dict(tol=float("inf")),
                dict(tol=float("nan")), dict(max_move=-1.0), dict(max_move=float("inf")), dict(max_move=float("nan")), dict(max_iters=-1), dict(max_iters=65)):
        with pytest.raises(P.ProjectError):
            P.check_opts(**{**good, **bad})
        for dry in (False, True):
            with pytest.raises(gpu.HipError) as e:
                ix.project(sdf, dry=dry, **{**good, **bad})
            assert e.value.code == -3, bad
    po = gpu.ProjectOpts(step=0.25, tol=1e-4, max_move=1.0, max_iters=8, flags=1)
    h, st = C.c_void_p(0x1234), gpu.ProjectStats(n_verts=77)
    assert gpu.lib().gsdf_hip_indexed_project(ix._h, sdf._h, C.byref(po), C.byref(h), C.byref(st)) == -3
    assert not h.value and st.n_verts == 77                                  # on an error *out is NULL and *st is not written
    flat2d = gpu.SDF2HIP(b.NewCircle(1))
    for dry in (False, True):
        with pytest.raises(gpu.HipError) as e:
            ix.project(flat2d, dry=dry, **good)
        assert e.value.code == -7                                             # GSDF_ERR_DIMENSION
    with pytest.raises(gpu.HipError) as e:
        ix.fit()
    assert e.value.code == -3
    ix.project(sdf, **{**good, "max_iters": 64})                             # the bounds themselves are fine
    ix.project(sdf, **{**good, "max_iters": 0, "tol": 0.0, "max_move": 0.0})


def test_whole_waves_of_one_value(gpu):
    """70 000 copies of one off-surface point: 273 whole workgroups and a ragged tail of 112 lanes, every one the same result."""
    shape = Builder().NewSphere(1)
    sdf, cpu = gpu.SDF3HIP(shape), OracleSDF(shape.tree())
    n = 70000
    v = np.tile(np.array([[0.3, -0.8, 0.75]], F), (n, 1))
    i = np.array([[0, 1, 2]], np.uint32)
    ix = gpu.IndexedHIP.from_arrays(v, i)
    o = dict(step=F(0.01), tol=F(1e-5), max_move=F(1), max_iters=8)
    pos, db, da, status, ts = P.project(cpu.Evaluate, v[:1], **o)
    e0 = sdf.Evaluations()
    dev, st = ix.project(sdf, **o)
    assert status[0] == P.CONVERGED and st.evals == n * ts["evals"] == sdf.Evaluations() - e0
    assert list(st.count) == [n if k == P.CONVERGED else 0 for k in range(8)] and st.steps_max == ts["steps_max"]
    b2, a2, s2 = dev.fit()
    assert (u32(dev.read()[0]) == u32(pos[0])).all() and (u32(b2) == u32(db[0])).all() and (u32(a2) == u32(da[0])).all() and (s2 == P.CONVERGED).all()
    assert (st.max_abs_before, st.max_abs_after, st.over_tol_before, st.over_tol_after) == (abs(float(db[0])), abs(float(da[0])), n, 0)
