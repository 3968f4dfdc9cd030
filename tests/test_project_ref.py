"""The numpy twin of the project contract (tests/projectref.py) over the oracle's evaluator: what the contract guarantees, on meshes
from the oracle's mesher welded by weldref and clustered by simplifyref (cell 4 res, the grid half a res below the lattice origin) --
and the library's side of the ABI (no GPU here).

Options everywhere: step res / 4, tol res / 1024, max_move 4 res, max_iters 8, shapes at resdiv 48."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import projectref as P
import simplifyref as S
import toporef as T
import weldref as W
from corpus import shapes3d
from oracle.oracle import OracleSDF
from test_gpu_weld import SMALL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
_made = {}


def opts_for(res, max_iters=8):
    return dict(step=F(res / F(4)), tol=F(res / F(1024)), max_move=F(F(4) * res), max_iters=max_iters)


def clustered(name):
    """(oracle, res, clustered verts, faces) of a SMALL shape at resdiv 48, made once."""
    if name not in _made:
        shape = dict(shapes3d()[1])[name]
        cpu = OracleSDF(shape.tree())
        res = F(float(shape.Diagonal()) / 48)
        origin, _ = W.lattice_of(shape.Bounds(), res)
        ref = cpu.render_octree(res)
        v, i, _, _ = W.weld(cpu, W.leaves_of_triangles(ref.tris, origin, res), origin, res)
        grid = tuple(F(o) - F(0.5) * res for o in origin)
        v2, i2, _, _ = S.simplify(v, i, F(4) * res, grid)
        _made[name] = (cpu, res, v2, i2)
    return _made[name]


def projected(name):
    key = (name, "projected")
    if key not in _made:
        cpu, res, v, _ = clustered(name)
        sdf = P.CountingSDF(cpu.Evaluate)
        _made[key] = P.project(sdf, v, **opts_for(res)) + (sdf.count,)
    return _made[key]


@pytest.mark.parametrize("name", SMALL)
def test_contract_guarantees(name):
    cpu, res, v, _ = clustered(name)
    o = opts_for(res)
    pos, db, da, status, st, counted = projected(name)
    assert pos.dtype == F and pos.shape == v.shape and status.dtype == np.uint8
    with np.errstate(invalid="ignore"):
        assert not (np.abs(da) > np.abs(db)).any()                              # never further from the surface
    u = (pos - v).astype(F)
    r = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
    assert (r <= F(o["max_move"] * o["max_move"])).all()                        # none leaves its ball
    still = np.isin(status, (P.ON, P.SKIPPED, P.REVERTED))
    assert (pos[still].view(np.uint32) == v[still].view(np.uint32)).all()
    assert st["evals"] == int((st["trips"] + 6 * st["gradients"]).sum()) == counted
    assert int(st["count"].sum()) == len(v) == st["n_verts"] and (st["count"] == np.bincount(status, minlength=8)).all()
    assert st["over_tol_after"] <= st["over_tol_before"] and st["max_abs_after"] <= st["max_abs_before"]
    assert st["steps_max"] == int(st["steps"].max()) <= 8 and len(P.stats_bytes(st)) == 112
    # d_after is the field at the result
    moved = ~still & (st["steps"] > 0)
    assert (cpu.Evaluate(pos[moved]).view(np.uint32) == da[moved].view(np.uint32)).all()
    # no trip: nothing moves, one evaluation per vertex
    p0, b0, a0, s0, st0 = P.project(cpu.Evaluate, v, **opts_for(res, 0))
    assert (p0.view(np.uint32) == v.view(np.uint32)).all() and st0["evals"] == len(v) and st0["steps_max"] == 0
    assert (b0.view(np.uint32) == a0.view(np.uint32)).all() and (b0.view(np.uint32) == db.view(np.uint32)).all()
    assert set(np.unique(s0)) <= {P.ON, P.ITERS} and st0["over_tol_before"] == st0["over_tol_after"] == st0["count"][P.ITERS]
    print(name, "V", len(v), {P.STATUS[k]: int(c) for k, c in enumerate(st["count"]) if c}, "max |d| / res", float(st["max_abs_before"] / res),
          "->", float(st["max_abs_after"] / res), "steps_max", st["steps_max"], "evals", st["evals"])


@pytest.mark.parametrize("name", ["sphere", "torus"])
def test_smooth_distance_fields_converge(name):
    _, _, _, status, st, _ = projected(name)
    assert set(np.unique(status)) <= {P.ON, P.CONVERGED}, {P.STATUS[k]: int(c) for k, c in enumerate(st["count"]) if c}
    assert st["over_tol_after"] == 0 and st["count"][P.CONVERGED] > 0


def test_sphere_volume_comes_back():
    _, _, v, i = clustered("sphere")
    pos = projected("sphere")[0]
    want = 4.0 * math.pi / 3.0
    before, after = T.analyse(v, i)["report"]["volume"], T.analyse(pos, i)["report"]["volume"]
    print("sphere volume: clustered", before, "projected", after, "4 pi / 3", want)
    assert abs(after - want) < abs(before - want)


def test_statuses_by_hand():
    """A unit sphere's field in float32 numpy: a point on it, one off it, a NaN vertex, a NaN field, a flat field, a clamp, and a field
    that gets worse."""
    sphere = lambda p: (np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]) - F(1)).astype(F)
    v = np.array([[1, 0, 0], [0, 1.25, 0], [np.nan, 0, 0], [0, 0, np.inf], [0, 0, 0.5]], F)
    pos, db, da, s, st = P.project(sphere, v, 0.01, 1e-5, 0.4, 8)
    assert s.tolist() == [P.ON, P.CONVERGED, P.SKIPPED, P.SKIPPED, P.CLAMPED]
    assert pos[0].tolist() == [1, 0, 0] and abs(float(pos[1, 1]) - 1) <= 1e-5 and pos[1, 0] == 0 and pos[1, 2] == 0
    assert np.isnan(pos[2, 0]) and np.isinf(pos[3, 2]) and db[2:4].view(np.uint32).tolist() == [0x7fc00000] * 2 == da[2:4].view(np.uint32).tolist()
    assert pos[4].tolist() == [0, 0, 0.5] and da[4] == db[4] == -0.5 and st["steps"][4] == 0   # the one step to z = 1 would leave the ball of 0.4
    assert st["count"].tolist() == [2, 1, 1, 0, 0, 1, 0, 0] and st["over_tol_before"] == 2 and st["over_tol_after"] == 1
    assert st["evals"] == int((st["trips"] + 6 * st["gradients"]).sum()) and st["trips"][2] == 0
    assert float(st["max_abs_before"]) == 0.5
    one = np.array([[0, 0, 2]], F)
    assert P.project(lambda p: np.full(len(p), np.nan, F), one, 0.01, 0, 1, 8)[3].tolist() == [P.NONFINITE]
    assert P.project(lambda p: np.full(len(p), 3, F), one, 0.01, 0, 1, 8)[3].tolist() == [P.FLAT]
    assert P.project(sphere, one, 0.01, 1e-5, 0, 8)[3].tolist() == [P.CLAMPED]
    assert P.project(sphere, one, 0.01, 1e-5, 4, 0)[3].tolist() == [P.ITERS]
    # a field whose Newton step overshoots to a worse place: d = z^(1/3) (the step from z goes to -2 z)
    p2, b2, a2, s2, st2 = P.project(lambda p: np.cbrt(p[:, 2]).astype(F), np.array([[0, 0, 0.5]], F), 1e-3, 1e-6, 100, 3)
    assert s2.tolist() == [P.REVERTED] and p2.tolist() == [[0, 0, 0.5]] and a2.tolist() == b2.tolist() and st2["steps_max"] == 3
    for bad in (dict(step=0), dict(step=np.inf), dict(tol=-1), dict(tol=np.nan), dict(max_move=-1), dict(max_move=np.inf), dict(max_iters=65), dict(max_iters=-1)):
        with pytest.raises(P.ProjectError) as e:
            P.check_opts(**{**dict(step=1, tol=0, max_move=1, max_iters=8), **bad})
        assert e.value.code == P.BAD_ARGUMENT


def test_abi_symbols_and_struct_sizes():
    """The library exports the two entry points, the ctypes mirrors are as large as the header asserts, and the argument checks that
    need no device answer GSDF_ERR_BAD_ARGUMENT."""
    from gsdf_amd import hip
    hdr = open(os.path.join(ROOT, "include", "gsdf_hip.h")).read()
    L = hip.lib()
    for name in ("gsdf_hip_indexed_project", "gsdf_hip_indexed_read_fit"):
        assert re.search(r"\bint %s\(" % name, hdr) and hasattr(L, name) and name in hip.SYMBOLS
    assert "indexed meshes: project onto the field (no reference counterpart)" in hdr
    size = lambda t: int(re.search(r"GSDF_ABI_ASSERT\(sizeof\(%s\) == (\d+)," % t, hdr).group(1))
    assert C.sizeof(hip.ProjectOpts) == size("gsdf_project_opts") == 32
    assert C.sizeof(hip.ProjectStats) == size("gsdf_project_stats") == 120
    for f, off in (("tol", 4), ("max_move", 8), ("max_iters", 12), ("flags", 16)):
        assert getattr(hip.ProjectOpts, f).offset == off and re.search(r"offsetof\(gsdf_project_opts, %s\) == %d\b" % (f, off), hdr), f
    for f, off in (("count", 8), ("evals", 72), ("over_tol_before", 80), ("max_abs_before", 96), ("steps_max", 104), ("ms_device", 112)):
        assert getattr(hip.ProjectStats, f).offset == off and re.search(r"offsetof\(gsdf_project_stats, %s\) == %d\b" % (f, off), hdr), f
    assert hip.ProjectStats.RESULT_BYTES == hip.ProjectStats.ms_device.offset == 112 and hip.PROJECT_STATUS == P.STATUS
    for k, n in enumerate(P.STATUS):
        assert re.search(r"GSDF_PROJECT_%s = %d\b" % (n, k), hdr), n
    kh = open(os.path.join(ROOT, "gsdf_amd", "csrc", "kernels_project.h")).read()
    for k, n in enumerate(P.STATUS):
        assert re.search(r"#define PROJECT_%s %du\b" % (n, k), kh), n
    h, st = C.c_void_p(), hip.ProjectStats()

    def call(**kw):
        o = hip.ProjectOpts(**{**dict(step=1.0, tol=0.0, max_move=1.0, max_iters=8), **kw})
        rc = L.gsdf_hip_indexed_project(None, None, C.byref(o), C.byref(h), C.byref(st))
        return rc, L.gsdf_hip_last_error().decode()

    rc, msg = call()
    assert rc == -3 and "null" in msg
    for kw, word in ((dict(step=0.0), "step"), (dict(step=float("nan")), "step"), (dict(tol=-1.0), "tol"), (dict(tol=float("inf")), "tol"),
                     (dict(max_move=-0.5), "max_move"), (dict(max_move=float("nan")), "max_move"), (dict(max_iters=65), "max_iters"),
                     (dict(max_iters=-1), "max_iters"), (dict(flags=2), "flags")):
        rc, msg = call(**kw)
        assert rc == -3 and word in msg, (kw, msg)
    assert L.gsdf_hip_indexed_project(None, None, None, None, None) == -3 and not h.value
    assert L.gsdf_hip_indexed_read_fit(None, None, None, None) == -3
