"""The numpy twin of the dual-contouring indexed-mesh contract (tests/dcref.py) held to the oracle's dual contouring
(oracle/orc_render.c: orc_render_dualcontour) on the shapes the GPU test uses. No GPU."""
import numpy as np
import pytest

import dcref as D
import toporef as T
from oracle.oracle import OracleSDF
from scaffold.builder import Builder

F = np.float32
NAMES = [c[0] for c in D.cases(Builder())]
_twin = {}


def twin(name, chiseled=False):
    if (name, chiseled) not in _twin:
        _, shape, res = next(c for c in D.cases(Builder()) if c[0] == name)
        _twin[(name, chiseled)] = D.mesh(OracleSDF(shape.tree()), F(res), chiseled)
    return _twin[(name, chiseled)]


@pytest.mark.parametrize("name", NAMES)
def test_twin_against_oracle(name):
    v, i, k, soup, q, ref = twin(name)
    keys = D.slot_keys(q)
    assert D.lattice_of(OracleSDF(next(c for c in D.cases(Builder()) if c[0] == name)[1].tree()).Bounds(), q["res"])[1] == ref.levels == q["levels"] <= 10
    assert len(keys) == 3 * ref.n_tris > 0 and len(q["coords"]) * 2 == ref.n_tris
    # slots with one key: one position in the oracle's soup, bit for bit
    order = np.argsort(keys, kind="stable")
    ks, ps = keys[order], np.ascontiguousarray(soup[order]).view(np.uint32)
    same = ks[1:] == ks[:-1]
    assert (ps[1:][same] == ps[:-1][same]).all()
    assert (np.ascontiguousarray(v[i.reshape(-1)]).view(np.uint32) == np.ascontiguousarray(soup).view(np.uint32)).all()
    assert len(np.unique(k)) == len(k) == len(v) and (k >> np.uint64(60) == 5).all()
    # every position in its cube's clamp box origin + res (c + [-0.1, 1.1]), a few ulp of slack
    c = np.stack([k & np.uint64(0xfffff), (k >> np.uint64(20)) & np.uint64(0xfffff), (k >> np.uint64(40)) & np.uint64(0xfffff)], axis=1).astype(np.float64)
    res, o = np.float64(q["res"]), q["origin"].astype(np.float64)
    lo, hi = o + res * (c - 0.1), o + res * (c + 1.1)
    slack = 4 * np.spacing(np.maximum(np.abs(lo), np.abs(hi)).astype(F)).astype(np.float64)
    assert ((v >= lo - slack) & (v <= hi + slack)).all()
    # every quad: the EdgeNeighbors pattern of its axis around its edge's cube, forwards or reversed
    off = q["coords"] - q["cube"][:, None, :]
    pat = D.NEIGHBORS[q["axis"]]
    fwd, rev = (off == pat).all(axis=(1, 2)), (off == pat[:, ::-1, :]).all(axis=(1, 2))
    assert (fwd ^ rev).all()
    # contract order: (z, y, x, a) strictly increasing
    cu, a = q["cube"], q["axis"]
    rank = ((cu[:, 2] * (1 << 20) + cu[:, 1]) * (1 << 20) + cu[:, 0]) * 4 + a
    assert (np.diff(rank) > 0).all()
    n = 1 << (q["levels"] - 1)
    rows = np.bincount(cu[:, 2] * n + cu[:, 1])
    print(name, "levels", ref.levels, "kept", q["n_kept"], "quads", len(a), "V", len(v), "longest row", int(rows.max()))
    if name == "long-box":
        assert ref.levels == 8 and rows.max() > 64


def test_chiseled_has_the_same_quads():
    for name in ("box", "torus-hex"):
        a, b = twin(name), twin(name, True)
        assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
        assert a[0].tobytes() != b[0].tobytes()


def test_sphere_topology():
    """The unit sphere at res 1/8. One would expect a closed sphere; the twin (and so the reference) says otherwise. The lattice starts
    at bounds.min - res/2 = -1.0625 and has 2^(levels-1) = 16 cells of 1/8 per axis -- the bounds' size over res is an exact power of
    two, so make_icube adds no level -- and ends at 0.9375, short of the sphere's far side at 1: the mesh has three holes, at +x, +y
    and +z (bbox max 0.931). One shell, consistently oriented, no non-manifold edge, 72 boundary edges (three loops of 24), Euler
    characteristic 2 - 3 = -1. The long box, whose lattice has room on every side, is closed with Euler characteristic 2."""
    v, i, *_ = twin("sphere")
    rep = T.analyse(v, i)["report"]
    got = {f: int(rep[f]) for f in ("closed_oriented", "n_shells", "euler", "degenerate", "boundary_edges", "nonmanifold_edges", "misoriented_edges")}
    assert got == {"closed_oriented": 0, "n_shells": 1, "euler": -1, "degenerate": 0, "boundary_edges": 72, "nonmanifold_edges": 0, "misoriented_edges": 0}, got
    assert rep["bbox"][3:].max() < 0.9375 + 0.1 / 8 + 1e-6 and rep["bbox"][:3].min() > -1.0
    v, i, *_ = twin("long-box")
    rep = T.analyse(v, i)["report"]
    assert (rep["closed_oriented"], rep["n_shells"], rep["euler"], rep["degenerate"]) == (1, 1, 2, 0), rep
    assert abs(rep["volume"] - 2.0) < 0.1
