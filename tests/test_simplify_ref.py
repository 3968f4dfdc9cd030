"""The numpy twin of the simplify contract (tests/simplifyref.py) on meshes whose answers are worked out by hand, its invariants on
the report's hand meshes and on a random soup -- and the library's side of the ABI (no GPU here).

The flat grid. 4 x 4 unit squares are 5 x 5 vertices (x, y in 0 .. 4, z = 0), each square (x, y) cut into (v00, v10, v11) and
(v00, v11, v01). With cell = 2 a half-open cell covers two of the five coordinates, so five coordinates fall into THREE cells per
axis whatever the origin: 9 clusters, not 4 (a closed span of 4 does not fit two half-open cells of 2).
  origin 0:    x -> cell 0 0 1 1 2, means 0.5, 2.5, 4;   a face survives iff its square straddles a boundary in x and in y: squares
               (1, 1), (3, 1), (1, 3), (3, 3) -> 8 faces over all 9 clusters, 24 collapsed, largest cluster 4
  origin 0.5:  x -> cell -1 0 0 1 1, means 0, 1.5, 3.5;  squares (0, 0), (2, 0), (0, 2), (2, 2) -> 8 faces with the same index
               pattern over 9 other positions
Four clusters come from 4 x 4 VERTICES (3 x 3 squares, coordinates 0 .. 3) at origin 0: x -> 0 0 1 1, the one surviving square is
(1, 1): 2 faces, 4 vertices at (0.5 | 2.5, 0.5 | 2.5)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import simplifyref as S
import toporef as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 1 << 19


def grid(n):
    """n x n unit squares in z = 0: ((n + 1)^2 vertices, 2 n^2 faces), squares in rows of increasing y."""
    v = np.array([[x, y, 0] for y in range(n + 1) for x in range(n + 1)], np.float32)
    at = lambda x, y: y * (n + 1) + x
    f = []
    for y in range(n):
        for x in range(n):
            f += [(at(x, y), at(x + 1, y), at(x + 1, y + 1)), (at(x, y), at(x + 1, y + 1), at(x, y + 1))]
    return v, np.array(f, np.uint32)


def key(cx, cy, cz):
    return (cx + B) | (cy + B) << 20 | (cz + B) << 40 | 4 << 60


FACES_9 = [(0, 1, 2), (0, 2, 3), (1, 4, 5), (1, 5, 2), (3, 2, 6), (3, 6, 7), (2, 5, 8), (2, 8, 6)]
ORDER_9 = [(0, 0), (1, 0), (1, 1), (0, 1), (2, 0), (2, 1), (1, 2), (0, 2), (2, 2)]   # (cell x, cell y) rank of vertex 0 .. 8


def test_flat_grid_origin_0():
    v, i = grid(4)
    v2, i2, k2, st = S.simplify(v, i, 2.0, (0, 0, 0))
    mean = [0.5, 2.5, 4.0]
    assert v2.dtype == np.float32 and i2.dtype == np.uint32 and k2.dtype == np.uint64
    assert v2.tolist() == [[mean[a], mean[b], 0.0] for a, b in ORDER_9]
    assert i2.tolist() == [list(f) for f in FACES_9]
    assert k2.tolist() == [key(a, b, 0) for a, b in ORDER_9]
    assert st == {"n_verts_in": 25, "n_tris_in": 32, "used_verts_in": 25, "degenerate_in": 0, "cells": 9, "collapsed": 24, "n_verts": 9, "n_tris": 8,
                  "largest_cell": 4, "exponent": 3}
    assert len(S.stats_bytes(st)) == 80
    # a degenerate face and a vertex nothing names (non-finite: it is ignored, and so is it by the exponent) change the counts alone
    va = np.vstack([v, [[np.nan, 100, 100]]]).astype(np.float32)
    ia = np.vstack([[[0, 0, 1]], i, [[7, 25, 7]]]).astype(np.uint32)
    v3, i3, k3, st3 = S.simplify(va, ia, 2.0, (0, 0, 0))
    assert v3.tolist() == v2.tolist() and (i3 == i2).all() and (k3 == k2).all()
    assert (st3["n_verts_in"], st3["n_tris_in"], st3["used_verts_in"], st3["degenerate_in"], st3["exponent"]) == (26, 34, 25, 2, 7)
    assert {k: st3[k] for k in ("cells", "collapsed", "n_verts", "n_tris", "largest_cell")} == {k: st[k] for k in ("cells", "collapsed", "n_verts", "n_tris", "largest_cell")}


def test_flat_grid_origin_half():
    v, i = grid(4)
    v2, i2, k2, st = S.simplify(v, i, 2.0, (0.5, 0.5, 0.5))
    mean = [0.0, 1.5, 3.5]
    assert v2.tolist() == [[mean[a], mean[b], 0.0] for a, b in ORDER_9]
    assert i2.tolist() == [list(f) for f in FACES_9]
    assert k2.tolist() == [key(a - 1, b - 1, -1) for a, b in ORDER_9]
    assert (st["cells"], st["collapsed"], st["n_verts"], st["n_tris"], st["largest_cell"]) == (9, 24, 9, 8, 4)
    # the means through Python integers: the members of cluster (0 | 1, 1) are x in {1, 2} | {3, 4}, y in {1, 2}
    assert S.mean_of([[1, 1, 0], [2, 1, 0], [1, 2, 0], [2, 2, 0]], 3).tolist() == [1.5, 1.5, 0.0] == v2[2].tolist()
    assert S.mean_of([[3, 1, 0], [4, 1, 0], [3, 2, 0], [4, 2, 0]], 3).tolist() == [3.5, 1.5, 0.0] == v2[5].tolist()


def test_four_clusters():
    v, i = grid(3)
    v2, i2, k2, st = S.simplify(v, i, 2.0, (0, 0, 0))
    assert v2.tolist() == [[0.5, 0.5, 0], [2.5, 0.5, 0], [2.5, 2.5, 0], [0.5, 2.5, 0]] and i2.tolist() == [[0, 1, 2], [0, 2, 3]]
    assert k2.tolist() == [key(0, 0, 0), key(1, 0, 0), key(1, 1, 0), key(0, 1, 0)]
    assert st == {"n_verts_in": 16, "n_tris_in": 18, "used_verts_in": 16, "degenerate_in": 0, "cells": 4, "collapsed": 16, "n_verts": 4, "n_tris": 2,
                  "largest_cell": 4, "exponent": 2}


def test_means_round_once():
    """Three members whose mean is no float32: (1 + 1 + 2) / 3 = 4/3 -> the float32 next to it; a singleton keeps its bits (-0.0 here)."""
    v = np.array([[1, 0, 0], [1, 0.5, 0], [2, 0.25, 0], [10, -0.0, 0], [10, 10, 10.5], [20, 30, 30]], np.float32)
    i = np.array([[0, 3, 4], [1, 3, 5], [2, 4, 5]], np.uint32)
    v2, i2, _, st = S.simplify(v, i, 4.0)
    assert st["exponent"] == 5 and st["cells"] == 4 and st["largest_cell"] == 3 and st["collapsed"] == 0
    assert v2[0].tolist() == [float(np.float32(4 / 3)), 0.25, 0.0] and (v2[0] == S.mean_of(v[:3], 5)).all()
    assert v2[1].view(np.uint32).tolist() == v[3].view(np.uint32).tolist() and np.signbit(v2[1, 1])
    assert i2.tolist() == [[0, 1, 2], [0, 1, 3], [0, 2, 3]]


def test_nothing_kept_and_errors():
    with pytest.raises(S.SimplifyError) as e:
        S.simplify(T.TET_V, T.TET_I, 8.0, (-1, -1, -1))
    assert e.value.code == S.EMPTY_BUFFERS
    _, _, _, st = S.simplify(T.TET_V, T.TET_I, 8.0, (-1, -1, -1), dry=True)
    assert (st["cells"], st["collapsed"], st["n_verts"], st["n_tris"], st["largest_cell"], st["used_verts_in"]) == (1, 4, 0, 0, 4, 4)
    v, i = T.hand_meshes()["tet-nan"]
    with pytest.raises(S.SimplifyError) as e:
        S.simplify(v, i, 1.0)
    assert e.value.code == S.BAD_ARGUMENT and e.value.msg.startswith("1 used")
    with pytest.raises(S.SimplifyError) as e:
        S.simplify(T.TET_V, T.TET_I, 6.0 / (1 << 19))          # vertex 1: c_x = 2^19
    assert e.value.code == S.RESOLUTION and "vertex 1 " in e.value.msg
    S.simplify(T.TET_V, T.TET_I, np.float32(6.0 / (1 << 19)) * np.float32(1.0001))
    for cell in (0.0, -1.0, np.inf, np.nan):
        with pytest.raises(S.SimplifyError) as e:
            S.simplify(T.TET_V, T.TET_I, cell)
        assert e.value.code == S.BAD_ARGUMENT


def soup(seed=5, n_verts=200, n_tris=400):
    rng = np.random.default_rng(seed)
    v = rng.uniform(-3, 5, (n_verts, 3)).astype(np.float32)
    i = rng.integers(0, n_verts, (n_tris, 3)).astype(np.uint32)
    i[::37, 1] = i[::37, 0]
    return v, i


def check_invariants(v, i, cell, origin):
    v2, i2, k2, st = S.simplify(v, i, cell, origin)
    assert st["n_tris"] + st["collapsed"] + st["degenerate_in"] == st["n_tris_in"] == len(i)
    assert (len(v2), len(i2)) == (st["n_verts"], st["n_tris"]) and st["n_verts"] <= st["cells"] <= st["used_verts_in"] <= st["n_verts_in"]
    flat = i2.reshape(-1).astype(np.int64)
    uniq, first = np.unique(flat, return_index=True)
    assert (uniq == np.arange(len(v2))).all() and (np.diff(first) > 0).all()          # numbered by first appearance
    assert not ((i2[:, 0] == i2[:, 1]) | (i2[:, 1] == i2[:, 2]) | (i2[:, 0] == i2[:, 2])).any()
    assert len(np.unique(k2)) == len(k2) and (k2 >> np.uint64(60) == 4).all()
    # every vertex lies in the cell its key names
    c = np.stack([((k2 >> np.uint64(20 * a)) & np.uint64((1 << 20) - 1)).astype(np.int64) - B for a in range(3)], axis=1)
    lo = np.asarray(origin, np.float32).astype(np.float64) + c * float(np.float32(cell))
    assert (v2 >= lo - 1e-6 * abs(lo)).all() and (v2 <= lo + float(np.float32(cell)) * (1 + 1e-6)).all()
    _, _, _, dry = S.simplify(v, i, cell, origin, dry=True)
    assert dry == st
    return st


def test_invariants_hand_meshes():
    for name, (v, i) in T.hand_meshes().items():
        if name == "tet-nan":
            continue
        for cell, origin in ((3.0, (0, 0, 0)), (5.0, (-0.5, 0.25, 1))):
            check_invariants(v, i, cell, origin)


def test_invariants_random_soup():
    v, i = soup()
    assert len(v) == 200 and len(i) == 400
    st = check_invariants(v, i, 2.0, (0, 0, 0))                                          # 0.25 of the extent 8
    assert st["degenerate_in"] > 0 and st["collapsed"] > 0 and 1 < st["largest_cell"] and st["cells"] < st["used_verts_in"]
    check_invariants(v, i, 2.0, (-3, -3, -3))


def test_abi_symbol_and_struct_sizes():
    """The library exports gsdf_hip_indexed_simplify, the ctypes mirrors are as large as the header asserts, and the argument checks
    that need no device answer GSDF_ERR_BAD_ARGUMENT."""
    from gsdf_amd import hip
    hdr = open(os.path.join(ROOT, "include", "gsdf_hip.h")).read()
    L = hip.lib()
    name = "gsdf_hip_indexed_simplify"
    assert re.search(r"\bint %s\(" % name, hdr) and "indexed meshes: simplify" in hdr
    assert hasattr(L, name) and name in hip.SYMBOLS
    size = lambda t: int(re.search(r"GSDF_ABI_ASSERT\(sizeof\(%s\) == (\d+)," % t, hdr).group(1))
    assert C.sizeof(hip.SimplifyOpts) == size("gsdf_simplify_opts") == 32
    assert C.sizeof(hip.SimplifyStats) == size("gsdf_simplify_stats") == 120
    for f, off in (("cells", 32), ("n_verts", 48), ("exponent", 72), ("ms_cells", 80)):
        assert getattr(hip.SimplifyStats, f).offset == off and re.search(r"offsetof\(gsdf_simplify_stats, %s\) == %d\b" % (f, off), hdr), f
    for f, off in (("origin", 4), ("flags", 16)):
        assert getattr(hip.SimplifyOpts, f).offset == off and re.search(r"offsetof\(gsdf_simplify_opts, %s\) == %d\b" % (f, off), hdr), f
    assert hip.SimplifyStats.RESULT_BYTES == hip.SimplifyStats.ms_cells.offset == len(S.stats_bytes(dict.fromkeys(S.STAT_FIELDS + ["exponent"], 0)))
    assert [f for f, _ in hip.SimplifyStats._fields_[:9]] == S.STAT_FIELDS
    h, st = C.c_void_p(), hip.SimplifyStats()

    def call(ix, **kw):
        o = hip.SimplifyOpts(cell=kw.get("cell", 1.0), flags=kw.get("flags", 0))
        rc = L.gsdf_hip_indexed_simplify(ix, C.byref(o), C.byref(h), C.byref(st))
        return rc, L.gsdf_hip_last_error().decode()

    rc, msg = call(None)
    assert rc == -3 and "null" in msg                                                     # NULL handle
    for cell in (0.0, -2.0, float("inf"), float("nan")):
        rc, msg = call(None, cell=cell)
        assert rc == -3 and "cell" in msg, (cell, msg)
    rc, msg = call(None, flags=1)
    assert rc == -3 and "flags" in msg
    assert L.gsdf_hip_indexed_simplify(None, None, None, None) == -3 and not h.value
