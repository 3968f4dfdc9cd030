"""The numpy twin of the adaptive-simplify contract (tests/adaptiveref.py): against the uniform simplifier's twin where the two must
agree, its own invariants (the partition, monotonicity in tol and levels, independence of order, the error bound recomputed by a
plain loop), a dyadic cube whose answers are exact by construction -- and the library's side of the ABI (no GPU here).

The dyadic cube. The surface of [-2, 2]^3, 16 x 16 quads of edge 1/4 per side, cell = 1/4, the grid half a spacing below the lattice:
vertex j of an axis (x = -2 + j / 4) has level-0 cell j, so a level-l cell holds 2^l consecutive j, aligned, and j = 16 (the far
sides) is alone in its cells. Inside one side every face's normal has one non-zero component and the cell's mean has that
coordinate equal to the side's, exactly (n times the same integer, divided by n), so t is exactly 0; a cell that holds an edge
vertex sees a face of the other side, off whose plane the mean lies by a dyadic amount > 0. With tol = 0 the choice is therefore
decided by exact arithmetic."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import adaptiveref as A
import simplifyref as S
import toporef as T
import weldref as W
from corpus import shapes3d
from oracle.oracle import OracleSDF

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
HUGE = 3e38
_made = {}


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def welded(name="torus", resdiv=48):
    """(verts, idx, keys, res, grid origin: half a res below the lattice origin) of a SMALL shape welded by weldref, made once."""
    if name not in _made:
        shape = dict(shapes3d()[1])[name]
        cpu = OracleSDF(shape.tree())
        res = F32(float(shape.Diagonal()) / resdiv)
        origin, _ = W.lattice_of(shape.Bounds(), res)
        v, i, k, _ = W.weld(cpu, W.leaves_of_triangles(cpu.render_octree(res).tris, origin, res), origin, res)
        _made[name] = (v, i, k, res, tuple(F32(o) - F32(0.5) * res for o in origin))
    return _made[name]


def hand():
    return {n: m for n, m in T.hand_meshes().items() if n != "tet-nan"}


def decode(k):
    """(kind, level, cell (n, 3)) of adaptive keys."""
    k = np.asarray(k, np.uint64)
    c = np.stack([((k >> np.uint64(18 * a)) & np.uint64((1 << 18) - 1)).astype(np.int64) - A.BIAS for a in range(3)], axis=1)
    return (k >> np.uint64(60)).astype(np.int64), ((k >> np.uint64(54)) & np.uint64(63)).astype(np.int64), c


def same_as_uniform(v, i, cell, origin, keys=None):
    v2, i2, k2, st = A.simplify(v, i, cell, HUGE, 1, origin, keys)
    sv, si, sk, ss = S.simplify(v, i, cell, origin)
    assert v2.shape == sv.shape and (u32(v2) == u32(sv)).all() and i2.tobytes() == si.tobytes()
    for f in ("n_verts_in", "n_tris_in", "used_verts_in", "degenerate_in", "cells", "collapsed", "n_verts", "n_tris", "exponent"):
        assert st[f] == ss[f], f
    assert st["largest_cluster"] == ss["largest_cell"] and sum(st["chosen"]) + st["singles"] == ss["cells"] and st["chosen"][1:] == [0] * 15
    # keys: a cluster's differs from the uniform one's in kind and layout alone; a vertex that stays alone keeps its input key
    kind, level, c = decode(k2)
    sc = np.stack([((sk >> np.uint64(20 * a)) & np.uint64((1 << 20) - 1)).astype(np.int64) - S.BIAS for a in range(3)], axis=1)
    many = kind == A.KIND if keys is None else ~np.isin(k2, np.asarray(keys, np.uint64))
    assert (c[many] == sc[many]).all() and (level[many] == 0).all() and (kind[many] == A.KIND).all()
    assert many.sum() + (~many).sum() == len(k2) == st["n_verts"]
    return st


def test_one_level_and_a_huge_tol_is_the_uniform_simplifier():
    for name, (v, i) in hand().items():
        for cell, origin in ((3.0, (0, 0, 0)), (5.0, (-0.5, 0.25, 1)), (7.0, (0, 0, 0))):
            try:
                S.simplify(v, i, cell, origin)
            except S.SimplifyError as e:
                with pytest.raises(A.AdaptiveError) as got:
                    A.simplify(v, i, cell, HUGE, 1, origin)
                assert got.value.code == e.code == A.EMPTY_BUFFERS
                continue
            same_as_uniform(v, i, cell, origin)
    v, i, k, res, grid = welded()
    st = same_as_uniform(v, i, F32(3) * res, grid, k)
    assert st["chosen"][0] > 100 and st["collapsed"] > 0 and st["max_err"] > 0


def check_partition(v, i, cell, tol, levels, origin):
    """Two vertices share a cluster iff they share the accepted ancestor both chose; returns the partition's size."""
    s = A.solve(v, i, cell, tol, levels, origin)
    used, level, single = s["used"], s["level"], s["single"]
    assert (level[~used] == -1).all() and not single[~used].any() and ((level >= 0) ^ single)[used].all()
    size = int(single.sum())
    for l in range(levels):
        at = s["cell_of"][l]
        chosen = np.unique(at[level == l])
        size += len(chosen)
        assert (s["err"][l][chosen] <= s["tol"]).all() and (s["count"][l][chosen] > 1).all()
        members = np.isin(at, chosen) & used
        assert (level[members] == l).all()                                   # the whole cell chose it: a partition
        for l2 in range(l + 1, levels):                                     # and nothing above it was accepted
            assert (s["err"][l2][s["cell_of"][l2][members]] > s["tol"]).all()
    for x in np.flatnonzero(single):
        acc = [l for l in range(levels) if s["err"][l][s["cell_of"][l][x]] <= s["tol"]]
        assert not acc or s["count"][max(acc)][s["cell_of"][max(acc)][x]] == 1
    # nesting: the level-(l+1) cell of a vertex is a function of its level-l cell
    for l in range(levels - 1):
        a, b = s["cell_of"][l][used], s["cell_of"][l + 1][used]
        assert len(np.unique(np.stack([a, b], axis=1), axis=0)) == len(np.unique(a))
        _, _, ca = decode(s["key"][l][a])
        _, lb, cb = decode(s["key"][l + 1][b])
        assert (ca >> 1 == cb).all() and (lb == l + 1).all()
    _, _, _, st = A.simplify(v, i, cell, tol, levels, origin, dry=True)
    assert size == sum(st["chosen"]) + st["singles"] and st["cells"] == sum(len(k) for k in s["key"])
    return size


def test_partition_is_nested_and_consistent():
    for name, (v, i) in hand().items():
        for tol in (0.0, 0.5, 2.0):
            check_partition(v, i, 3.0, tol, 3, (-0.5, 0.25, 1))
    v, i, _, res, grid = welded()
    assert check_partition(v, i, res, res / F32(4), 5, grid) < A.solve(v, i, res, 0, 1, grid)["used"].sum()


def test_monotone_in_tol_and_levels():
    v, i, _, res, grid = welded()
    tols = [F32(0), res / F32(16), res / F32(4), res, F32(4) * res]
    table = {}
    for levels in (1, 2, 4, 6):
        for tol in tols:
            st = A.simplify(v, i, res, tol, levels, grid, dry=True)[3]
            table[levels, float(tol)] = (st["n_tris"], sum(st["chosen"]) + st["singles"])
    for levels in (1, 2, 4, 6):
        row = [table[levels, float(t)] for t in tols]
        for a, b in zip(row, row[1:]):
            assert b[0] <= a[0] and b[1] <= a[1], (levels, row)
        assert row[-1][0] < row[0][0]
    for tol in tols:
        col = [table[l, float(tol)] for l in (1, 2, 4, 6)]
        for a, b in zip(col, col[1:]):
            assert b[0] <= a[0] and b[1] <= a[1], (float(tol), col)
    assert table[6, float(res)][0] < table[1, float(res)][0]


def keyed(v, i, k):
    rows = np.concatenate([k.astype(np.uint64)[:, None], u32(v).astype(np.uint64)], axis=1)
    faces = k[i.astype(np.int64)]
    return rows[np.lexsort(rows.T[::-1])].tobytes(), faces[np.lexsort(faces.T[::-1])].tobytes()


def test_order_independence():
    v, i, k, res, grid = welded("smoothunion")
    args = (res, res / F32(4), 4, grid)
    v2, i2, k2, st = A.simplify(v, i, *args, keys=k)
    want = keyed(v2, i2, k2)
    assert len(np.unique(k2)) == len(k2) and st["singles"] > 0 and sum(st["chosen"][1:]) > 0
    perm = np.random.default_rng(31).permutation(len(i))
    b = A.simplify(v, i[perm], *args, keys=k)
    assert keyed(*b[:3]) == want and A.stats_bytes(b[3]) == A.stats_bytes(st)
    vp = np.random.default_rng(32).permutation(len(v))
    vv, kk = np.empty_like(v), np.empty_like(k)
    vv[vp], kk[vp] = v, k
    c = A.simplify(vv, vp[i.astype(np.int64)].astype(np.uint32), *args, keys=kk)
    assert keyed(*c[:3]) == want and A.stats_bytes(c[3]) == A.stats_bytes(st)


def loop_error(v, faces, members, r):
    """max t over the (face, corner) pairs with the corner in `members`, in Python floats, one face at a time."""
    worst = 0.0
    r = [float(x) for x in r]
    for a, b, c in faces:
        if len({a, b, c}) < 3 or not ({a, b, c} & members):
            continue
        pa, pb, pc = ([float(x) for x in v[j]] for j in (a, b, c))
        u, w = [pb[k] - pa[k] for k in range(3)], [pc[k] - pa[k] for k in range(3)]
        n = [u[1] * w[2] - u[2] * w[1], u[2] * w[0] - u[0] * w[2], u[0] * w[1] - u[1] * w[0]]
        L = math.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
        if not L > 0:
            continue
        g = [r[k] - pa[k] for k in range(3)]
        t = abs((n[0] * g[0] + n[1] * g[1]) + n[2] * g[2]) / L
        worst = max(worst, t)
    return worst


@pytest.mark.parametrize("tol", [0.25, 1.0])
def test_chosen_errors_recomputed_by_a_plain_loop(tol):
    v, i = S_soup()
    levels, cell, origin = 3, 1.0, (-3, -3, -3)
    s = A.solve(v, i, cell, tol, levels, origin)
    st = A.simplify(v, i, cell, tol, levels, origin, dry=True)[3]
    faces = [tuple(int(x) for x in f) for f in i]
    worst, n = 0.0, 0
    for l in range(levels):
        for c in np.unique(s["cell_of"][l][s["level"] == l]):
            members = set(np.flatnonzero(s["cell_of"][l] == c).tolist())
            assert len(members) > 1
            pos = S.mean_of(v[sorted(members)], s["e"])
            assert (u32(pos) == u32(s["pos"][l][c])).all()
            err = loop_error(v, faces, members, pos)
            assert err <= float(F32(tol)) and err == s["err"][l][c]
            worst, n = max(worst, err), n + 1
    assert n == sum(st["chosen"]) > 3 and worst == st["max_err"] > 0


def S_soup():
    """A patch of a gently curved sheet (so that some cells are accepted and some are not), with two degenerate faces."""
    n = 13
    xs = np.linspace(-2.5, 2.5, n)
    v = np.array([[x, y, 0.08 * x * x * (1 + 0.5 * y) + 0.02 * math.sin(5 * x * y)] for y in xs for x in xs], np.float32)
    at = lambda x, y: y * n + x
    f = [t for y in range(n - 1) for x in range(n - 1) for t in ((at(x, y), at(x + 1, y), at(x + 1, y + 1)), (at(x, y), at(x + 1, y + 1), at(x, y + 1)))]
    f[5] = (f[5][0], f[5][0], f[5][2])
    f.append((7, 8, 7))
    return v, np.array(f, np.uint32)


def dyadic_cube(n=16, half=2.0):
    """The surface of [-half, half]^3, n x n quads per side, outward: lattice vertices welded by their lattice coordinates."""
    num, verts, faces = {}, [], []

    def vertex(p):
        if p not in num:
            num[p] = len(verts)
            verts.append([-half + 2 * half * c / n for c in p])
        return num[p]

    for axis in range(3):
        a, b = (axis + 1) % 3, (axis + 2) % 3
        for side in (0, n):
            for y in range(n):
                for x in range(n):
                    def p(dx, dy):
                        q = [0, 0, 0]
                        q[axis], q[a], q[b] = side, x + dx, y + dy
                        return vertex(tuple(q))
                    quad = [p(0, 0), p(1, 0), p(1, 1), p(0, 1)]          # counter-clockwise seen from +axis
                    if side == 0:
                        quad.reverse()
                    faces += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
    return np.array(verts, np.float32), np.array(faces, np.uint32)


def test_dyadic_cube():
    v, i = dyadic_cube()
    before = T.analyse(v, i)["report"]
    assert len(i) == 6 * 16 * 16 * 2 and before["closed_oriented"] == 1 and before["n_shells"] == 1
    assert abs(before["volume"] - 64.0) <= (len(i) / 2) * math.ldexp(1.0, 3 * before["exponent"] - 62)
    h = 0.25
    grid = (-2 - h / 2,) * 3
    v2, i2, k2, st = A.simplify(v, i, h, 0.0, 4, grid)
    # exact by construction: every cluster lies in one side's plane, and so does every vertex that stays alone
    assert (np.abs(v2) == 2).any(axis=1).all() and (np.abs(v2) <= 2).all()
    assert st["max_err"] == 0.0 and st["n_tris"] < len(i) and st["chosen"][3] > 0 and st["singles"] > 0
    s = A.solve(v, i, h, 0.0, 4, grid)
    for l in range(4):
        e = s["err"][l]
        assert ((e == 0) | (e >= h / 4)).all()                          # exactly 0 inside a side, a dyadic step off it at the edges
    after = T.analyse(v2, i2)["report"]
    print("dyadic cube: F", len(i), "->", st["n_tris"], "V", len(v), "->", st["n_verts"], "chosen", st["chosen"][:4], "singles", st["singles"],
          "closed", after["closed_oriented"], "shells", after["n_shells"], "volume", after["volume"], "boundary", after["boundary_edges"],
          "nonmanifold", after["nonmanifold_edges"], "misoriented", after["misoriented_edges"])
    assert after["closed_oriented"] == 1 and after["n_shells"] == 1
    # the report's contract: the volume's quantisation error is at most n_tris / 2 units of 2^(3 e - 62); on dyadic coordinates the terms
    # themselves are exact, so the two volumes differ by at most the sum of the two bounds
    margin = (len(i) / 2) * math.ldexp(1.0, 3 * before["exponent"] - 62) + (len(i2) / 2) * math.ldexp(1.0, 3 * after["exponent"] - 62)
    assert abs(after["volume"] - before["volume"]) <= margin


def test_argument_errors_of_the_twin():
    v, i = T.TET_V, T.TET_I
    for kw in (dict(cell=0.0), dict(cell=np.nan), dict(tol=-1.0), dict(tol=np.inf), dict(levels=0), dict(levels=17), dict(origin=(0, np.inf, 0))):
        with pytest.raises(A.AdaptiveError) as e:
            A.simplify(v, i, **{**dict(cell=1.0, tol=0.0, levels=2), **kw})
        assert e.value.code == A.BAD_ARGUMENT, kw
    with pytest.raises(A.AdaptiveError) as e:
        A.simplify(v, i, 6.0 / (1 << 17), 0.0, 2)                            # vertex 1: c_x = 2^17
    assert e.value.code == A.RESOLUTION and "vertex 1 " in e.value.msg
    vn, inn = T.hand_meshes()["tet-nan"]
    with pytest.raises(A.AdaptiveError) as e:
        A.simplify(vn, inn, 1.0, 0.0, 2)
    assert e.value.code == A.BAD_ARGUMENT and e.value.msg.startswith("1 used")
    with pytest.raises(A.AdaptiveError) as e:
        A.simplify(v, i, 8.0, 100.0, 1, (-1, -1, -1))
    assert e.value.code == A.EMPTY_BUFFERS
    st = A.simplify(v, i, 8.0, 100.0, 1, (-1, -1, -1), dry=True)[3]
    assert (st["n_tris"], st["n_verts"], st["cells"], st["collapsed"], st["largest_cluster"], st["chosen"][0], st["singles"]) == (0, 0, 1, 4, 4, 1, 0)
    assert len(A.stats_bytes(st)) == 224


def test_abi_symbol_and_struct_sizes():
    """The library exports gsdf_hip_indexed_simplify_adaptive, the ctypes mirrors are as large as the header asserts, and the argument
    checks that need no device answer GSDF_ERR_BAD_ARGUMENT."""
    from gsdf_amd import hip
    hdr = open(os.path.join(ROOT, "include", "gsdf_hip.h")).read()
    L = hip.lib()
    name = "gsdf_hip_indexed_simplify_adaptive"
    assert re.search(r"\bint %s\(" % name, hdr) and "indexed meshes: adaptive simplify" in hdr
    assert "Raising tol or levels\n *   only coarsens the partition" in hdr
    assert hasattr(L, name) and name in hip.SYMBOLS
    size = lambda t: int(re.search(r"GSDF_ABI_ASSERT\(sizeof\(%s\) == (\d+)," % t, hdr).group(1))
    assert C.sizeof(hip.AdaptiveOpts) == size("gsdf_adaptive_opts") == 32
    assert C.sizeof(hip.AdaptiveStats) == size("gsdf_adaptive_stats") == 272
    for f, off in (("cells", 32), ("chosen", 40), ("singles", 168), ("n_verts", 184), ("max_err", 208), ("exponent", 216), ("ms_cells", 224)):
        assert getattr(hip.AdaptiveStats, f).offset == off and re.search(r"offsetof\(gsdf_adaptive_stats, %s\) == %d\b" % (f, off), hdr), f
    for f, off in (("origin", 4), ("tol", 16), ("levels", 20), ("flags", 24)):
        assert getattr(hip.AdaptiveOpts, f).offset == off and re.search(r"offsetof\(gsdf_adaptive_opts, %s\) == %d\b" % (f, off), hdr), f
    zero = dict.fromkeys(A.STAT_FIELDS, 0)
    zero["chosen"] = [0] * 16
    assert hip.AdaptiveStats.RESULT_BYTES == hip.AdaptiveStats.ms_cells.offset == len(A.stats_bytes(zero)) == 224
    assert [f for f, _ in hip.AdaptiveStats._fields_[:13]] == A.STAT_FIELDS
    kh = open(os.path.join(ROOT, "gsdf_amd", "csrc", "kernels_simplify_adaptive.h")).read()
    assert re.search(r"#define ADAPTIVE_KIND %dull\b" % A.KIND, kh) and re.search(r"#define ADAPTIVE_BIAS %d\.0\b" % A.BIAS, kh)
    h, st = C.c_void_p(), hip.AdaptiveStats()

    def call(**kw):
        o = hip.AdaptiveOpts(**{**dict(cell=1.0, tol=0.0, levels=4), **kw})
        rc = L.gsdf_hip_indexed_simplify_adaptive(None, C.byref(o), C.byref(h), C.byref(st))
        return rc, L.gsdf_hip_last_error().decode()

    rc, msg = call()
    assert rc == -3 and "null" in msg                                                     # NULL handle
    for kw, word in ((dict(cell=0.0), "cell"), (dict(cell=-2.0), "cell"), (dict(cell=float("inf")), "cell"), (dict(cell=float("nan")), "cell"),
                     (dict(origin=(C.c_float * 3)(0, float("nan"), 0)), "origin"), (dict(tol=-1.0), "tol"), (dict(tol=float("inf")), "tol"),
                     (dict(tol=float("nan")), "tol"), (dict(levels=0), "levels"), (dict(levels=17), "levels"), (dict(flags=1), "flags")):
        rc, msg = call(**kw)
        assert rc == -3 and word in msg, (kw, msg)
    assert L.gsdf_hip_indexed_simplify_adaptive(None, None, None, None) == -3 and not h.value
