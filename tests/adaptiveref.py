"""A numpy twin of the indexed-mesh ADAPTIVE SIMPLIFY contract (include/gsdf_hip.h, "indexed meshes: adaptive simplify"):
(verts, idx, input keys) and the options in; the clustered mesh, its vertices' keys and the stats' leading block out. Written from
the header; nothing here looks at a device result.

Per level the cells by np.unique over the keys, their integer sums in int64, the means as simplifyref does (float64(S) / float64(n),
a power of two, one rounding to float32); the error terms with numpy's float64 operations in the contract's association (separate
ufunc calls: nothing is contracted) and np.maximum.at; the choice from the top level down. solve() returns everything the tests ask
about (levels, clusters, errors); simplify() the mesh, as simplifyref.simplify does."""
import math
import struct

import numpy as np

import simplifyref as S
import toporef as T

BIAS = 1 << 17
KIND = 6
MAX_LEVELS = 16
# the leading block of gsdf_adaptive_stats, in its order (224 bytes)
STAT_FIELDS = ["n_verts_in", "n_tris_in", "used_verts_in", "degenerate_in", "cells", "chosen", "singles", "collapsed", "n_verts", "n_tris",
               "largest_cluster", "max_err", "exponent"]
AdaptiveError = S.SimplifyError
BAD_ARGUMENT, RESOLUTION, EMPTY_BUFFERS = S.BAD_ARGUMENT, S.RESOLUTION, S.EMPTY_BUFFERS


def stats_bytes(st):
    return struct.pack("<5Q16Q5Qdii", *[int(st[f]) for f in STAT_FIELDS[:5]], *[int(x) for x in st["chosen"]],
                       *[int(st[f]) for f in ("singles", "collapsed", "n_verts", "n_tris", "largest_cluster")], float(st["max_err"]), int(st["exponent"]), 0)


def cell_key(c, level):
    """The key of the level-`level` cells of the level-0 cells c (n, 3) int64."""
    b = (c >> np.int64(level)) + BIAS
    return (b[:, 0] | (b[:, 1] << 18) | (b[:, 2] << 36)).astype(np.uint64) | np.uint64(level << 54) | np.uint64(KIND << 60)


def plane_terms(v, nd, r):
    """t of the contract for the non-degenerate faces nd (n, 3) over float32 vertices v, measured from the float32 points r (n, 3);
    (t, has_plane)."""
    pa, pb, pc = (v[nd[:, k]].astype(np.float64) for k in range(3))
    with np.errstate(all="ignore"):
        u, w = pb - pa, pc - pa
        n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2], u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
        L = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        g = r.astype(np.float64) - pa
        t = np.abs((n[:, 0] * g[:, 0] + n[:, 1] * g[:, 1]) + n[:, 2] * g[:, 2]) / L
    return t, L > 0


def solve(verts, idx, cell, tol, levels=8, origin=(0, 0, 0)):
    """The contract up to the choice. A dict: used (V,), nd, n_deg, e, tol (float64), per level l the arrays key[l] (cells,),
    count[l], pos[l] (cells, 3) float32, err[l] (cells,) float64, label[l], cell_of[l] (V,) (index into the level's arrays, -1 unused);
    level (V,) the chosen level or -1 (SINGLE or unused), single (V,) bool."""
    cell, tol = np.float32(cell), np.float32(tol)
    org = np.asarray(origin, np.float32).reshape(3)
    if not (cell > 0 and np.isfinite(cell)) or not np.isfinite(org).all():
        raise AdaptiveError(BAD_ARGUMENT, "cell and origin must be finite, cell > 0")
    if not (tol >= 0 and np.isfinite(tol)):
        raise AdaptiveError(BAD_ARGUMENT, "tol must be finite and not negative")
    if int(levels) != levels or not 1 <= levels <= MAX_LEVELS:
        raise AdaptiveError(BAD_ARGUMENT, "levels must be 1 .. 16")
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    i = np.asarray(idx).astype(np.int64).reshape(-1, 3)
    deg = (i[:, 0] == i[:, 1]) | (i[:, 1] == i[:, 2]) | (i[:, 0] == i[:, 2])
    nd = i[~deg]
    used = np.zeros(len(v), bool)
    used[nd.reshape(-1)] = True
    bad = used & ~np.isfinite(v).all(axis=1)
    if bad.any():
        raise AdaptiveError(BAD_ARGUMENT, "%d used vertices have a NaN or infinite coordinate" % int(bad.sum()))
    with np.errstate(all="ignore"):
        c = np.floor((v.astype(np.float64) - org.astype(np.float64)) / np.float64(cell))
    far = used & ~(np.abs(c) < BIAS).all(axis=1)
    if far.any():
        raise AdaptiveError(RESOLUTION, "vertex %d lies 2^17 cells or more from the origin" % int(np.flatnonzero(far)[0]))
    uv = np.flatnonzero(used)
    c0 = c[uv].astype(np.int64)
    e = T.exponent_of(v)
    q = np.rint(v[uv].astype(np.float64) * math.ldexp(1.0, 30 - e)).astype(np.int64)
    tol64 = np.float64(tol)
    out = {"used": used, "nd": nd, "n_deg": int(deg.sum()), "e": e, "tol": tol64, "levels": int(levels), "key": [], "count": [], "pos": [], "err": [],
           "label": [], "cell_of": []}
    for l in range(int(levels)):
        ukeys, inv, counts = np.unique(cell_key(c0, l), return_inverse=True, return_counts=True)
        inv = inv.reshape(-1)
        Ssum = np.zeros((len(ukeys), 3), np.int64)
        np.add.at(Ssum, inv, q)
        label = np.full(len(ukeys), len(v), np.int64)
        np.minimum.at(label, inv, uv)
        pos = np.empty((len(ukeys), 3), np.float32)
        one = counts == 1
        pos[one] = v[label[one]]
        many = ~one
        pos[many] = ((Ssum[many].astype(np.float64) / counts[many].astype(np.float64)[:, None]) * np.float64(math.ldexp(1.0, e - 30))).astype(np.float32)
        cell_of = np.full(len(v), -1, np.int64)
        cell_of[uv] = inv
        err = np.zeros(len(ukeys), np.float64)
        for corner in range(3):
            at = cell_of[nd[:, corner]]
            t, ok = plane_terms(v, nd, pos[at])
            np.maximum.at(err, at[ok], t[ok])
        for name, a in (("key", ukeys), ("count", counts), ("pos", pos), ("err", err), ("label", label), ("cell_of", cell_of)):
            out[name].append(a)
    level = np.full(len(v), -1, np.int64)
    for l in range(int(levels) - 1, -1, -1):
        acc = np.zeros(len(v), bool)
        acc[uv] = out["err"][l][out["cell_of"][l][uv]] <= tol64
        level[(level < 0) & acc] = l
    single = used.copy()
    for l in range(int(levels)):
        m = level == l
        big = out["count"][l][out["cell_of"][l][m]] > 1
        single[np.flatnonzero(m)[big]] = False
    level[single] = -1
    out["level"], out["single"] = level, single
    return out


def simplify(verts, idx, cell, tol, levels=8, origin=(0, 0, 0), keys=None, dry=False):
    """(verts (V2, 3) float32, idx (F2, 3) uint32, keys (V2,) uint64, stats dict). keys: the input's (zeros if None), which the SINGLE
    vertices keep. dry: (None, None, None, stats), and no error where nothing is kept."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    F = len(np.asarray(idx).reshape(-1, 3))
    kin = np.zeros(len(v), np.uint64) if keys is None else np.asarray(keys, np.uint64)
    s = solve(v, idx, cell, tol, levels, origin)
    L = s["levels"]
    base = np.concatenate([[0], np.cumsum([len(k) for k in s["key"]])]).astype(np.int64)
    n_cells = int(base[-1])
    # cluster numbers: the chosen cell (all levels in one range), or n_cells + v for a vertex that stays alone
    cid = np.full(len(v), -1, np.int64)
    cid[s["single"]] = n_cells + np.flatnonzero(s["single"])
    chosen, largest, max_err = [0] * MAX_LEVELS, (1 if s["single"].any() else 0), 0.0
    for l in range(L):
        m = s["level"] == l
        at = s["cell_of"][l][m]
        cid[m] = base[l] + at
        cl = np.unique(at)
        chosen[l] = len(cl)
        if len(cl):
            largest = max(largest, int(s["count"][l][cl].max()))
            max_err = max(max_err, float(s["err"][l][cl].max()))
    pos = np.concatenate(s["pos"] + [v])
    key = np.concatenate(s["key"] + [kin])
    fc = cid[s["nd"]]
    collapsed = (fc[:, 0] == fc[:, 1]) | (fc[:, 1] == fc[:, 2]) | (fc[:, 0] == fc[:, 2])
    kept = fc[~collapsed]
    uniq, first, finv = np.unique(kept.reshape(-1), return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    number = np.empty(len(uniq), np.int64)
    number[order] = np.arange(len(uniq))
    old = uniq[order]
    st = {"n_verts_in": len(v), "n_tris_in": F, "used_verts_in": int(s["used"].sum()), "degenerate_in": s["n_deg"], "cells": n_cells, "chosen": chosen,
          "singles": int(s["single"].sum()), "collapsed": int(collapsed.sum()), "n_verts": len(uniq), "n_tris": len(kept), "largest_cluster": largest,
          "max_err": max_err, "exponent": s["e"]}
    if dry:
        return None, None, None, st
    if len(kept) == 0:
        raise AdaptiveError(EMPTY_BUFFERS, "nothing kept")
    return pos[old].copy(), number[finv.reshape(-1)].reshape(-1, 3).astype(np.uint32), key[old].copy(), st
