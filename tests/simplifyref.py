"""A numpy + Python-integer twin of the indexed-mesh SIMPLIFY contract (include/gsdf_hip.h, "indexed meshes: simplify"):
(verts, idx, cell, origin) in; the clustered mesh, its vertices' keys and the stats' leading block out. Nothing here looks at a device
result.

Cells by two float64 operations and a floor per coordinate (numpy's float64 subtraction and division are IEEE operations); clusters
by np.unique over the keys; the sums of the quantised coordinates in int64 (|q| <= 2^30 and fewer than 2^32 members: no overflow),
the mean as float64(S) / float64(n), scaled by a power of two and rounded to float32 once; mean_of() restates that for one cluster
with Python integers (float() of a Python int is correctly rounded), for the hand-checked tests."""
import math
import struct

import numpy as np

import toporef as T

BIAS = 1 << 19
KIND = 4
# the leading block of gsdf_simplify_stats, in its order: nine uint64, then int32 exponent, int32 reserved (80 bytes)
STAT_FIELDS = ["n_verts_in", "n_tris_in", "used_verts_in", "degenerate_in", "cells", "collapsed", "n_verts", "n_tris", "largest_cell"]


class SimplifyError(Exception):
    """code: the GSDF_ERR_* the device returns for the same input."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code
        self.msg = msg


BAD_ARGUMENT, RESOLUTION, EMPTY_BUFFERS = -3, -8, -1


def stats_bytes(st):
    return struct.pack("<9Qii", *[int(st[f]) for f in STAT_FIELDS], int(st["exponent"]), 0)


def mean_of(points, e):
    """The contract's position of a cluster of more than one member, one coordinate at a time, through Python integers."""
    p = np.asarray(points, np.float32).reshape(-1, 3)
    out = np.empty(3, np.float32)
    for k in range(3):
        s = sum(int(np.rint(np.float64(x) * math.ldexp(1.0, 30 - e))) for x in p[:, k])
        out[k] = np.float32((float(s) / float(len(p))) * math.ldexp(1.0, e - 30))
    return out


def cluster(verts, idx, cell, origin=(0, 0, 0)):
    """The clustering half of the contract: (used (V,) bool, key (V,) uint64 with 0 for unused vertices, nondegenerate faces (n, 3) int64,
    number of degenerate faces). Raises the contract's errors."""
    cell = np.float32(cell)
    org = np.asarray(origin, np.float32).reshape(3)
    if not (cell > 0 and np.isfinite(cell)) or not np.isfinite(org).all():
        raise SimplifyError(BAD_ARGUMENT, "cell and origin must be finite, cell > 0")
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    i = np.asarray(idx).astype(np.int64).reshape(-1, 3)
    deg = (i[:, 0] == i[:, 1]) | (i[:, 1] == i[:, 2]) | (i[:, 0] == i[:, 2])
    nd = i[~deg]
    used = np.zeros(len(v), bool)
    used[nd.reshape(-1)] = True
    bad = used & ~np.isfinite(v).all(axis=1)
    if bad.any():
        raise SimplifyError(BAD_ARGUMENT, "%d used vertices have a NaN or infinite coordinate" % int(bad.sum()))
    with np.errstate(all="ignore"):
        c = np.floor((v.astype(np.float64) - org.astype(np.float64)) / np.float64(cell))
    far = used & ~(np.abs(c) < BIAS).all(axis=1)
    if far.any():
        raise SimplifyError(RESOLUTION, "vertex %d lies 2^19 cells or more from the origin" % int(np.flatnonzero(far)[0]))
    ci = np.where(used[:, None], c, 0).astype(np.int64) + BIAS
    key = (ci[:, 0] | (ci[:, 1] << 20) | (ci[:, 2] << 40)).astype(np.uint64) | (np.uint64(KIND) << np.uint64(60))
    return used, np.where(used, key, np.uint64(0)), nd, int(deg.sum())


def simplify(verts, idx, cell, origin=(0, 0, 0), dry=False):
    """(verts (V2, 3) float32, idx (F2, 3) uint32, keys (V2,) uint64, stats dict). dry: (None, None, None, stats), and no error where
    nothing is kept."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    used, key, nd, n_deg = cluster(v, idx, cell, origin)
    F = len(np.asarray(idx).reshape(-1, 3))
    uv = np.flatnonzero(used)
    ukeys, inv, counts = np.unique(key[uv], return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    cl = np.full(len(v), -1, np.int64)
    cl[uv] = inv                                    # cluster (index into ukeys) of every used vertex
    e = T.exponent_of(v)
    # positions of all clusters
    q = np.rint(v[uv].astype(np.float64) * math.ldexp(1.0, 30 - e)).astype(np.int64)
    S = np.zeros((len(ukeys), 3), np.int64)
    np.add.at(S, inv, q)
    pos = np.empty((len(ukeys), 3), np.float32)
    single = counts == 1
    label = np.full(len(ukeys), len(v), np.int64)
    np.minimum.at(label, inv, uv)
    pos[single] = v[label[single]]
    many = ~single
    # int64 -> float64 and float64 -> float32 conversions round to nearest, ties to even (mean_of() says the same with Python integers)
    pos[many] = ((S[many].astype(np.float64) / counts[many].astype(np.float64)[:, None]) * np.float64(math.ldexp(1.0, e - 30))).astype(np.float32)
    # faces
    fc = cl[nd]
    collapsed = (fc[:, 0] == fc[:, 1]) | (fc[:, 1] == fc[:, 2]) | (fc[:, 0] == fc[:, 2])
    kept = fc[~collapsed]
    flat = kept.reshape(-1)
    uniq, first, finv = np.unique(flat, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    number = np.empty(len(uniq), np.int64)
    number[order] = np.arange(len(uniq))
    old = uniq[order]
    st = {"n_verts_in": len(v), "n_tris_in": F, "used_verts_in": int(used.sum()), "degenerate_in": n_deg, "cells": len(ukeys),
          "collapsed": int(collapsed.sum()), "n_verts": len(uniq), "n_tris": len(kept), "largest_cell": int(counts.max()) if len(counts) else 0,
          "exponent": e}
    if dry:
        return None, None, None, st
    if len(kept) == 0:
        raise SimplifyError(EMPTY_BUFFERS, "nothing kept")
    return pos[old].copy(), number[finv.reshape(-1)].reshape(-1, 3).astype(np.uint32), ukeys[old].copy(), st
