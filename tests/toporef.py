"""A numpy + Python-integer twin of the indexed-mesh REPORT contract (include/gsdf_hip.h, "indexed meshes: report and extract"):
(verts, idx) in, the report, the shell table and the shell numbers out. Nothing here looks at a device result.

Pairs by np.unique; shells by iterated minimum-label propagation with pointer jumping (the device uses a lock-free union-find);
the measures with the contract's float64 terms in the contract's order, quantised with np.rint, summed as integers (low 32 bits and
the arithmetic-shifted rest in int64, which fewer than 2^31 terms cannot overflow; combined in Python ints), converted back with one
rounding (int / 2**s and float(int) are correctly rounded in Python)."""
import math

import numpy as np

NONE = 0xffffffff
SHELL_DTYPE = np.dtype([("n_verts", "<u8"), ("n_tris", "<u8"), ("nonfinite", "<u8"), ("edges", "<u8"), ("boundary_edges", "<u8"),
                        ("nonmanifold_edges", "<u8"), ("misoriented_edges", "<u8"), ("euler", "<i8"), ("area", "<f8"), ("volume", "<f8"),
                        ("centroid", "<f8", (3,)), ("bbox", "<f4", (6,)), ("label", "<u4"), ("reserved", "<u4")])
QNAN = np.array([0x7ff8000000000000], np.uint64).view(np.float64)[0]


def exponent_of(verts):
    """e of the contract: the smallest integer >= -125 with |x| < 2^e for every finite coordinate."""
    bits = np.ascontiguousarray(verts, np.float32).reshape(-1).view(np.uint32) & np.uint32(0x7fffffff)
    fin = bits[bits < 0x7f800000]
    biased = int(fin.max()) >> 23 if fin.size else 0
    return max(biased, 1) - 126


def _ordered(bits):
    return bits ^ np.where(bits >> np.uint32(31) != 0, np.uint32(0xffffffff), np.uint32(0x80000000))


def _unordered(o):
    o = np.asarray(o, np.uint32)
    return np.where(o & np.uint32(0x80000000) != 0, o ^ np.uint32(0x80000000), ~o).astype(np.uint32).view(np.float32)


def _value(t, shift):
    """The integer t times 2^-shift as float64, one rounding."""
    return np.float64(t / (1 << shift)) if shift >= 0 else np.float64(float(t << -shift))


def _quotient(m, v):
    return QNAN if v == 0 else np.float64(m) / np.float64(v)


def components(n_verts, a, b):
    """Minimum vertex number of the connected component of every vertex, for the graph with edges (a[i], b[i])."""
    lab = np.arange(n_verts, dtype=np.int64)
    while True:
        new = lab.copy()
        m = np.minimum(lab[a], lab[b])
        np.minimum.at(new, a, m)
        np.minimum.at(new, b, m)
        new = new[new]  # a label is a vertex of the same component: so is its label
        if (new == lab).all():
            return lab
        lab = new


def terms(a, b, c):
    """The contract's float64 terms of faces with corners a, b, c (n, 3) float32: (area, volume, moment x, y, z)."""
    a, b, c = (np.asarray(x, np.float32).astype(np.float64) for x in (a, b, c))
    u, w = b - a, c - a
    nx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    ny = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    nz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    area = 0.5 * np.sqrt((nx * nx + ny * ny) + nz * nz)
    mx = b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]
    my = b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2]
    mz = b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0]
    det = (a[:, 0] * mx + a[:, 1] * my) + a[:, 2] * mz
    out = [area, det / 6.0]
    for k in range(3):
        out.append((det * ((a[:, k] + b[:, k]) + c[:, k])) / 24.0)
    return out


def analyse(verts, idx):
    """{'report': dict, 'shells': SHELL_DTYPE array, 'shell_of_vertex': (V,) uint32, 'shell_of_face': (F,) uint32}."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    i = np.asarray(idx).astype(np.int64).reshape(-1, 3)
    V, F = len(v), len(i)
    deg = (i[:, 0] == i[:, 1]) | (i[:, 1] == i[:, 2]) | (i[:, 0] == i[:, 2])
    nd = i[~deg]
    used = np.zeros(V, bool)
    used[nd.reshape(-1)] = True
    # pairs
    p, q = nd[:, [0, 1, 2]].reshape(-1), nd[:, [1, 2, 0]].reshape(-1)
    code = (np.minimum(p, q).astype(np.uint64) << np.uint64(32)) | np.maximum(p, q).astype(np.uint64)
    uc, inv = np.unique(code, return_inverse=True)
    inv = inv.reshape(-1)
    fw = np.bincount(inv[p < q], minlength=len(uc)).astype(np.int64)
    rv = np.bincount(inv[p > q], minlength=len(uc)).astype(np.int64)
    pa, pb = (uc >> np.uint64(32)).astype(np.int64), (uc & np.uint64(0xffffffff)).astype(np.int64)
    # shells
    lab = components(V, pa, pb)
    labels = np.unique(lab[used])
    n_shells = len(labels)
    sov = np.where(used, np.searchsorted(labels, lab), NONE).astype(np.uint32)
    sof = np.full(F, NONE, np.uint32)
    sof[~deg] = sov[nd[:, 0]]
    sh = np.zeros(n_shells, SHELL_DTYPE)
    sh["label"] = labels
    sh["n_verts"] = np.bincount(sov[used], minlength=n_shells)
    sh["n_tris"] = np.bincount(sof[~deg], minlength=n_shells)
    ps = sov[pa]  # a pair's shell: that of its smaller vertex
    uses = fw + rv
    sh["edges"] = np.bincount(ps, minlength=n_shells)
    sh["boundary_edges"] = np.bincount(ps[uses == 1], minlength=n_shells)
    sh["nonmanifold_edges"] = np.bincount(ps[uses > 2], minlength=n_shells)
    sh["misoriented_edges"] = np.bincount(ps[(uses == 2) & (fw != 1)], minlength=n_shells)
    sh["euler"] = sh["n_verts"].astype(np.int64) - sh["edges"].astype(np.int64) + sh["n_tris"].astype(np.int64)
    # measures over the finite non-degenerate faces
    fin = np.isfinite(v[nd.reshape(-1)]).reshape(-1, 9).all(axis=1)
    sh["nonfinite"] = np.bincount(sof[~deg][~fin], minlength=n_shells)
    ff = nd[fin]
    fs = sof[~deg][fin].astype(np.int64)
    e = exponent_of(v)
    shifts = [59 - 2 * e, 62 - 3 * e, 62 - 4 * e, 62 - 4 * e, 62 - 4 * e]
    with np.errstate(all="ignore"):
        tt = terms(v[ff[:, 0]], v[ff[:, 1]], v[ff[:, 2]])
    ints = np.zeros((n_shells, 5), object)
    for k, (t, s) in enumerate(zip(tt, shifts)):
        qk = np.rint(t * math.ldexp(1.0, s)).astype(np.int64)
        lo, hi = np.zeros(n_shells, np.int64), np.zeros(n_shells, np.int64)
        np.add.at(lo, fs, qk & np.int64(0xffffffff))
        np.add.at(hi, fs, qk >> np.int64(32))
        for j in range(n_shells):
            ints[j, k] = int(hi[j]) * 2 ** 32 + int(lo[j])
    bb_min = np.full((n_shells, 3), 0xff800000, np.uint32)
    bb_max = np.full((n_shells, 3), 0x007fffff, np.uint32)
    ob = _ordered(v.view(np.uint32))
    for c in range(3):
        np.minimum.at(bb_min, fs, ob[ff[:, c]])
        np.maximum.at(bb_max, fs, ob[ff[:, c]])
    for j in range(n_shells):
        val = [_value(ints[j, k], shifts[k]) for k in range(5)]
        sh["area"][j], sh["volume"][j] = val[0], val[1]
        sh["centroid"][j] = [_quotient(val[2 + k], val[1]) for k in range(3)]
    sh["bbox"] = np.concatenate([_unordered(bb_min), _unordered(bb_max)], axis=1) if n_shells else np.zeros((0, 6), np.float32)
    tot = [sum(ints[j, k] for j in range(n_shells)) for k in range(5)]
    tv = [_value(tot[k], shifts[k]) for k in range(5)]
    rep = {"n_verts": V, "n_tris": F, "degenerate": int(deg.sum()), "nonfinite": int((~fin).sum()), "used_verts": int(used.sum()),
           "edges": len(uc), "boundary_edges": int((uses == 1).sum()), "nonmanifold_edges": int((uses > 2).sum()),
           "misoriented_edges": int(((uses == 2) & (fw != 1)).sum()), "n_shells": n_shells}
    rep["euler"] = rep["used_verts"] - rep["edges"] + (F - rep["degenerate"])
    rep["area"], rep["volume"] = tv[0], tv[1]
    rep["centroid"] = np.array([_quotient(tv[2 + k], tv[1]) for k in range(3)], np.float64)
    rep["bbox"] = np.concatenate([_unordered(bb_min.min(axis=0) if n_shells else np.full(3, 0xff800000, np.uint32)),
                                  _unordered(bb_max.max(axis=0) if n_shells else np.full(3, 0x007fffff, np.uint32))]).astype(np.float32)
    rep["closed_oriented"] = int(rep["degenerate"] == 0 and rep["boundary_edges"] == 0 and rep["nonmanifold_edges"] == 0 and rep["misoriented_edges"] == 0)
    rep["exponent"] = e
    return {"report": rep, "shells": sh, "shell_of_vertex": sov, "shell_of_face": sof}


def extract(verts, idx, keys, normals, shell_of_face, keep=None, drop_degenerate=True):
    """The contract's extract: (verts, idx, keys, normals or None) of the kept faces, vertices numbered by first appearance."""
    v = np.ascontiguousarray(verts, np.float32).reshape(-1, 3)
    i = np.asarray(idx).astype(np.int64).reshape(-1, 3)
    sof = np.asarray(shell_of_face).astype(np.int64)
    isdeg = sof == NONE
    if keep is None:
        kf = np.where(isdeg, not drop_degenerate, True)
    else:
        kf = np.where(isdeg, False, np.asarray(keep, bool)[np.where(isdeg, 0, sof)])
    flat = i[kf].reshape(-1)
    uniq, first, inv = np.unique(flat, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    number = np.empty(len(uniq), np.int64)
    number[order] = np.arange(len(uniq))
    old = uniq[order]
    return (v[old].copy(), number[inv.reshape(-1)].reshape(-1, 3).astype(np.uint32), np.asarray(keys, np.uint64)[old].copy(),
            None if normals is None else np.asarray(normals, np.float32)[old].copy())


# ---- hand meshes with known answers -------------------------------------------------------------------------------------------------
TET_V = np.array([[0, 0, 0], [6, 0, 0], [0, 6, 0], [0, 0, 6]], np.float32)      # volume 36, area 54 + 18 sqrt(3), centroid (1.5, 1.5, 1.5)
TET_I = np.array([[0, 2, 1], [0, 1, 3], [1, 2, 3], [0, 3, 2]], np.uint32)       # outward


def cube(lo, hi, inward=False):
    """An axis-aligned cube as 8 vertices and 12 outward (or inward) triangles."""
    lo, hi = float(lo), float(hi)
    v = np.array([[x, y, z] for z in (lo, hi) for y in (lo, hi) for x in (lo, hi)], np.float32)
    quads = [(0, 2, 3, 1), (4, 5, 7, 6), (0, 1, 5, 4), (2, 6, 7, 3), (0, 4, 6, 2), (1, 3, 7, 5)]
    i = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.uint32)
    return v, (i[:, ::-1].copy() if inward else i)


def join(*meshes):
    vs, is_, off = [], [], 0
    for v, i in meshes:
        vs.append(v)
        is_.append(i.astype(np.uint32) + np.uint32(off))
        off += len(v)
    return np.concatenate(vs).astype(np.float32), np.concatenate(is_).astype(np.uint32)


def hand_meshes():
    """name -> (verts, idx)."""
    out = {"tet": (TET_V, TET_I), "tet-hole": (TET_V, TET_I[:3]), "tet-degenerate": (TET_V, np.vstack([TET_I, [[0, 0, 1]]]).astype(np.uint32))}
    fl = TET_I.copy()
    fl[0] = fl[0][::-1]
    out["tet-flipped"] = (TET_V, fl)
    # a second tetrahedron on the other side of the edge (0, 1): that pair is used four times
    v2 = np.vstack([TET_V, [[0, -6, 0], [0, 0, -6]]]).astype(np.float32)
    t2 = np.array([[0, 4, 1], [0, 1, 5], [1, 4, 5], [0, 5, 4]], np.uint32)  # outward too
    out["two-tets-one-edge"] = (v2, np.vstack([TET_I, t2]).astype(np.uint32))
    out["two-tets-apart"] = join((TET_V, TET_I), (TET_V + np.float32(18), TET_I))
    out["cube-in-cube"] = join(cube(0, 24), cube(6, 18, inward=True))  # multiples of 6: every term is an integer
    vn = TET_V.copy()
    vn[3, 1] = np.nan
    out["tet-nan"] = (vn, TET_I)
    return out


def random_soup(seed=7, n_verts=5000, n_tris=20000):
    """Random index triples over clustered vertex ranges (hundreds of shells, every edge class, mixed waves), some faces repeated,
    some degenerate, a few non-finite vertices."""
    rng = np.random.default_rng(seed)
    v = (rng.standard_normal((n_verts, 3)) * 3).astype(np.float32)
    v[rng.choice(n_verts, 5, replace=False), rng.integers(0, 3, 5)] = [np.nan, np.inf, -np.inf, np.nan, np.inf]
    # faces inside windows of 6 consecutive vertices: small components; a tail of long-range faces joins some of them
    base = rng.integers(0, n_verts - 6, n_tris)
    i = (base[:, None] // 6 * 6 + rng.integers(0, 6, (n_tris, 3))).astype(np.int64)
    far = rng.choice(n_tris, n_tris // 50, replace=False)
    i[far] = rng.integers(0, n_verts // 4, (len(far), 3))
    rep = rng.choice(n_tris, n_tris // 20, replace=False)
    i[rep] = i[(rep + 1) % n_tris]
    return v, i.astype(np.uint32)
