"""A numpy twin of the indexed-mesh contract (include/gsdf_hip.h, "indexed meshes"): cut leaves in, (verts, idx, keys) out.

The distances come from the oracle's evaluator, the cases from the marching-cubes tables the oracle exports; nothing here looks at
a device result. A leaf's corners are formed as the mesher forms them: origin O + res * float32(i) per axis, max corner = that + res
(so the two copies of a lattice plane that neighbouring leaves see differ in their last bits, which is why the weld is by key)."""
import numpy as np

from oracle.oracle import mc_tables

F32 = np.float32
SQRT3 = F32(1.73205080757)  # glrender.go:9
# marchcubes.go's edge -> corner pairs and Box.Vertices' corner offsets (x, y, z per corner)
PAIR = np.array([[0, 1], [1, 2], [2, 3], [3, 0], [4, 5], [5, 6], [6, 7], [7, 4], [0, 4], [1, 5], [2, 6], [3, 7]])
CORNER = np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0, 0, 1], [1, 0, 1], [1, 1, 1], [0, 1, 1]])


def lattice_of(bounds, res):
    """(origin (3,) float32, levels) of the octree over `bounds` (octreerenderer.go:79-80, 222-235): the bounds scaled by 1.01
    about their centre, in float32."""
    bb = np.asarray(bounds, F32)
    mn, mx = bb[:3], bb[3:]
    c = F32(0.5) * (mn + mx)
    h = F32(0.5) * np.maximum(F32(1.01) * (mx - mn), F32(0))
    lo, hi = c - h, c + h
    levels = int(np.ceil(F32(np.log2(np.float64(F32((hi - lo).max() / F32(res))))))) + 1
    return lo.astype(F32), levels


def leaf_corners(leaves, origin, res):
    """(n, 8, 3) float32 corner positions of the leaves with integer coordinates `leaves` (n, 3)."""
    res = F32(res)
    o = (np.asarray(origin, F32)[None, :] + res * np.asarray(leaves).astype(F32)).astype(F32)
    m = (o + res).astype(F32)
    return np.where(CORNER[None, :, :] == 1, m[:, None, :], o[:, None, :]).astype(F32)


def pack_key(ixyz, kind):
    ixyz = np.asarray(ixyz).astype(np.uint64)
    return ixyz[..., 0] | (ixyz[..., 1] << np.uint64(20)) | (ixyz[..., 2] << np.uint64(40)) | (np.asarray(kind).astype(np.uint64) << np.uint64(60))


def soup_of(sdf, leaves, origin, res):
    """Marching cubes (marchcubes.go:14-98) over the leaves in the given order: (soup (S, 3) float32 positions, keys (S,) uint64),
    slot 3 t + c = corner c of triangle t."""
    leaves = np.asarray(leaves, np.int64).reshape(-1, 3)
    res = F32(res)
    _, tri = mc_tables()
    pos = leaf_corners(leaves, origin, res)
    d = sdf.Evaluate(pos.reshape(-1, 3)).reshape(-1, 8)
    with np.errstate(invalid="ignore"):
        live = np.abs(d[:, 0]) <= F32(F32(2) * SQRT3) * res  # marchCubes' first-corner test
        case = ((d < 0) * (1 << np.arange(8))).sum(axis=1)
    case = np.where(live, case, 0)
    ntri = (tri[case] >= 0).sum(axis=1) // 3
    # one row per slot: its leaf and its edge; table order, corners of a triangle reversed (marchcubes.go:64-68)
    leaf_of = np.repeat(np.arange(len(leaves)), 3 * ntri)
    first = np.cumsum(3 * ntri) - 3 * ntri
    within = np.arange(len(leaf_of)) - np.repeat(first, 3 * ntri)
    k, j = within // 3, within % 3
    edge = tri[case[leaf_of], 3 * k + (2 - j)].astype(np.int64)
    a, b = PAIR[edge, 0], PAIR[edge, 1]
    p1, p2 = pos[leaf_of, a], pos[leaf_of, b]
    v1, v2 = d[leaf_of, a], d[leaf_of, b]
    eps = F32(1e-12)
    with np.errstate(all="ignore"):
        c1, c2 = np.abs(F32(0) - v1) < eps, np.abs(F32(0) - v2) < eps
        t = np.where(c1 & c2, F32(0.5), ((F32(0) - v1) / (v2 - v1)).astype(F32)).astype(F32)
        r = (p1 + (t[:, None] * (p2 - p1).astype(F32)).astype(F32)).astype(F32)
    r = np.where((c1 & ~c2)[:, None], p1, r)
    r = np.where((c2 & ~c1)[:, None], p2, r).astype(F32)
    # keys: a lattice point where mcInterpolate returned an end unchanged, else the lattice edge by its lower end
    oa, ob = CORNER[a], CORNER[b]
    axis = np.argmax(oa != ob, axis=1)
    snap = c1 != c2
    off = np.where(snap[:, None], np.where(c1[:, None], oa, ob), np.minimum(oa, ob))
    keys = pack_key(leaves[leaf_of] + off, np.where(snap, 3, axis))
    return r, keys


def weld_soup(soup, keys):
    """The contract's vertices and faces of a keyed soup: (verts (V, 3), idx (F, 3) uint32, vertex keys (V,))."""
    uniq, first, inv = np.unique(keys, return_index=True, return_inverse=True)  # first: the smallest slot of each key
    order = np.argsort(first, kind="stable")       # vertices numbered by their smallest slot
    number = np.empty(len(uniq), np.int64)
    number[order] = np.arange(len(uniq))
    owner = first[order]
    return soup[owner].copy(), number[inv].reshape(-1, 3).astype(np.uint32), keys[owner].copy()


def weld(sdf, leaves, origin, res):
    soup, keys = soup_of(sdf, leaves, origin, res)
    v, i, k = weld_soup(soup, keys)
    return v, i, k, soup


def leaves_of_triangles(tris, origin, res):
    """Candidate cut leaves of a triangle list on the lattice, sorted: the leaves under every triangle's centroid and corners (a
    superset of the leaves that made them; a leaf the surface does not cut contributes nothing to soup_of)."""
    t = np.asarray(tris, np.float64).reshape(-1, 3, 3)
    pts = np.concatenate([t.mean(axis=1), t.reshape(-1, 3)])
    pts = pts[np.isfinite(pts).all(axis=1)]
    ijk = np.floor((pts - np.asarray(origin, np.float64)) / np.float64(res)).astype(np.int64)
    ijk = ijk[(ijk >= 0).all(axis=1)]
    return np.unique(ijk, axis=0)


def edge_report(idx):
    """Connectivity of an indexed mesh: {'V', 'E', 'F', 'euler', 'degenerate', 'closed_oriented'}; closed_oriented = every directed
    edge (a, b) occurs once and (b, a) once."""
    idx = np.asarray(idx, np.int64).reshape(-1, 3)
    deg = (idx[:, 0] == idx[:, 1]) | (idx[:, 1] == idx[:, 2]) | (idx[:, 0] == idx[:, 2])
    a = idx[:, [0, 1, 2]].reshape(-1)
    b = idx[:, [1, 2, 0]].reshape(-1)
    n = int(idx.max()) + 1 if idx.size else 0
    code, rev = a * n + b, b * n + a
    uc, cnt = np.unique(code, return_counts=True)
    und = np.unique(np.minimum(a, b) * n + np.maximum(a, b))
    ok = bool((cnt == 1).all() and len(np.setdiff1d(rev, uc)) == 0 and not deg.any())
    V = len(np.unique(idx))
    return {"V": V, "E": len(und), "F": len(idx), "euler": V - len(und) + len(idx), "degenerate": int(deg.sum()), "closed_oriented": ok}


def sorted_triangles(tris):
    t = np.ascontiguousarray(tris, F32).reshape(-1, 9)
    return t[np.lexsort(t.T[::-1])]
