"""A numpy twin of the dual-contouring indexed-mesh contract (include/gsdf_hip.h, "indexed meshes: dual contouring"): which quads
there are, in which order, and the key of every slot -- from the oracle's evaluator alone. Nothing here looks at a device result.

The lattice is taken from the oracle's bounds exactly as oracle/orc_render.c: orc_render_dualcontour takes it (bounds + -res/2 in
float32, make_icube's levels, cube origin = origin + res * float32(i)); a cube is kept unless abs(d(origin)) >= 2 res; the three edge
ends are origin.x + res, origin.y + res, origin.z + res, evaluated on their own (they are not the neighbours' origins bit for bit).
The positions are not restated: the soup is the oracle's own triangle list, which is in this order, and weldref.weld_soup welds it by
these keys."""
import numpy as np

import weldref as W

F32 = np.float32
KIND = 5
# EdgeNeighborsX/Y/Z (glrender/dual_contour.go:271-287): per axis the four cubes around the edge, offsets in cube units
NEIGHBORS = np.array([[[0, -1, -1], [0, 0, -1], [0, 0, 0], [0, -1, 0]],
                      [[-1, 0, -1], [-1, 0, 0], [0, 0, 0], [0, 0, -1]],
                      [[-1, -1, 0], [0, -1, 0], [0, 0, 0], [-1, 0, 0]]], np.int64)
CORNERS = np.array([0, 1, 2, 2, 3, 0])  # quad -> the six slots of its two triangles


def lattice_of(bounds, res):
    """(origin (3,) float32, levels) of DualContourRenderer.Reset (dual_contour.go:26-41)."""
    res = F32(res)
    bb = np.asarray(bounds, F32)
    sub = F32(res / F32(2))
    mn, mx = (bb[:3] + -sub).astype(F32), (bb[3:] + -sub).astype(F32)
    long_axis = F32((mx - mn).astype(F32).max())
    levels = int(np.ceil(F32(np.log2(np.float64(F32(long_axis / res)))))) + 1
    return mn, levels


def quads(sdf, res, levels=None):
    """The quads in contract order: {'coords': (Q, 4, 3) int64 lattice coordinates of q0..q3 (after the flip), 'axis': (Q,),
    'cube': (Q, 3) the cube the edge belongs to, 'origin', 'levels', 'n_kept'}."""
    res = F32(res)
    origin, lv = lattice_of(sdf.Bounds(), res)
    levels = lv if levels is None else int(levels)
    if levels > 10:
        raise ValueError("more than 10 levels: the oracle refuses the lattice")
    n = 1 << (levels - 1)
    ax = np.arange(n)
    grid = np.full((n, n, n), -1, np.int32)  # [z, y, x] -> kept cube number, in (z, y, x) order
    kept, d0 = [], []
    xs = (origin[0] + res * ax.astype(F32)).astype(F32)
    ys = (origin[1] + res * ax.astype(F32)).astype(F32)
    zs = (origin[2] + res * ax.astype(F32)).astype(F32)
    count = 0
    for z in range(n):
        pos = np.empty((n, n, 3), F32)
        pos[..., 0], pos[..., 1], pos[..., 2] = xs[None, :], ys[:, None], zs[z]
        d = sdf.Evaluate(pos.reshape(-1, 3)).reshape(n, n)
        with np.errstate(invalid="ignore"):
            keep = ~(np.abs(d) >= F32(res * F32(2)))
        yy, xx = np.nonzero(keep)  # row-major: y, then x
        grid[z, yy, xx] = count + np.arange(len(yy))
        count += len(yy)
        kept.append(np.stack([xx, yy, np.full(len(yy), z)], axis=1))
        d0.append(d[yy, xx])
    kept = np.concatenate(kept).astype(np.int64)
    d0 = np.concatenate(d0).astype(F32)
    o = np.stack([xs[kept[:, 0]], ys[kept[:, 1]], zs[kept[:, 2]]], axis=1)
    ends = np.repeat(o[:, None, :], 3, axis=1)
    for a in range(3):
        ends[:, a, a] = (o[:, a] + res).astype(F32)
    de = sdf.Evaluate(ends.reshape(-1, 3)).reshape(-1, 3) if len(kept) else np.zeros((0, 3), F32)
    sign = lambda v: np.ascontiguousarray(v, F32).view(np.uint32) >> 31
    active = sign(de) != sign(d0)[:, None]
    ci, ai = np.nonzero(active)  # cube-major, then axis: (z, y, x, a)
    nbr = kept[ci][:, None, :] + NEIGHBORS[ai]
    inside = ((nbr >= 0) & (nbr < n)).all(axis=2)
    nc = np.clip(nbr, 0, n - 1)
    idx = np.where(inside, grid[nc[..., 2], nc[..., 1], nc[..., 0]], -1)
    ok = (idx >= 0).all(axis=1)
    ci, ai, nbr = ci[ok], ai[ok], nbr[ok]
    with np.errstate(invalid="ignore"):
        flip = (de[ci, ai] - d0[ci]).astype(F32) < 0
    coords = np.where(flip[:, None, None], nbr[:, ::-1, :], nbr)
    return {"coords": coords, "axis": ai, "cube": kept[ci], "origin": origin, "levels": levels, "n_kept": len(kept), "res": res}


def slot_keys(q):
    """(S,) uint64: the key of every slot, quad g = faces 2 g = (q0, q1, q2), 2 g + 1 = (q2, q3, q0)."""
    return W.pack_key(q["coords"][:, CORNERS, :].reshape(-1, 3), KIND)


def mesh(sdf, res, chiseled=False):
    """The contract's (verts, idx, keys) and what they were made of: (verts, idx, keys, soup (S, 3), quads dict, oracle MeshResult)."""
    ref = sdf.render_dualcontour(F32(res), chiseled)
    q = quads(sdf, res, ref.levels)
    keys = slot_keys(q)
    soup = ref.tris.reshape(-1, 3)
    if len(keys) != len(soup):
        raise AssertionError(f"the twin has {len(keys)} slots, the oracle {len(soup)}")
    v, i, k = W.weld_soup(soup, keys)
    return v, i, k, soup, q, ref


def cases(b):
    """(name, shape, res) of the shapes the CPU and the GPU tests hold to each other: tests/test_gpu_mesh.py's dual-contouring cases,
    and a long box -- 8 levels, lattice rows along x with more than 64 quads (more than a wave)."""
    return [("sphere", b.NewSphere(1.0), 1.0 / 8), ("box", b.NewBox(2, 2, 2, 0), 2.0 / 8), ("bolt", b.Scene("bolt"), 0.5),
            ("npt-flange", b.Scene("npt-flange"), 0.9), ("knurled-cylinder", b.Scene("knurled-cylinder"), 0.8),
            ("torus-hex", b.Union(b.NewTorus(1.0, 0.3), b.NewHexagonalPrism(0.4, 0.6)), 1.0 / 6), ("long-box", b.NewBox(8, 0.5, 0.5, 0), 0.08)]
