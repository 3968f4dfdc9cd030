"""CPU twin of the contour tracer (include/gsdf_hip.h, section "contours"), written from that contract in numpy float32 over any
Evaluate (the oracle's by default): the lattice, the inside test, the cut edges and their vertices, the segments of the sixteen cell
cases as succ (tail -> head), and the loops by a plain walk along succ from each leader. What the device must equal, to the byte."""
import math

import numpy as np

F = np.float32
NONE = -1

# case -> segments (tail, head); cell edges B 0 (bottom), R 1, T 2, L 3; the part on the left of tail -> head
B, R, T, L = 0, 1, 2, 3
SEGMENTS = {1: [(B, L)], 2: [(R, B)], 3: [(R, L)], 4: [(T, R)], 5: [(B, L), (T, R)], 6: [(T, B)], 7: [(T, L)], 8: [(L, T)], 9: [(B, T)],
            10: [(R, B), (L, T)], 11: [(R, T)], 12: [(L, R)], 13: [(B, R)], 14: [(L, B)]}


def axis_nodes(lo, hi, res):
    q = F(F(F(hi) - F(lo)) / F(res))
    if not q >= 0:
        return 4
    if not q < 2.0 ** 31:
        raise ValueError("lattice too large")
    return int(math.floor(float(q))) + 4


def lattice(bb, res):
    """(nx, ny, xs, ys): the node coordinates, float32."""
    bb = np.asarray(bb, F)
    res = F(res)
    if not (np.isfinite(res) and res > 0) or not np.isfinite(bb[[0, 1, 3, 4]]).all():
        raise ValueError("bad res or bounds")
    nx, ny = axis_nodes(bb[0], bb[3], res), axis_nodes(bb[1], bb[4], res)
    if nx * ny >= 2 ** 31:
        raise ValueError("lattice too large")
    xs = (F(bb[0] - res) + (np.arange(nx, dtype=F) * res).astype(F)).astype(F)
    ys = (F(bb[1] - res) + (np.arange(ny, dtype=F) * res).astype(F)).astype(F)
    return nx, ny, xs, ys


def positions(xs, ys, z=None):
    gx, gy = np.meshgrid(xs, ys)  # row j, column i
    cols = [gx.ravel(), gy.ravel()] + ([np.full(gx.size, F(z), F)] if z is not None else [])
    return np.ascontiguousarray(np.stack(cols, axis=1).astype(F))


class Layer:
    pass


def trace_layer(d, xs, ys, res):
    """One layer: d (ny, nx) float32 distances. -> Layer with succ (dense over the edge keys, NONE where the edge has no segment
    leaving it), cut (bool over the edge keys), xy / keys / loop_start in the contract's order, and the counts."""
    ny, nx = d.shape
    res = F(res)
    interior = np.zeros((ny, nx), bool)
    interior[1:-1, 1:-1] = True
    neg = d < 0
    inside = neg & interior
    out = Layer()
    out.border_inside = int((neg & ~interior).sum())
    out.nonfinite_nodes = int((~np.isfinite(d)).sum())
    node = np.arange(ny * nx, dtype=np.int64).reshape(ny, nx)
    # cut edges
    cut = np.zeros(2 * nx * ny, bool)
    cut[(2 * node[:, :-1])[inside[:, :-1] != inside[:, 1:]]] = True
    cut[(2 * node[:-1, :] + 1)[inside[:-1, :] != inside[1:, :]]] = True
    # segments
    c = (inside[:-1, :-1] * 1 + inside[:-1, 1:] * 2 + inside[1:, 1:] * 4 + inside[1:, :-1] * 8)
    n0 = node[:-1, :-1]
    edge = [2 * n0, 2 * (n0 + 1) + 1, 2 * (n0 + nx), 2 * n0 + 1]  # B, R, T, L of every cell
    succ = np.full(2 * nx * ny, NONE, np.int64)
    writes = np.zeros(2 * nx * ny, np.int64)
    for case, segs in SEGMENTS.items():
        m = c == case
        for tail, head in segs:
            succ[edge[tail][m]] = edge[head][m]
            np.add.at(writes, edge[tail][m], 1)
    out.succ, out.cut, out.writes = succ, cut, writes
    out.saddle_cells = int(((c == 5) | (c == 10)).sum())
    out.case_counts = np.bincount(c.ravel(), minlength=16)
    # vertices of the cut edges, by key
    keys = np.flatnonzero(cut)
    axis, n = keys & 1, keys >> 1
    j, i = n // nx, n % nx
    j2, i2 = j + axis, i + (1 - axis)
    d_lo, d_hi = d[j, i], d[j2, i2]
    d_out = np.where(inside[j, i], d_hi, d_lo)
    ok = np.isfinite(d_lo) & np.isfinite(d_hi) & (d_out >= 0)
    with np.errstate(all="ignore"):
        t = np.where(ok, (d_lo / (d_lo - d_hi).astype(F)).astype(F), F(0.5)).astype(F)
    step = (t * res).astype(F)
    vx = np.where(axis == 0, (xs[i] + step).astype(F), xs[i]).astype(F)
    vy = np.where(axis == 1, (ys[j] + step).astype(F), ys[j]).astype(F)
    # loops: from each leader (the smallest key not yet visited) along succ
    at = np.full(2 * nx * ny, -1, np.int64)
    at[keys] = np.arange(len(keys))
    seen = np.zeros(len(keys), bool)
    order, starts = [], [0]
    for v0 in range(len(keys)):
        if seen[v0]:
            continue
        v = v0
        while not seen[v]:
            seen[v] = True
            order.append(v)
            nxt = succ[keys[v]]
            if nxt == NONE or at[nxt] < 0:
                raise AssertionError("succ leaves the cut edges")
            v = at[nxt]
        if v != v0:
            raise AssertionError("succ is not a permutation")
        starts.append(len(order))
    order = np.array(order, np.int64)
    out.keys = keys[order].astype(np.uint32)
    out.xy = np.ascontiguousarray(np.stack([vx[order], vy[order]], axis=1).astype(F)).reshape(-1, 2)
    out.loop_start = np.array(starts, np.int64)
    return out


class Contour:
    def loops(self, layer=None):
        return [self.xy[self.loop_start[q]:self.loop_start[q + 1]] for q in range(len(self.loop_layer)) if layer is None or self.loop_layer[q] == layer]

    def areas(self):
        return np.array([area(l) for l in self.loops()], np.float64)


def area(xy):
    p = np.asarray(xy, np.float64)
    q = np.roll(p, -1, axis=0)
    return 0.5 * float(np.sum(p[:, 0] * q[:, 1] - q[:, 0] * p[:, 1]))


def perimeter(xy):
    p = np.asarray(xy, np.float64)
    return float(np.sqrt(((np.roll(p, -1, axis=0) - p) ** 2).sum(axis=1)).sum())


def ceil_log2(n):
    r = 0
    while (1 << r) < n:
        r += 1
    return r


def contour(evaluate, bb, res, z=None, order=None):
    """The twin of gsdf_hip_contour2 (z None) / gsdf_hip_slice3 (z: the float32 heights). evaluate(pos) -> float32 distances;
    order: a permutation of the lattice nodes to evaluate them in (the result must not depend on it)."""
    nx, ny, xs, ys = lattice(bb, res)
    zs = [None] if z is None else [F(v) for v in np.asarray(z, F).reshape(-1)]
    if not zs:
        raise ValueError("no layers")
    out = Contour()
    out.layers = []
    xy, keys, starts, layers = [], [], [0], []
    for k, zk in enumerate(zs):
        pos = positions(xs, ys, zk)
        if order is None:
            d = evaluate(pos)
        else:
            d = np.empty(len(pos), F)
            d[order] = evaluate(pos[order])
        lay = trace_layer(np.asarray(d, F).reshape(ny, nx), xs, ys, res)
        out.layers.append(lay)
        base = starts[-1]
        xy.append(lay.xy)
        keys.append(lay.keys)
        starts += [base + int(s) for s in lay.loop_start[1:]]
        layers += [k] * (len(lay.loop_start) - 1)
    out.xy = np.ascontiguousarray(np.concatenate(xy).astype(F)).reshape(-1, 2)
    out.keys = np.concatenate(keys).astype(np.uint32)
    out.loop_start = np.array(starts, np.uint32)
    out.loop_layer = np.array(layers, np.uint32)
    out.stats = {"nx": nx, "ny": ny, "n_layers": len(zs), "n_verts": len(out.keys), "n_loops": len(layers),
                 "border_inside": sum(l.border_inside for l in out.layers), "nonfinite_nodes": sum(l.nonfinite_nodes for l in out.layers),
                 "saddle_cells": sum(l.saddle_cells for l in out.layers), "rank_rounds": ceil_log2(max(len(l.keys) for l in out.layers)),
                 "evals": nx * ny * len(zs)}
    return out


def of_oracle(tree, res, z=None, order=None):
    from oracle.oracle import OracleSDF
    o = OracleSDF(tree)
    return contour(o.Evaluate, o.Bounds(), res, z, order)


def layer_heights(bb, h):
    """z_k = fl(bb.min.z + fl((k + 0.5) h)), float32, while below bb.max.z (gsdf_amd.hip.layer_heights)."""
    bb = np.asarray(bb, F)
    h = F(h)
    n = int(math.ceil(float(F(bb[5] - bb[2]) / h))) + 1
    z = (F(bb[2]) + ((np.arange(n, dtype=F) + F(0.5)) * h).astype(F)).astype(F)
    return np.ascontiguousarray(z[z < bb[5]])


# ---- what the tests of the twin and of the device share ------------------------------------------------------------------------
def res_for(bb, div):
    """diag / div of the xy bounds (float32); 0.1 where the bounds are empty."""
    bb = np.asarray(bb, F)
    diag = math.hypot(float(bb[3] - bb[0]), float(bb[4] - bb[1]))
    return F(diag / div) if diag > 0 else F(0.1)


def check_structure(c):
    """succ is a permutation of exactly the cut edges; every leader is an axis-1 edge; loops partition the vertices."""
    for lay in c.layers:
        dom = lay.succ != NONE
        assert (dom == lay.cut).all(), "the domain of succ is not the cut-edge set"
        assert (lay.writes[dom] == 1).all() and (lay.writes[~dom] == 0).all(), "a succ slot with more than one writer"
        img = np.sort(lay.succ[dom])
        assert (img == np.flatnonzero(lay.cut)).all(), "succ is not a permutation of the cut edges"
    assert c.loop_start[0] == 0 and c.loop_start[-1] == len(c.keys) and (np.diff(c.loop_start.astype(np.int64)) >= 4).all()
    leaders = c.keys[c.loop_start[:-1]]
    assert (leaders & 1 == 1).all(), "a leader on an axis-0 edge"
    for q in range(len(c.loop_layer)):
        k = c.keys[c.loop_start[q]:c.loop_start[q + 1]]
        assert k.min() == k[0]
    order = list(zip(c.loop_layer.tolist(), leaders.tolist()))
    assert order == sorted(order)


def saddle_shape(b, like):
    sx = 0.5 if like else -0.5
    return b.Union2D(b.Translate2D(b.NewRectangle(1, 1), sx, 0.5), b.Translate2D(b.NewRectangle(1, 1), -sx, -0.5))
