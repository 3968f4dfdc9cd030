"""CPU twin of the loops' offset (include/gsdf_hip.h, section "contours: offset"), written from that contract: numpy float64
elementwise operations (single IEEE operations, never fused) of every node against EVERY edge of its layer -- no culling, so that a
culling error on the device shows as a byte difference -- then contourref.trace_layer on every inset's lattice. What the device must
equal, to the byte."""
import struct

import numpy as np

import contourref as R

F = np.float32
MAX_INSETS = 8


def check_arguments(res, insets):
    res = F(res)
    insets = np.asarray(insets, F).reshape(-1)
    if not (np.isfinite(res) and res > 0):
        raise ValueError("res must be finite and positive")
    if not 1 <= len(insets) <= MAX_INSETS:
        raise ValueError("n_insets must be 1 .. 8")
    if not np.isfinite(insets).all():
        raise ValueError("a non-finite inset")
    return res, insets


def lattice(c, res, insets):
    """(nx, ny, xs, ys, band) of a call: the handle's exact box grown for the negative insets, then the tracer's lattice."""
    res, insets = check_arguments(res, insets)
    xy = np.asarray(c.xy, F).reshape(-1, 2)
    lo = xy.min(axis=0) if len(xy) else np.zeros(2, F)
    hi = xy.max(axis=0) if len(xy) else np.zeros(2, F)
    g = F(max(F(0), (-insets).max()))
    with np.errstate(over="ignore"):
        bb = np.array([F(lo[0] - g), F(lo[1] - g), 0, F(hi[0] + g), F(hi[1] + g), 0], F)
        band = F(F(np.abs(insets).max()) + F(F(2) * res))
    nx, ny, xs, ys = R.lattice(bb, res)
    if nx * ny * len(insets) >= 2 ** 31:
        raise ValueError("lattice too large")
    return nx, ny, xs, ys, band


def layer_edges(c, layer):
    """(a, b): the float64 ends of the edges of one layer (a vertex and its successor in the loop), (n, 2) each."""
    P = np.asarray(c.xy, F).astype(np.float64).reshape(-1, 2)
    ls = np.asarray(c.loop_start, np.int64)
    tails, heads = [], []
    for q in np.flatnonzero(np.asarray(c.loop_layer) == layer):
        v = np.arange(ls[q], ls[q + 1])
        tails.append(v)
        heads.append(np.roll(v, -1))
    if not tails:
        return np.zeros((0, 2)), np.zeros((0, 2))
    return P[np.concatenate(tails)], P[np.concatenate(heads)]


def distance_layer(a, b, xs, ys, band, clamp=True, block=256):
    """The contract's D of one layer over the lattice (ny, nx), float32, and its INSIDE and in-band node masks."""
    ny, nx = len(ys), len(xs)
    px = np.tile(xs.astype(np.float64), ny)[:, None]
    py = np.repeat(ys.astype(np.float64), nx)[:, None]
    m2 = np.full(nx * ny, np.inf)
    count = np.zeros(nx * ny, np.int64)
    for e0 in range(0, len(a), block):
        ax, ay, bx, by = a[None, e0:e0 + block, 0], a[None, e0:e0 + block, 1], b[None, e0:e0 + block, 0], b[None, e0:e0 + block, 1]
        with np.errstate(all="ignore"):
            ex, ey = bx - ax, by - ay
            wx, wy = px - ax, py - ay
            ee = (ex * ex) + (ey * ey)
            h = np.where(ee > 0, np.minimum(np.maximum(((wx * ex) + (wy * ey)) / ee, 0.0), 1.0), 0.0)
            qx, qy = wx - (h * ex), wy - (h * ey)
            d2 = (qx * qx) + (qy * qy)
            m2 = np.minimum(m2, d2.min(axis=1))
            straddle = (ay < py) != (by < py)
            t = (py - ay) / (by - ay)
            xc = ax + (t * (bx - ax))
            count += (straddle & (xc > px)).sum(axis=1)
    r = np.sqrt(m2)
    a_ = np.minimum(r, np.float64(band)) if clamp else r
    inside = (count & 1) == 1
    with np.errstate(over="ignore"):
        D = np.where(inside, -a_, a_).astype(F)
    return D.reshape(ny, nx), inside.reshape(ny, nx), (np.minimum(r, np.float64(band)) < np.float64(band)).reshape(ny, nx)


STATS_FORMAT = "<6Q4I4f"  # bytes 0 .. 79 of gsdf_offset_stats


def offset(c, res, insets, clamp=True):
    """The twin of gsdf_hip_contour_offset on a contoursimpref.Loops (or anything with its fields): a contourref.Contour with n_layers,
    D (the float32 lattice of every input layer), xs, ys, band and stats (the fields of gsdf_offset_stats before the times)."""
    res, insets = check_arguments(res, insets)
    nx, ny, xs, ys, band = lattice(c, res, insets)
    L, K = int(c.n_layers), len(insets)
    out = R.Contour()
    out.layers, out.D = [], []
    out.xs, out.ys, out.band = xs, ys, band
    xy, keys, starts, layers = [np.zeros((0, 2), F)], [np.zeros(0, np.uint32)], [0], []
    inside_nodes = band_nodes = 0
    for l in range(L):
        a, b = layer_edges(c, l)
        D, inside, in_band = distance_layer(a, b, xs, ys, band, clamp)
        out.D.append(D)
        inside_nodes += int(inside.sum())
        band_nodes += int(in_band.sum())
        for i in range(K):
            with np.errstate(over="ignore"):
                f = (D + insets[i]).astype(F)
            lay = R.trace_layer(f, xs, ys, res)
            out.layers.append(lay)
            base = starts[-1]
            xy.append(lay.xy)
            keys.append(lay.keys)
            starts += [base + int(s) for s in lay.loop_start[1:]]
            layers += [l * K + i] * (len(lay.loop_start) - 1)
    out.xy = np.ascontiguousarray(np.concatenate(xy).astype(F)).reshape(-1, 2)
    out.keys = np.concatenate(keys).astype(np.uint32)
    out.loop_start = np.array(starts, np.uint32)
    out.loop_layer = np.array(layers, np.uint32)
    out.n_layers = L * K
    out.stats = {"n_verts": len(out.keys), "n_loops": len(layers), "border_inside": sum(l.border_inside for l in out.layers),
                 "saddle_cells": sum(l.saddle_cells for l in out.layers), "inside_nodes": inside_nodes, "band_nodes": band_nodes,
                 "nx": nx, "ny": ny, "n_layers_in": L, "n_insets": K, "x0": xs[0], "y0": ys[0], "band": band, "res": res, "n_layers": L * K}
    return out


def stats_bytes(st):
    """Bytes 0 .. 79 of the gsdf_offset_stats the device must report."""
    return struct.pack(STATS_FORMAT, *(int(st[k]) for k in ("n_verts", "n_loops", "border_inside", "saddle_cells", "inside_nodes", "band_nodes", "nx", "ny",
                                                            "n_layers_in", "n_insets")), *(float(st[k]) for k in ("x0", "y0", "band", "res")))


def distance(c, res, insets, layer):
    """The twin of gsdf_hip_contour_distance: (ny, nx) float32."""
    nx, ny, xs, ys, band = lattice(c, res, insets)
    if not 0 <= layer < int(c.n_layers):
        raise ValueError("no such layer")
    a, b = layer_edges(c, layer)
    return distance_layer(a, b, xs, ys, band)[0]


# ---- what the tests of the twin and of the device share ------------------------------------------------------------------------
def same_bytes(got, want):
    """xy, keys, loop_start and loop_layer of two results, bit for bit."""
    assert got.loop_start.tolist() == want.loop_start.tolist()
    assert got.loop_layer.tolist() == want.loop_layer.tolist()
    assert (np.asarray(got.keys) == np.asarray(want.keys)).all()
    assert np.asarray(got.xy, F).reshape(-1, 2).shape == want.xy.shape
    assert (np.asarray(got.xy, F).reshape(-1, 2).view(np.uint32) == want.xy.view(np.uint32)).all()


def scaled(c, k):
    """The loops with every coordinate times 2^k (exact while nothing leaves the normal range)."""
    import contoursimpref as S
    return S.Loops(np.ldexp(np.asarray(c.xy, F), k).astype(F), c.loop_start, c.loop_layer, c.n_layers, c.keys)
