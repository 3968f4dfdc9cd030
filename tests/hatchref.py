"""CPU twin of the hatch fill (include/gsdf_hip.h, section "contours: hatch fill"), written from that contract: numpy float64
elementwise operations (single IEEE operations, never fused) over edges x candidate lines, Python integers for the length sums. What
the device must equal, to the byte."""
import math

import numpy as np

import contoursimpref as S

F = np.float32
LAYER_DTYPE = np.dtype([("length", "<f8"), ("n_segments", "<u8"), ("k_min", "<i4"), ("k_max", "<i4")])


class Hatch:
    """seg (n, 4) float32, line n int32, layer_start n_layers + 1 uint32, layers LAYER_DTYPE records, stats (a dict with the fields
    of gsdf_hatch_stats before ms_device); and what the tests of the twin itself look at: t of every crossing, the crossings per
    (layer, k) as line_counts, the sorted crossings as records."""

    def segments(self, layer):
        return self.seg[self.layer_start[layer]:self.layer_start[layer + 1]]


def directions(angles_deg):
    """float32(cos), float32(sin) of each angle, computed in float64: what ContourHIP.hatch hands the library."""
    a = np.radians(np.asarray(angles_deg, np.float64).reshape(-1))
    return np.stack([np.cos(a), np.sin(a)], axis=1).astype(F)


def check_arguments(c, spacing, dirs, offset):
    spacing, offset = F(spacing), F(offset)
    dirs = np.asarray(dirs, F).reshape(-1, 2)
    if not (np.isfinite(spacing) and spacing > 0):
        raise ValueError("spacing must be finite and positive")
    if not np.isfinite(offset):
        raise ValueError("offset must be finite")
    if not 1 <= len(dirs) <= 4:
        raise ValueError("n_dirs must be 1 .. 4")
    for dx, dy in dirs:
        if not (np.isfinite(dx) and np.isfinite(dy) and abs(dx) <= 1 and abs(dy) <= 1) or (dx == 0 and dy == 0):
            raise ValueError("bad dir")
    e = S.exponent(c.xy)
    if (math.ldexp(1.0, e + 1) + abs(float(offset))) / float(spacing) >= 2.0 ** 29:
        raise ValueError("spacing is too small for these coordinates")
    return float(spacing), float(offset), dirs.astype(np.float64), e


def hatch(c, spacing, dirs, offset=0.0):
    """The twin of gsdf_hip_contour_hatch on a contoursimpref.Loops (or anything with its fields)."""
    sp, off, dirs, e = check_arguments(c, spacing, dirs, offset)
    L = int(c.n_layers)
    P = np.asarray(c.xy, F).astype(np.float64).reshape(-1, 2)
    ls = np.asarray(c.loop_start, np.int64)
    V = len(P)
    out = Hatch()
    out.exponent = e
    if V:
        nxt = np.arange(1, V + 1, dtype=np.int64)
        nxt[ls[1:] - 1] = ls[:-1]
        layer_v = np.repeat(np.asarray(c.loop_layer, np.int64), np.diff(ls))
        d = dirs[layer_v % len(dirs)]
        dx, dy = d[:, 0], d[:, 1]
        xa, ya, xb, yb = P[:, 0], P[:, 1], P[nxt, 0], P[nxt, 1]
        sa, sb = ((-dy) * xa) + (dx * ya), ((-dy) * xb) + (dx * yb)
        ua, ub = (dx * xa) + (dy * ya), (dx * xb) + (dy * yb)
        # candidates: a margin around the estimate on both sides; the predicate decides, and the margins must come out uncrossed
        lo, hi = np.minimum(sa, sb), np.maximum(sa, sb)
        k0 = np.floor((lo - off) / sp).astype(np.int64) - 2
        k1 = np.floor((hi - off) / sp).astype(np.int64) + 2
        n_c = k1 - k0 + 1
        first = np.concatenate([[0], np.cumsum(n_c)])
        if first[-1] >= 1 << 32:
            raise OverflowError("2^32 crossings or more")
        j = np.repeat(np.arange(V, dtype=np.int64), n_c)
        k = k0[j] + (np.arange(first[-1], dtype=np.int64) - first[:-1][j])
        ck = off + (k.astype(np.float64) * sp)
        crossed = (sa[j] < ck) != (sb[j] < ck)
        assert not crossed[(k <= k0[j] + 1) | (k >= k1[j] - 1)].any(), "the candidate range is too narrow"
        j, k, ck = j[crossed], k[crossed], ck[crossed]
    else:
        j = k = np.zeros(0, np.int64)
        ck = np.zeros(0)
    n = len(j)
    if n:
        with np.errstate(all="raise"):
            t = (ck - sa[j]) / (sb[j] - sa[j])
        uc = ua[j] + (t * (ub[j] - ua[j]))
        xc = (xa[j] + (t * (xb[j] - xa[j]))).astype(F)
        yc = (ya[j] + (t * (yb[j] - ya[j]))).astype(F)
        lay = layer_v[j]
        order = np.lexsort((j, uc, k, lay))  # (the last key is the first to decide; -0.0 and 0.0 compare equal)
        j, k, t, uc, xc, yc, lay = (a[order] for a in (j, k, t, uc, xc, yc, lay))
        line_id = np.stack([lay, k], axis=1)
        new = np.concatenate([[True], (line_id[1:] != line_id[:-1]).any(axis=1)])
        out.line_counts = np.diff(np.concatenate([np.flatnonzero(new), [n]]))
        out.line_ids = line_id[new]
    else:
        t = uc = np.zeros(0)
        xc = yc = np.zeros(0, F)
        lay = np.zeros(0, np.int64)
        out.line_counts = np.zeros(0, np.int64)
        out.line_ids = np.zeros((0, 2), np.int64)
    out.t = t
    out.records = (lay, k, uc, j)                       # every crossing's layer, line, u_c and tail vertex, in sorted order
    assert (out.line_counts % 2 == 0).all(), "a line with an odd number of crossings"
    # even counts on every line: the pairs of the whole sorted list are the pairs of the lines
    out.seg = np.stack([xc[0::2], yc[0::2], xc[1::2], yc[1::2]], axis=1).astype(F).reshape(-1, 4)
    out.line = k[0::2].astype(np.int32)
    seg_layer = lay[0::2]
    out.layer_start = np.searchsorted(seg_layer, np.arange(L + 1)).astype(np.uint32)
    q = S.quantised(uc[1::2] - uc[0::2], math.ldexp(1.0, 58 - e)) if n else []
    out.layers = np.zeros(L, LAYER_DTYPE)
    total = 0
    slots = 0
    for l in range(L):
        s0, s1 = int(out.layer_start[l]), int(out.layer_start[l + 1])
        sm = sum(q[s0:s1])
        total += sm
        ks = out.line[s0:s1]
        out.layers[l] = (math.ldexp(float(sm), e - 58), s1 - s0, int(ks.min()) if s1 > s0 else 0, int(ks.max()) if s1 > s0 else -1)
        slots += int(ks.max()) - int(ks.min()) + 1 if s1 > s0 else 0
    if slots >= 1 << 31:
        raise OverflowError("2^31 line slots or more")
    b = out.seg.view(np.uint32)
    out.stats = {"n_segments": n // 2, "n_crossings": n, "n_lines": len(out.line_counts), "max_line_crossings": int(out.line_counts.max()) if n else 0,
                 "zero_length": int(((b[:, 0] == b[:, 2]) & (b[:, 1] == b[:, 3])).sum()), "n_layers": L, "length": math.ldexp(float(total), e - 58)}
    return out


# ---- what the tests of the twin and of the device share ------------------------------------------------------------------------
def annulus(n_out=90, n_in=40, r_out=10.0, r_in=4.0, cx=3.0, cy=-2.0):
    """An outer circle (counter-clockwise) and a hole (clockwise): properly nested."""
    return [S.circle(n_out, r_out, cx, cy), S.circle(n_in, r_in, cx, cy)[::-1].copy()]


def hand_loops():
    """Five layers, layer 3 empty: an annulus, the lattice rectangle (37, 41) of the simplification's tests, a triangle inside a
    square hole inside a square; a rectangle and an annulus again."""
    sq = lambda a, c=0.0: np.array([(c - a, c - a), (c + a, c - a), (c + a, c + a), (c - a, c + a)], F)  # noqa: E731
    tri = np.array([(-1, -1), (1.5, -0.5), (0, 1.25)], F)
    loops = annulus() + [S.rectangle(37, 41)] + [sq(8), sq(4)[::-1].copy(), tri] + [S.rectangle(5, 3, 0.5)] + annulus(31, 17, 6.0, 2.5, -1.0, 0.5)
    return S.pack(loops, [0, 0, 1, 2, 2, 2, 4, 4, 4], 5)


def comb(teeth=400, w=0.5, h=3.0):
    """Thin rectangles in a row, each touching the next: a horizontal line crosses 2 x teeth edges, and where two teeth touch the two
    crossings have the same u_c (the tail's vertex number decides)."""
    return S.pack([np.array([(i * w, 0), ((i + 1) * w, 0), ((i + 1) * w, h), (i * w, h)], F) for i in range(teeth)])


def inside_even_odd(p, loops):
    """Even-odd point-in-polygon of the points p (m, 2) against closed loops, plain float64 ray casting along +x (independent of the
    hatch's arithmetic)."""
    p = np.asarray(p, np.float64)
    odd = np.zeros(len(p), bool)
    for l in loops:
        a = np.asarray(l, np.float64)
        b = np.roll(a, -1, axis=0)
        for (ax, ay), (bx, by) in zip(a, b):
            if ay == by:
                continue
            straddle = (ay <= p[:, 1]) != (by <= p[:, 1])
            with np.errstate(all="ignore"):
                x_at = ax + (p[:, 1] - ay) / (by - ay) * (bx - ax)
            odd ^= straddle & (p[:, 0] < x_at)
    return odd
