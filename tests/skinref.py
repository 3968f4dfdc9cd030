"""CPU twin of the skin classification of the hatch (include/gsdf_hip.h, section "contours: skin classification of the hatch"),
written from that contract on top of hatchref's: numpy float64 elementwise operations (single IEEE operations, never fused) over
edges x candidate lines for every source layer, Python integers for the length sums. What the device must equal, to the byte."""
import math

import numpy as np

import contoursimpref as S
import hatchref as H

F = np.float32
OUTSIDE = 4
SKIN_LAYER_DTYPE = np.dtype([("length", "<f8", (4,)), ("n_segments", "<u8", (4,))])
STATS_FIELDS = ("n_segments", "n_crossings", "n_own_crossings", "n_lines", "max_line_crossings", "zero_length", "n_class", "length", "n_layers", "below", "above")


class Skin(H.Hatch):
    """A Hatch (seg, line, layer_start, layers: the layers' totals) with cls n uint8, skin_layers SKIN_LAYER_DTYPE records and the
    stats of gsdf_skin_stats before ms_device; start_u / end_u: every piece's two values, records: the sorted crossings (what the tests
    of the twin look at)."""


def classes_of(mask, below, above):
    """The class of every source mask (bit r: source r is present): OUTSIDE, or bit 0 bottom | bit 1 top."""
    mask = np.asarray(mask, np.int64)
    need_b = ((1 << below) - 1) << 1
    need_a = ((1 << above) - 1) << (1 + below)
    c = ((mask & need_b) != need_b).astype(np.int64) | (((mask & need_a) != need_a).astype(np.int64) << 1)
    return np.where(mask & 1, c, OUTSIDE)


def skin(c, spacing, dirs, below, above, offset=0.0):
    """The twin of gsdf_hip_contour_hatch_skin on a contoursimpref.Loops (or anything with its fields)."""
    sp, off, dirs, e = H.check_arguments(c, spacing, dirs, offset)
    if not (0 <= below <= 8 and 0 <= above <= 8):
        raise ValueError("below and above must be 0 .. 8")
    L = int(c.n_layers)
    P = np.asarray(c.xy, F).astype(np.float64).reshape(-1, 2)
    ls = np.asarray(c.loop_start, np.int64)
    V = len(P)
    if V * (1 + below + above) >= 1 << 32:
        raise OverflowError("2^32 (edge, source) pairs or more")
    cols = {f: [] for f in ("lay", "k", "r", "j", "uc", "xc", "yc")}
    if V:
        nxt = np.arange(1, V + 1, dtype=np.int64)
        nxt[ls[1:] - 1] = ls[:-1]
        layer_v = np.repeat(np.asarray(c.loop_layer, np.int64), np.diff(ls))
        xa, ya, xb, yb = P[:, 0], P[:, 1], P[nxt, 0], P[nxt, 1]
        for r in range(1 + below + above):
            # the edges of layer m are source r of target layer l
            target = layer_v + (0 if r == 0 else (r if r <= below else -(r - below)))
            ok = np.flatnonzero((target >= 0) & (target < L))
            if not len(ok):
                continue
            d = dirs[target[ok] % len(dirs)]
            dx, dy = d[:, 0], d[:, 1]
            sa, sb = ((-dy) * xa[ok]) + (dx * ya[ok]), ((-dy) * xb[ok]) + (dx * yb[ok])
            ua, ub = (dx * xa[ok]) + (dy * ya[ok]), (dx * xb[ok]) + (dy * yb[ok])
            lo, hi = np.minimum(sa, sb), np.maximum(sa, sb)
            k0 = np.floor((lo - off) / sp).astype(np.int64) - 2
            k1 = np.floor((hi - off) / sp).astype(np.int64) + 2
            n_c = k1 - k0 + 1
            first = np.concatenate([[0], np.cumsum(n_c)])
            i = np.repeat(np.arange(len(ok), dtype=np.int64), n_c)
            k = k0[i] + (np.arange(first[-1], dtype=np.int64) - first[:-1][i])
            ck = off + (k.astype(np.float64) * sp)
            crossed = (sa[i] < ck) != (sb[i] < ck)
            assert not crossed[(k <= k0[i] + 1) | (k >= k1[i] - 1)].any(), "the candidate range is too narrow"
            i, k, ck = i[crossed], k[crossed], ck[crossed]
            if not len(i):
                continue
            j = ok[i]
            with np.errstate(all="raise"):
                t = (ck - sa[i]) / (sb[i] - sa[i])
            cols["uc"].append(ua[i] + (t * (ub[i] - ua[i])))
            cols["xc"].append((xa[j] + (t * (xb[j] - xa[j]))).astype(F))
            cols["yc"].append((ya[j] + (t * (yb[j] - ya[j]))).astype(F))
            cols["lay"].append(target[j])
            cols["k"].append(k)
            cols["r"].append(np.full(len(j), r, np.int64))
            cols["j"].append(j)
    cat = lambda f, dt: np.concatenate(cols[f]) if cols[f] else np.zeros(0, dt)  # noqa: E731
    lay, k, r, j, uc = cat("lay", np.int64), cat("k", np.int64), cat("r", np.int64), cat("j", np.int64), cat("uc", np.float64)
    xc, yc = cat("xc", F), cat("yc", F)
    # lines that count: those with a crossing of source 0
    line_key = lay * (1 << 32) + (k + (1 << 31))
    keep = np.isin(line_key, np.unique(line_key[r == 0]))
    lay, k, r, j, uc, xc, yc, line_key = (a[keep] for a in (lay, k, r, j, uc, xc, yc, line_key))
    n = len(j)
    if n >= 1 << 32:
        raise OverflowError("2^32 crossings or more")
    order = np.lexsort((j, r, uc, line_key))  # (the last key is the first to decide; -0.0 and 0.0 compare equal)
    lay, k, r, j, uc, xc, yc, line_key = (a[order] for a in (lay, k, r, j, uc, xc, yc, line_key))
    out = Skin()
    out.exponent = e
    out.records = (line_key, uc, r, j, xc, yc)          # every crossing's line, u_c, source, tail vertex and point, in sorted order
    if n:
        new_line = np.concatenate([[True], line_key[1:] != line_key[:-1]])
        new_value = new_line | np.concatenate([[True], uc[1:] != uc[:-1]])
        line_counts = np.diff(np.concatenate([np.flatnonzero(new_line), [n]]))
        # the sources' parity after every record; every source crosses a line an even number of times, so it is 0 where a line ends
        mask = np.bitwise_xor.accumulate(np.int64(1) << r)
        assert (mask[np.concatenate([np.flatnonzero(new_line)[1:] - 1, [n - 1]])] == 0).all(), "a line with an odd number of crossings of one source"
        lead = np.flatnonzero(new_value)                          # the first crossing of every value under (r, j)
        last = np.concatenate([lead[1:] - 1, [n - 1]])
        after = classes_of(mask[last], below, above)              # the class of the gap behind every value
        before = np.concatenate([[OUTSIDE], after[:-1]])          # (a line starts OUTSIDE because the one before it ends so)
        bnd = np.flatnonzero(after != before)
        piece = np.flatnonzero(after[bnd] != OUTSIDE)
        assert not len(piece) or piece[-1] + 1 < len(bnd), "the last line does not end outside"
        start, end = lead[bnd[piece]], lead[bnd[piece + 1]]       # a piece runs to the next boundary, which is of its line
        assert (line_key[start] == line_key[end]).all(), "a line that does not end outside"
        cls = after[bnd[piece]]
    else:
        line_counts = np.zeros(0, np.int64)
        start = end = cls = np.zeros(0, np.int64)
    out.line_counts = line_counts
    out.seg = np.stack([xc[start], yc[start], xc[end], yc[end]], axis=1).astype(F).reshape(-1, 4)
    out.line = k[start].astype(np.int32)
    out.cls = cls.astype(np.uint8)
    out.start_u, out.end_u = uc[start], uc[end]
    out.layer_start = np.searchsorted(lay[start], np.arange(L + 1)).astype(np.uint32)
    q = S.quantised(uc[end] - uc[start], math.ldexp(1.0, 58 - e)) if len(start) else []
    out.layers = np.zeros(L, H.LAYER_DTYPE)
    out.skin_layers = np.zeros(L, SKIN_LAYER_DTYPE)
    total = [0, 0, 0, 0]
    for l in range(L):
        s0, s1 = int(out.layer_start[l]), int(out.layer_start[l + 1])
        sums, counts = [0, 0, 0, 0], [0, 0, 0, 0]
        for i in range(s0, s1):
            sums[cls[i]] += q[i]
            counts[cls[i]] += 1
        for a in range(4):
            total[a] += sums[a]
            out.skin_layers[l]["length"][a] = math.ldexp(float(sums[a]), e - 58)
            out.skin_layers[l]["n_segments"][a] = counts[a]
        ks = out.line[s0:s1]
        out.layers[l] = (math.ldexp(float(sum(sums)), e - 58), s1 - s0, int(ks.min()) if s1 > s0 else 0, int(ks.max()) if s1 > s0 else -1)
    b = out.seg.view(np.uint32)
    out.stats = {"n_segments": len(start), "n_crossings": n, "n_own_crossings": int((r == 0).sum()), "n_lines": len(line_counts),
                 "max_line_crossings": int(line_counts.max()) if n else 0, "zero_length": int(((b[:, 0] == b[:, 2]) & (b[:, 1] == b[:, 3])).sum()),
                 "n_class": [int((cls == a).sum()) for a in range(4)], "length": [math.ldexp(float(t), e - 58) for t in total],
                 "n_layers": L, "below": below, "above": above}
    return out


# ---- what the tests of the twin and of the device share ------------------------------------------------------------------------
def square(a, cx=0.0, cy=0.0):
    """The square of half side a about (cx, cy), counter-clockwise."""
    return np.array([(cx - a, cy - a), (cx + a, cy - a), (cx + a, cy + a), (cx - a, cy + a)], F)


def square_stack():
    """Seven layers of one square each: two equal layers, a shrink, a shrink again, a shifted growth and two equal layers."""
    return S.pack([square(5), square(5), square(3.5), square(2.25), square(4, 1.5, -0.75), square(3, 0.25, 0.5), square(3, 0.25, 0.5)], list(range(7)), 7)


def pyramid():
    """An 8 x 8 square at layer 0 under a 4 x 4 square at layer 1, both centred at (4, 4)."""
    return S.pack([square(4, 4, 4), square(2, 4, 4)], [0, 1], 2)


def shifted_combs(teeth=400, w=0.5):
    """hatchref.comb in three layers, each shifted by one tooth width: the layers' crossings tie at every tooth."""
    one = H.comb(teeth, w)
    loops, layers = [], []
    for l in range(3):
        loops += [p + np.array([l * w, 0], F) for p in one.loops()]
        layers += [l] * teeth
    return S.pack(loops, layers, 3)
