"""CPU twin of the loops' simplification and measures (include/gsdf_hip.h, section "contours: simplify and measures"), written from
that contract: numpy float64 for q2 (numpy's elementwise operations are single IEEE operations, never fused), Python integers for the
measures' sums. One numpy pass per level over all loops at once, so that a loop of 200 000 vertices takes seconds. What the device
must equal, to the byte."""
import math

import numpy as np

F = np.float32
MAX_LEVELS = 16
LOOP_DTYPE = np.dtype([("area", "<f8"), ("length", "<f8"), ("bbox", "<f4", (4,)), ("n_verts", "<u4"), ("layer", "<u4")])
LAYER_DTYPE = np.dtype([("area", "<f8"), ("length", "<f8"), ("bbox", "<f4", (4,)), ("n_loops", "<u4"), ("n_verts", "<u4")])


class Loops:
    """xy (n, 2) float32, keys n uint32, loop_start n_loops + 1 uint32, loop_layer n_loops uint32, n_layers."""

    def __init__(self, xy, loop_start, loop_layer=None, n_layers=1, keys=None):
        self.xy = np.ascontiguousarray(xy, F).reshape(-1, 2)
        self.loop_start = np.ascontiguousarray(loop_start, np.uint32)
        nl = len(self.loop_start) - 1
        self.loop_layer = np.zeros(nl, np.uint32) if loop_layer is None else np.ascontiguousarray(loop_layer, np.uint32)
        self.keys = np.zeros(len(self.xy), np.uint32) if keys is None else np.ascontiguousarray(keys, np.uint32)
        self.n_layers = int(n_layers)

    @classmethod
    def of(cls, c, n_layers=None):
        """From anything with xy / keys / loop_start / loop_layer (contourref.Contour, hip.ContourHIP)."""
        nl = n_layers if n_layers is not None else (c.n_layers if hasattr(c, "n_layers") else c.stats["n_layers"])
        return cls(c.xy, c.loop_start, c.loop_layer, nl, c.keys)

    def loops(self):
        return [self.xy[self.loop_start[q]:self.loop_start[q + 1]] for q in range(len(self.loop_layer))]


def kmax_of(n, levels):
    """The largest k <= levels with 3 2^k <= n."""
    k = 0
    while k < levels and 3 * (2 << k) <= n:
        k += 1
    return k


def q2(ax, ay, bx, by, px, py):
    """The contract's squared point-to-segment distance, elementwise over float64 arrays, operation by operation."""
    with np.errstate(all="ignore"):
        ux, uy = bx - ax, by - ay
        dd = ux * ux + uy * uy
        wx, wy = px - ax, py - ay
        t = wx * ux + wy * uy
        near_a = wx * wx + wy * wy
        vx, vy = px - bx, py - by
        near_b = vx * vx + vy * vy
        cr = wx * uy - wy * ux
        mid = (cr * cr) / dd
        return np.where((dd == 0) | (t <= 0), near_a, np.where(t >= dd, near_b, mid))


def one_pass(xy, loop_start, tol2, levels):
    """-> keep (bool per vertex), spans (17 counts of maximal acceptable spans), the largest q2 of a dropped vertex against its maximal
    span (0.0 if none), the loops that lost a vertex (bool per loop)."""
    P = np.asarray(xy, F).astype(np.float64)
    ls = np.asarray(loop_start, np.int64)
    n_of = np.diff(ls)
    V = len(P)
    q = np.repeat(np.arange(len(n_of)), n_of)
    l0, n = ls[:-1][q], n_of[q]
    j = np.arange(V, dtype=np.int64) - l0
    km = np.array([kmax_of(int(x), levels) for x in n_of], np.int64)[q]
    top = np.zeros(V, np.int64)
    top_q2 = np.zeros(V, np.float64)
    top_s = np.zeros(V, np.int64)
    for k in range(1, MAX_LEVELS + 1):
        w = 1 << k
        interior = (k <= km) & (j % w != 0)
        if not interior.any():
            continue
        s = j - j % w
        e = np.minimum(s + w, n)
        a, b = l0 + s, l0 + np.where(e == n, 0, e)
        d = q2(P[a, 0], P[a, 1], P[b, 0], P[b, 1], P[:, 0], P[:, 1])
        beyond = interior & ~(d <= tol2)
        rejected = np.zeros(V, bool)  # by the span's first vertex
        rejected[a[beyond]] = True
        ok = interior & ~rejected[a]
        top[ok] = k
        top_q2[ok] = d[ok]
        top_s[ok] = s[ok]
    dropped = top > 0
    first = dropped & (j == top_s + 1)
    spans = np.bincount(top[first], minlength=MAX_LEVELS + 1).astype(np.int64)
    changed = np.zeros(len(n_of), bool)
    changed[q[dropped]] = True
    return ~dropped, spans, float(top_q2[dropped].max()) if dropped.any() else 0.0, changed


def simplify(c, tol, levels=8, passes=1):
    """The twin of gsdf_hip_contour_simplify: (Loops, stats dict with the leading block's fields)."""
    if not (F(tol) >= 0) or not 0 <= levels <= MAX_LEVELS or not 0 <= passes <= 8:
        raise ValueError("bad argument")
    levels, passes = levels or 8, passes or 1
    tol2 = float(F(tol)) * float(F(tol)) if np.isfinite(F(tol)) else math.inf
    xy, keys, ls = c.xy, c.keys, c.loop_start
    spans = np.zeros(MAX_LEVELS + 1, np.int64)
    worst, changed_total = 0.0, 0
    for _ in range(passes):
        keep, sp, w2, changed = one_pass(xy, ls, tol2, levels)
        spans += sp
        worst = max(worst, w2)
        changed_total += int(changed.sum())
        kept_before = np.concatenate([[0], np.cumsum(keep)])
        ls = kept_before[np.asarray(ls, np.int64)].astype(np.uint32)
        xy, keys = xy[keep], keys[keep]
    out = Loops(xy, ls, c.loop_layer, c.n_layers, keys)
    st = {"n_verts_in": len(c.xy), "n_verts_out": len(xy), "n_loops": len(c.loop_layer), "loops_changed": changed_total,
          "spans": [int(x) for x in spans], "max_level": max([k for k in range(MAX_LEVELS + 1) if spans[k]], default=0),
          "max_dev": math.sqrt(worst)}
    return out, st


# ---- measures ----------------------------------------------------------------------------------------------------------------------
def exponent(xy):
    bits = np.ascontiguousarray(xy, F).view(np.uint32).ravel() & np.uint32(0x7fffffff)
    bits = bits[bits < 0x7f800000]
    m = int(bits.max()) if len(bits) else 0
    return max(m >> 23, 1) - 126


def ordered(f32):
    b = np.ascontiguousarray(f32, F).view(np.uint32).astype(np.uint64)
    return np.where(b >> 31 != 0, b ^ 0xffffffff, b ^ 0x80000000).astype(np.uint32)


def unordered(o):
    o = np.asarray(o, np.uint32).astype(np.uint64)
    return np.where(o >> 31 != 0, o ^ 0x80000000, o ^ 0xffffffff).astype(np.uint32).view(F)


def quantised(term, scale):
    """round-to-nearest-even of term * scale, as Python integers (|q| <= 2^62: exact in int64)."""
    return [int(x) for x in np.rint(term * scale).astype(np.int64)]


def measures(c):
    """The twin of gsdf_hip_contour_measures: (loops, layers) records."""
    P = c.xy.astype(np.float64)
    ls = np.asarray(c.loop_start, np.int64)
    nl = len(c.loop_layer)
    e = exponent(c.xy)
    loops = np.zeros(nl, LOOP_DTYPE)
    layers = np.zeros(c.n_layers, LAYER_DTYPE)
    lay_area, lay_len = [0] * c.n_layers, [0] * c.n_layers
    lay_box = np.tile(np.array([0xff800000, 0xff800000, 0x007fffff, 0x007fffff], np.uint32), (c.n_layers, 1))
    if len(P):
        nxt = np.arange(1, len(P) + 1, dtype=np.int64)
        nxt[ls[1:] - 1] = ls[:-1]
        x0, y0, x1, y1 = P[:, 0], P[:, 1], P[nxt, 0], P[nxt, 1]
        a = x0 * y1 - x1 * y0
        dx, dy = x1 - x0, y1 - y0
        ln = np.sqrt(dx * dx + dy * dy)
        qa, ql = quantised(a, math.ldexp(1.0, 61 - 2 * e)), quantised(ln, math.ldexp(1.0, 60 - e))
        ob = ordered(c.xy)  # (n, 2)
    for k in range(nl):
        s0, s1, lay = int(ls[k]), int(ls[k + 1]), int(c.loop_layer[k])
        sa, sl = sum(qa[s0:s1]), sum(ql[s0:s1])
        box = np.array([ob[s0:s1, 0].min(), ob[s0:s1, 1].min(), ob[s0:s1, 0].max(), ob[s0:s1, 1].max()], np.uint32)
        loops[k] = (math.ldexp(float(sa), 2 * e - 62), math.ldexp(float(sl), e - 60), unordered(box), s1 - s0, lay)
        lay_area[lay] += sa
        lay_len[lay] += sl
        lay_box[lay, :2] = np.minimum(lay_box[lay, :2], box[:2])
        lay_box[lay, 2:] = np.maximum(lay_box[lay, 2:], box[2:])
        layers[lay]["n_loops"] += 1
        layers[lay]["n_verts"] += s1 - s0
    for lay in range(c.n_layers):
        layers[lay]["area"] = math.ldexp(float(lay_area[lay]), 2 * e - 62)
        layers[lay]["length"] = math.ldexp(float(lay_len[lay]), e - 60)
        layers[lay]["bbox"] = unordered(lay_box[lay])
    return loops, layers


# ---- what the tests of the twin and of the device share ------------------------------------------------------------------------
def seg_dist(p, a, b):
    """Distance of every point p (m, 2) to the nearest of the segments a[i] b[i] (k, 2), plain float64 geometry (not the contract's q2)."""
    p, a, b = (np.asarray(v, np.float64) for v in (p, a, b))
    out = np.empty(len(p))
    u = b - a
    dd = (u * u).sum(axis=1)
    for i0 in range(0, len(p), 512):
        w = p[i0:i0 + 512, None, :] - a[None, :, :]
        with np.errstate(all="ignore"):
            t = np.clip(np.where(dd > 0, (w * u[None]).sum(axis=2) / dd, 0.0), 0.0, 1.0)
        d = w - t[..., None] * u[None]
        out[i0:i0 + 512] = np.sqrt((d * d).sum(axis=2)).min(axis=1)
    return out


def hausdorff(old, new, samples=(0.25, 0.5, 0.75)):
    """Both directed distances between two closed polygons (vertices and a few points along every edge against the other's edges)."""
    def pts(l):
        l = np.asarray(l, np.float64)
        n = np.roll(l, -1, axis=0)
        return np.concatenate([l] + [l + t * (n - l) for t in samples])
    old, new = np.asarray(old, np.float64), np.asarray(new, np.float64)
    return (float(seg_dist(pts(old), new, np.roll(new, -1, axis=0)).max()), float(seg_dist(pts(new), old, np.roll(old, -1, axis=0)).max()))


def circle(n, r=10.0, cx=3.0, cy=-2.0):
    """n vertices on a circle, counter-clockwise, float32."""
    th = (np.arange(n, dtype=np.float64) * (2 * math.pi / n))
    return np.stack([cx + r * np.cos(th), cy + r * np.sin(th)], axis=1).astype(F)


def rectangle(nx, ny, step=0.125):
    """A rectangle whose sides carry lattice-like collinear vertices: nx per horizontal side, ny per vertical one; counter-clockwise."""
    xs, ys = np.arange(nx) * step, np.arange(ny) * step
    w, h = nx * step, ny * step
    pts = [(x, 0.0) for x in xs] + [(w, y) for y in ys] + [(w - x, h) for x in xs] + [(0.0, h - y) for y in ys]
    return np.array(pts, F)


def pack(loops, layers=None, n_layers=None):
    """Several (n, 2) arrays -> Loops."""
    ls = np.concatenate([[0], np.cumsum([len(l) for l in loops])]).astype(np.uint32)
    lay = np.zeros(len(loops), np.uint32) if layers is None else np.asarray(layers, np.uint32)
    nl = n_layers if n_layers is not None else (int(lay.max()) + 1 if len(lay) else 1)
    xy = np.concatenate([np.asarray(l, F).reshape(-1, 2) for l in loops])
    return Loops(xy, ls, lay, nl, np.arange(len(xy), dtype=np.uint32) * np.uint32(7) + np.uint32(1))


def mixed_loops(n_loops=3000, n_layers=5, seed=7):
    """Small loops of mixed sizes (3 .. 80 vertices: circles with noise, some rectangles) in several layers."""
    rng = np.random.default_rng(seed)
    loops = []
    for i in range(n_loops):
        n = int(rng.integers(3, 81))
        if i % 5 == 0 and n >= 8:
            l = rectangle(n // 4 + 1, n // 4, 0.25) + F(rng.uniform(-50, 50))
        else:
            l = circle(n, rng.uniform(0.5, 5.0), rng.uniform(-50, 50), rng.uniform(-50, 50))
            l = (l + rng.normal(0, 0.01, l.shape)).astype(F)
        loops.append(l)
    layers = np.sort(rng.integers(0, n_layers, n_loops)).astype(np.uint32)
    return pack(loops, layers, n_layers)
