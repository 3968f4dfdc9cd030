"""CPU twin of one UI frame (include/gsdf_hip.h: gsdf_view; gsdfaux/ui.go:247-355): the contract's float32 arithmetic in numpy,
operation for operation -- every product, sum, square root and division one float32 operation, sums left to right as the shader
writes them -- over a distance function such as OracleSDF.Evaluate. The device kernel (gsdf_amd/csrc/kernels_view.h) must give
the same bytes, depth bits and evaluation counts.

The samples of a pixel run in the contract's order (m outer, n inner) and, for a hit, the four normal taps in theirs; each march
step evaluates the rays still marching in one batch. Per pixel the twin also records whether its march met a non-finite distance
(`nonfinite`): there the evaluator is held to the oracle only where the oracle's distance is finite (tests/test_gpu_nan.py).
"""
import numpy as np

F = np.float32
TOL = F(1e-4)
E = F(0.5773)
K = F(E * F(1e-4))
LIGHT = F(0.57703)


def _clamp01(x):
    return np.where(np.isnan(x), F(0), np.minimum(np.maximum(x, F(0)), F(1))).astype(F)


def _normalize(x, y, z):
    n = np.sqrt((x * x + y * y) + z * z)
    return x / n, y / n, z / n


def render(sdf, view, w, h):
    """sdf: (n,3) float32 -> (n,) float32; view: a gsdf_view (gsdf_amd.hip.GsdfView). Returns a dict of rgba (h,w,4) uint8,
    depth (h,w) float32, evals (h,w) uint32, nonfinite (h,w) bool and normal (h,w,3) float32 (the last hitting sample's, NaN
    where none hit), rows from the top."""
    ro = np.array(view.ro[:], F)
    uu, vv, ww = np.array(view.uu[:], F), np.array(view.vv[:], F), np.array(view.ww[:], F)
    aa, max_steps = int(view.aa), int(view.max_steps)
    tmax = F(F(1.3) * F(view.char_dist))
    n = w * h
    r, i = np.divmod(np.arange(n), w)
    fx = i.astype(F) + F(0.5)
    fy = (h - 1 - r).astype(F) + F(0.5)  # output row r is GL row h - 1 - r
    fw, fh, fa = F(w), F(h), F(aa)
    tot = np.zeros((3, n), F)
    depth = np.full(n, np.inf, F)
    evals = np.zeros(n, np.int64)
    nonfinite = np.zeros(n, bool)
    normal = np.full((3, n), np.nan, F)

    def evaluate(x, y, z):
        d = np.asarray(sdf(np.ascontiguousarray(np.stack([x, y, z], axis=1), F)), F)
        return d

    for m in range(aa):
        for nn in range(aa):
            ox, oy = F(F(m) / fa) - F(0.5), F(F(nn) / fa) - F(0.5)
            px = (F(2) * (fx + ox) - fw) / fh
            py = (F(2) * (fy + oy) - fh) / fh
            rx, ry, rz = _normalize((px * uu[0] + py * vv[0]) + F(1.5) * ww[0],
                                    (px * uu[1] + py * vv[1]) + F(1.5) * ww[1],
                                    (px * uu[2] + py * vv[2]) + F(1.5) * ww[2])
            t = np.zeros(n, F)
            steps = np.zeros(n, np.int64)
            hit = np.zeros(n, bool)
            live = np.arange(n)
            for _ in range(max_steps):
                if live.size == 0:
                    break
                tl = t[live]
                d = evaluate(ro[0] + tl * rx[live], ro[1] + tl * ry[live], ro[2] + tl * rz[live])
                steps[live] += 1
                nonfinite[live] |= ~np.isfinite(d)
                h_ok = d < TOL
                stop = h_ok | (tl > tmax)
                hit[live[h_ok]] = True
                go = ~stop
                t[live[go]] = tl[go] + d[go]
                live = live[go]
            hid = np.nonzero(hit)[0]
            evals += steps + 4 * hit
            if hid.size == 0:
                continue
            th = t[hid]
            hx, hy, hz = ro[0] + th * rx[hid], ro[1] + th * ry[hid], ro[2] + th * rz[hid]
            taps = [evaluate(hx + K, hy - K, hz - K), evaluate(hx - K, hy - K, hz + K),
                    evaluate(hx - K, hy + K, hz - K), evaluate(hx + K, hy + K, hz + K)]
            for d in taps:
                nonfinite[hid] |= ~np.isfinite(d)
            d0, d1, d2, d3 = taps
            nx = ((E * d0 + -E * d1) + -E * d2) + E * d3
            ny = ((-E * d0 + -E * d1) + E * d2) + E * d3
            nz = ((-E * d0 + E * d1) + -E * d2) + E * d3
            ux, uy, uz = _normalize(nx, ny, nz)
            dif = _clamp01((ux * LIGHT + uy * LIGHT) + uz * LIGHT)
            amb = F(0.5) + F(0.5) * uy
            tot[0, hid] = tot[0, hid] + np.sqrt(F(0.2) * amb + F(0.8) * dif)
            tot[1, hid] = tot[1, hid] + np.sqrt(F(0.3) * amb + F(0.7) * dif)
            tot[2, hid] = tot[2, hid] + np.sqrt(F(0.4) * amb + F(0.5) * dif)
            closer = th < depth[hid]
            depth[hid[closer]] = th[closer]
            normal[:, hid] = np.stack([ux, uy, uz])
    fs = F(aa * aa)
    rgba = np.full((n, 4), 255, np.uint8)
    for c in range(3):
        rgba[:, c] = (_clamp01(tot[c] / fs) * F(255) + F(0.5)).astype(np.uint8)
    return {"rgba": rgba.reshape(h, w, 4), "depth": depth.reshape(h, w), "evals": evals.astype(np.uint32).reshape(h, w),
            "nonfinite": nonfinite.reshape(h, w), "normal": normal.T.reshape(h, w, 3)}


class CountingSDF:
    """A distance function that counts the points it was asked for (the twin's own evaluation count)."""

    def __init__(self, fn):
        self.fn, self.count = fn, 0

    def __call__(self, pos):
        self.count += pos.shape[0]
        return self.fn(pos)
