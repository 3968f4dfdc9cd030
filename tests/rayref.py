"""A numpy twin of the RAYS contract (include/gsdf_hip.h, "rays"): raycast() is gsdf_hip_raycast3 -- (a distance function, origins,
directions, the options) in; t, d, the status bytes, the evaluations per ray and the stats' leading block out -- and thickness() is
gsdf_hip_indexed_thickness -- the same march along the inward normal of every vertex. Nothing here looks at a device result.

Every product, sum, difference, division and square root is one float32 numpy operation in the contract's order; the comparisons are
numpy's IEEE ones (false on NaN) under `NOT`, as the contract writes them. Per trip only the rays still live are evaluated (like
projectref.project), so a counting distance function sees exactly st["evals"] points."""
import struct

import numpy as np

from projectref import CountingSDF  # noqa: F401  (the tests' counting distance function)

F = np.float32
SKIPPED, HIT, CROSSED, MISS, STEPS, NONFINITE, FLAT = range(7)
STATUS = ["SKIPPED", "HIT", "CROSSED", "MISS", "STEPS", "NONFINITE", "FLAT"]
NOT_EVALUATED = np.array([0x7fc00000], np.uint32).view(F)[0]
BAD_ARGUMENT, DIMENSION, EMPTY_BUFFERS, CAPACITY = -3, -7, -1, -10
RESULT_BYTES = 104


class RayError(Exception):
    """code: the GSDF_ERR_* the device returns for the same options."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def check_opts(t0=0.0, tmax=np.inf, tol=1e-4, min_step=0.0, max_steps=256, refine=8, flags=0):
    t0, tmax, tol, min_step = F(t0), F(tmax), F(tol), F(min_step)
    if not (np.isfinite(t0) and t0 >= 0):
        raise RayError(BAD_ARGUMENT, "t0")
    if not tmax >= t0:
        raise RayError(BAD_ARGUMENT, "tmax")
    if not (np.isfinite(tol) and tol >= 0):
        raise RayError(BAD_ARGUMENT, "tol")
    if not (np.isfinite(min_step) and min_step >= 0):
        raise RayError(BAD_ARGUMENT, "min_step")
    if not 1 <= int(max_steps) <= 4096:
        raise RayError(BAD_ARGUMENT, "max_steps")
    if not 0 <= int(refine) <= 32:
        raise RayError(BAD_ARGUMENT, "refine")
    if flags != 0:
        raise RayError(BAD_ARGUMENT, "flags")
    return F(t0 + F(0)), tmax, tol, min_step, int(max_steps), int(refine)   # (a t0 of -0 is taken as +0)


def stats_bytes(st):
    """The leading block of gsdf_ray_stats (104 bytes)."""
    return struct.pack("<10QI2fIQ", int(st["n"]), *[int(c) for c in st["count"]], int(st["evals"]), int(st["steps_max"]), float(st["t_min"]),
                       float(st["t_max"]), 0, int(st["below"]))


def _march(sdf, o, r, takes_part, status, t0, tmax, tol, min_step, max_steps, refine):
    """Steps 2 .. 4 for the rays takes_part marks (the others keep `status`). Returns t, d, status, march and refine evaluations."""
    n = len(o)
    nan = np.full(n, NOT_EVALUATED, F)
    t, d = nan.copy(), nan.copy()
    nmarch, nref = np.zeros(n, np.int64), np.zeros(n, np.int64)
    inside = np.zeros(n, bool)
    a, b, db = np.zeros(n, F), np.zeros(n, F), np.zeros(n, F)

    def evaluate(idx, tt):
        tt = tt.astype(F)[:, None]
        pos = (o[idx] + (tt * r[idx]).astype(F)).astype(F)
        return np.asarray(sdf(np.ascontiguousarray(pos, F)), F).reshape(-1)

    with np.errstate(all="ignore"):
        live = np.flatnonzero(takes_part)
        te = np.full(n, t0, F)
        crossed = []
        first = True
        while live.size:                                                    # 2. and 3.: one march evaluation per trip
            dv = evaluate(live, te[live])
            nmarch[live] += 1
            nonfin = np.isnan(dv)
            hit = ~nonfin & ~(np.abs(dv) > tol)
            if first:
                inside[live] = np.signbit(dv)
            cross = ~nonfin & ~hit & (np.signbit(dv) != inside[live])
            go = ~(nonfin | hit | cross)
            out_of_steps = go & (nmarch[live] >= max_steps)
            status[live[nonfin]], t[live[nonfin]], d[live[nonfin]] = NONFINITE, te[live[nonfin]], NOT_EVALUATED
            for m, code in ((hit, HIT), (out_of_steps, STEPS)):
                status[live[m]], t[live[m]], d[live[m]] = code, te[live[m]], dv[m]
            c = live[cross]
            status[c], a[c], b[c], db[c] = CROSSED, t[c], te[c], dv[cross]  # (t: the point before, tp)
            crossed.append(c)
            go &= ~out_of_steps
            live, dv = live[go], dv[go]
            t[live], d[live] = te[live], dv                                 # tp, dp
            s = np.abs(dv)
            s = np.where(s < min_step, min_step, s).astype(F)
            tn = (t[live] + s).astype(F)
            miss = tn > tmax
            status[live[miss]] = MISS
            live, tn = live[~miss], tn[~miss]
            te[live] = tn
            first = False
        live = np.concatenate(crossed) if crossed else live                 # 4.
        t[live], d[live] = b[live], db[live]
        for _ in range(refine):
            if not live.size:
                break
            m = (a[live] + ((b[live] - a[live]).astype(F) * F(0.5)).astype(F)).astype(F)
            ok = (m > a[live]) & (m < b[live])
            live, m = live[ok], m[ok]
            if not live.size:
                break
            dm = evaluate(live, m)
            nref[live] += 1
            nonfin = np.isnan(dm)
            close = ~nonfin & ~(np.abs(dm) > tol)
            near = ~nonfin & ~close & (np.signbit(dm) == inside[live])
            far = ~nonfin & ~near                                           # close, or on the far side: b = m, db = dm
            a[live[near]] = m[near]
            b[live[far]], db[live[far]] = m[far], dm[far]
            t[live[far]], d[live[far]] = m[far], dm[far]
            live = live[~nonfin & ~close]
    return t, d, status, nmarch, nref


def _stats(n, t, status, evals, steps, thin):
    found = (status == HIT) | (status == CROSSED)
    with np.errstate(invalid="ignore"):
        below = int((found & (t < F(thin))).sum())
    return {"n": n, "count": np.bincount(status, minlength=8).astype(np.int64), "evals": int(evals), "steps_max": int(steps.max()) if n else 0,
            "t_min": F(t[found].min()) if found.any() else F(np.inf), "t_max": F(t[found].max()) if found.any() else F(0), "below": below}


def raycast(sdf, origins, dirs, t0=0.0, tmax=np.inf, tol=1e-4, min_step=0.0, max_steps=256, refine=8, thin=0.0):
    """sdf: (n, 3) float32 -> (n,) float32. Returns (t (n,), d (n,), status (n,) uint8, steps (n,) uint16, stats dict)."""
    opts = check_opts(t0, tmax, tol, min_step, max_steps, refine)
    o = np.ascontiguousarray(origins, F).reshape(-1, 3)
    r = np.ascontiguousarray(dirs, F).reshape(-1, 3)
    n = len(o)
    if n == 0:
        raise RayError(EMPTY_BUFFERS, "no rays")
    status = np.full(n, SKIPPED, np.uint8)
    part = np.isfinite(o).all(axis=1) & np.isfinite(r).all(axis=1)          # 1.
    t, d, status, nmarch, nref = _march(sdf, o, r, part, status, *opts)
    steps = (nmarch + nref).astype(np.uint16)
    return t, d, status, steps, _stats(n, t, status, nmarch.sum() + nref.sum(), nmarch + nref, thin)


def thickness(sdf, verts, step, t0, tmax, tol, min_step=0.0, max_steps=256, refine=8, thin=0.0):
    """Returns (thickness (V,) float32, status (V,) uint8, stats dict)."""
    opts = check_opts(t0, tmax, tol, min_step, max_steps, refine)
    step = F(step)
    if not (np.isfinite(step) and step > 0):
        raise RayError(BAD_ARGUMENT, "step")
    x = np.ascontiguousarray(verts, F).reshape(-1, 3)
    V = len(x)
    h = F(step * F(0.5))
    status = np.full(V, SKIPPED, np.uint8)
    part = np.flatnonzero(np.isfinite(x).all(axis=1))
    r = np.zeros((V, 3), F)
    with np.errstate(all="ignore"):
        xp = x[part]
        g = np.empty((len(part), 3), F)
        for k in range(3):                                                  # normals_kernel's taps, in its order
            a, b = xp.copy(), xp.copy()
            a[:, k] = xp[:, k] + h
            b[:, k] = xp[:, k] - h
            if len(part):
                da = np.asarray(sdf(np.ascontiguousarray(a)), F).reshape(-1)
                g[:, k] = da - np.asarray(sdf(np.ascontiguousarray(b)), F).reshape(-1)
        s = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]
        flat = ~(s > 0)
        ln = np.sqrt(s)
        r[part] = -(g / ln[:, None]).astype(F)
    status[part[flat]] = FLAT
    go = np.zeros(V, bool)
    go[part[~flat]] = True
    r[~go] = 0
    t, _, status, nmarch, nref = _march(sdf, x, r, go, status, *opts)
    found = (status == HIT) | (status == CROSSED)
    th = np.where(found, t, np.where(status == MISS, F(np.inf), NOT_EVALUATED)).astype(F)
    th.view(np.uint32)[~found & (status != MISS)] = 0x7fc00000
    return th, status, _stats(V, t, status, 6 * len(part) + nmarch.sum() + nref.sum(), nmarch + nref, thin)
