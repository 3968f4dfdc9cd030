"""A numpy twin of the indexed-mesh PROJECT contract (include/gsdf_hip.h, "indexed meshes: project onto the field"): (verts, a
distance function, the options) in; positions, d_before, d_after, the status bytes and the stats' leading block out. Nothing here
looks at a device result.

Every product, sum, difference and the division is one float32 numpy operation in the contract's order; the comparisons are
numpy's IEEE ones (false on NaN) under `NOT`, as the contract writes them. Per trip only the vertices still live are evaluated
(like viewref.render), so a counting distance function sees exactly st["evals"] points."""
import struct

import numpy as np

F = np.float32
SKIPPED, ON, CONVERGED, ITERS, FLAT, CLAMPED, NONFINITE, REVERTED = range(8)
STATUS = ["SKIPPED", "ON", "CONVERGED", "ITERS", "FLAT", "CLAMPED", "NONFINITE", "REVERTED"]
NOT_EVALUATED = np.array([0x7fc00000], np.uint32).view(F)[0]
BAD_ARGUMENT, DIMENSION = -3, -7


class ProjectError(Exception):
    """code: the GSDF_ERR_* the device returns for the same options."""

    def __init__(self, code, msg):
        super().__init__(msg)
        self.code = code


def check_opts(step, tol, max_move, max_iters, flags=0):
    step, tol, max_move = F(step), F(tol), F(max_move)
    if not (np.isfinite(step) and step > 0):
        raise ProjectError(BAD_ARGUMENT, "step")
    if not (np.isfinite(tol) and tol >= 0):
        raise ProjectError(BAD_ARGUMENT, "tol")
    if not (np.isfinite(max_move) and max_move >= 0):
        raise ProjectError(BAD_ARGUMENT, "max_move")
    if not 0 <= int(max_iters) <= 64:
        raise ProjectError(BAD_ARGUMENT, "max_iters")
    if flags != 0:
        raise ProjectError(BAD_ARGUMENT, "flags")
    return step, tol, max_move, int(max_iters)


def stats_bytes(st):
    """The leading block of gsdf_project_stats (112 bytes)."""
    return struct.pack("<12Q2f2I", int(st["n_verts"]), *[int(c) for c in st["count"]], int(st["evals"]), int(st["over_tol_before"]),
                       int(st["over_tol_after"]), float(st["max_abs_before"]), float(st["max_abs_after"]), int(st["steps_max"]), 0)


def project(sdf, verts, step, tol, max_move, max_iters=8):
    """sdf: (n, 3) float32 -> (n,) float32. Returns (positions (V, 3) float32, d_before (V,), d_after (V,), status (V,) uint8, stats
    dict); stats has, besides the contract's fields, "trips" and "gradients" (V,): step 1 / step 2 reached per vertex, and "steps"."""
    step, tol, max_move, max_iters = check_opts(step, tol, max_move, max_iters)
    v0 = np.ascontiguousarray(verts, F).reshape(-1, 3)
    V = len(v0)
    h = F(step * F(0.5))
    h2 = F(h + h)
    mm = F(max_move * max_move)
    x = v0.copy()
    part = np.isfinite(v0).all(axis=1)
    status = np.full(V, SKIPPED, np.uint8)
    db = np.full(V, NOT_EVALUATED, F)
    dc = db.copy()
    trips, grads, steps = np.zeros(V, np.int64), np.zeros(V, np.int64), np.zeros(V, np.int64)

    def evaluate(p):
        return np.asarray(sdf(np.ascontiguousarray(p, F)), F).reshape(-1)

    live = np.flatnonzero(part)
    with np.errstate(all="ignore"):
        for it in range(max_iters + 1):
            if live.size == 0:
                break
            d = evaluate(x[live])                                            # 1.
            trips[live] += 1
            dc[live] = d
            if it == 0:
                db[live] = d
            nonfin = np.isnan(d) if it == 0 else np.zeros(len(d), bool)
            on = ~nonfin & ~(np.abs(d) > tol)
            out_of_trips = ~nonfin & ~on & (it == max_iters)
            status[live[nonfin]] = NONFINITE
            status[live[on]] = ON if it == 0 else CONVERGED
            status[live[out_of_trips]] = ITERS
            go = ~(nonfin | on | out_of_trips)
            live, d = live[go], d[go]
            if live.size == 0:
                break
            xl = x[live]
            g = np.empty((len(live), 3), F)                                  # 2.
            for k in range(3):
                a, b = xl.copy(), xl.copy()
                a[:, k] = xl[:, k] + h
                b[:, k] = xl[:, k] - h
                g[:, k] = evaluate(a) - evaluate(b)
            grads[live] += 1
            s = (g[:, 0] * g[:, 0] + g[:, 1] * g[:, 1]) + g[:, 2] * g[:, 2]  # 3.
            flat = ~(s > 0)
            t = (d * h2) / s                                                 # 4.
            xn = (xl - t[:, None] * g).astype(F)
            u = (xn - v0[live]).astype(F)                                    # 5.
            r = (u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1]) + u[:, 2] * u[:, 2]
            clamped = ~flat & ~(r <= mm)
            status[live[flat]] = FLAT
            status[live[clamped]] = CLAMPED
            ok = ~(flat | clamped)
            x[live[ok]] = xn[ok]
            steps[live[ok]] += 1
            live = live[ok]
        # the end
        judged = part & (status != NONFINITE)
        worse = judged & (np.isnan(dc) | (np.abs(dc) > np.abs(db)))
    status[worse] = REVERTED
    dc[worse] = db[worse]
    pos = x.copy()
    keep = worse | ~part | (steps == 0)
    pos[keep] = v0[keep]

    def over(d):
        with np.errstate(invalid="ignore"):
            return int((part & (np.isnan(d) | (np.abs(d) > tol))).sum())

    def largest(d):
        a = np.abs(d[part & ~np.isnan(d)])
        return F(a.max()) if a.size else F(0)

    st = {"n_verts": V, "count": np.bincount(status, minlength=8).astype(np.int64), "evals": int(trips.sum() + 6 * grads.sum()),
          "over_tol_before": over(db), "over_tol_after": over(dc), "max_abs_before": largest(db), "max_abs_after": largest(dc),
          "steps_max": int(steps.max()) if V else 0, "trips": trips, "gradients": grads, "steps": steps}
    return pos, db, dc, status, st


class CountingSDF:
    """A distance function that counts the points it was asked for (the twin's own evaluation count)."""

    def __init__(self, fn):
        self.fn, self.count = fn, 0

    def __call__(self, pos):
        self.count += pos.shape[0]
        return self.fn(pos)
