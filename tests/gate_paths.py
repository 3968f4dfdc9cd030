"""Hand-built trees whose gates (dev_ops.h: D_GATE2D / 3D / ZC / OB) whole waves take, the clusters of points that make them, and a
float64 predictor of what each cluster does to its gate. For tests/test_gpu_gate_paths.py; nothing here needs a GPU.

A gate skips its child only when EVERY point of a wave passes, so random points never take it: a cluster is 64 points (one wave of a
small host call) or 1024 (one tile of the device-resident call, whatever its points per lane), all within 1e-3 of the region's
diameter of one centre. The centres come from the gate's own region words: the region's centre, just inside and just outside each
face, and 0.5, 1, 2 and 4 diameters beyond the faces along the axes and a diagonal. Every cluster the predictor calls "pass" has
copies with ONE point replaced by a point inside the region (first, a middle and the last lane): the wave must not skip.

The predictor restates the gate's rule (dev_ops.h; interp.h: region_lb_*, gate_far) in float64: L from the region words, a (and c,
the enclosing difference's other operand) from the closed form of the operand evaluated first -- a sphere, circle or cylinder at the
origin; the toothed wheel's first copy through the oracle of one tooth -- and
    pass  : L > 0 and L > sg a + kk + m,  m = 1e-3 (L + |a|) + 2e-6 (|x| + |y| + |z|)
    outer : U = max(a, -L) + k4 < 0 and c + U <= -ok - (1e-3 (|c| + |U|) + 2e-6 (...))
A cluster is "pass" if every point passes one test with ten times the margin, "fail" if every point misses both by nine tenths of
it, "mixed" if it is a "pass" cluster with one "fail" point put in; anything else is unclassified, and the tests allow none.
"""
import numpy as np

import progcheck as PC
from gsdf_amd import hip
from oracle.oracle import OracleSDF
from scaffold.builder import Builder

F = np.float32
POLY7 = [(0, 0), (2, 0), (2.5, 1), (2, 2), (1, 2.5), (0, 2), (-0.5, 1)]
WHEEL_N = 9


def _sphere(r):
    return lambda p: np.linalg.norm(p, axis=1) - r


def _cyl(r, h):
    def f(p):
        dx, dy = np.hypot(p[:, 0], p[:, 1]) - r, np.abs(p[:, 2]) - h / 2
        return np.minimum(0, np.maximum(dx, dy)) + np.hypot(np.maximum(dx, 0), np.maximum(dy, 0))
    return f


def cases():
    """name -> dict(shape, dim, gate = (kind, flagged, which of that kind), target, a = closed form of lds[slot] at the gate,
    c = closed form of lds[oslot] or None)."""
    b = Builder()
    poly = lambda: b.NewPolygon(POLY7)
    ext = lambda: b.Translate(b.Extrude(poly(), 1.0), 3, 0.5, 0.25)
    p2 = lambda: b.Translate2D(poly(), 3, 0.5)
    screw = lambda: b.ScrewISO(2.0, 0.4, True, 4.0)
    star = b.NewPolygon([(1.2 * np.cos(t) * (1 if i % 2 else 0.5), 1.2 * np.sin(t) * (1 if i % 2 else 0.5)) for i, t in enumerate(np.linspace(0, 2 * np.pi, 12, endpoint=False))])
    tooth = b.Translate(b.Rotate(b.Extrude(star, 3.0), 0.5, (0, 0, 1)), 6.0, 0, 0)
    c3 = [(3, 0, 0), (0, 4, 0), (6, 0, 0), (0, 0, 5)]
    c2 = [(3, 0), (0, 4), (6, 0)]
    out = {}

    def add(name, shape, dim, kind, target, a, c=None, flagged=False, which=0, **kw):
        out[name] = dict(shape=shape, dim=dim, gate=(kind, flagged, which), target=target, a=a, c=c, **kw)

    add("union3d", b.Union(b.NewSphere(1), ext()), 3, "D_GATE3D", "D_COMBINE_MIN", _sphere(1))
    add("diff3d", b.Difference(b.NewSphere(4), ext()), 3, "D_GATE3D", "D_COMBINE_DIFF", _sphere(4))
    add("sunion3d", b.SmoothUnion(0.3, b.NewSphere(1), ext()), 3, "D_GATE3D", "D_COMBINE_SUNION", _sphere(1))
    add("sdiff3d", b.SmoothDifference(0.3, b.NewSphere(4), ext()), 3, "D_GATE3D", "D_COMBINE_SDIFF", _sphere(4))
    add("union2d", b.Union2D(b.NewCircle(1), p2()), 2, "D_GATE2D", "D_COMBINE_MIN", _sphere(1))
    add("diff2d", b.Difference2D(b.NewCircle(4), p2()), 2, "D_GATE2D", "D_COMBINE_DIFF", _sphere(4))
    add("zc-plain", b.Union(b.NewSphere(1), b.Translate(screw(), 5, 0, 0)), 3, "D_GATEZC", "D_COMBINE_MIN", _sphere(1))
    add("zc-hxy", b.Difference(b.NewCylinder(3, 3, 0), screw()), 3, "D_GATEZC", "D_COMBINE_DIFF", _cyl(3, 3), flagged=True)
    add("wheel", b.CircularArray(tooth, WHEEL_N, WHEEL_N), 3, "D_GATEOB", "D_COMBINE_MIN", None, wheel=tooth)
    # body - cutters - hole (knurled-cylinder in small): the hole is evaluated first, the cutters' gate carries its slot
    knurl = b.Twist(b.CircularArray(b.Translate(b.NewBox(1, 1, 4, 0), 4, 0, 0), 12, 12), 0.2)
    add("outer-smooth", b.SmoothDifference(0.5, b.SmoothDifference(0.5, b.NewSphere(4), knurl), b.NewCylinder(1, 10, 0)), 3,
        "D_GATEZC", "D_COMBINE_SDIFF", _sphere(4), c=_cyl(1, 10), flagged=True)
    add("outer-plain", b.Difference(b.Difference(b.NewSphere(4), ext()), b.NewCylinder(1, 10, 0)), 3, "D_GATE3D", "D_COMBINE_DIFF", _sphere(4), c=_cyl(1, 10))
    # wide unions: every child gated, the first against the D_UBOUND* bound (the running minimum in closed form: `wide`)
    w3 = b.Union(b.NewSphere(1), *[b.Translate(b.NewSphere(r), *c) for c, r in zip(c3, (1, 1, 1, 0.5))])
    w2 = b.Union2D(b.NewCircle(1), *[b.Translate2D(b.NewCircle(1), *c) for c in c2])
    for k in (0, 2):
        add(f"wide3d-gate{k}", w3, 3, "D_GATE3D", "D_COMBINE_MIN", None, which=k, wide=[((0, 0, 0), 1)] + list(zip(c3, (1, 1, 1, 0.5))))
        add(f"wide2d-gate{k}", w2, 2, "D_GATE2D", "D_COMBINE_MIN", None, which=k, wide=[((0, 0), 1)] + [(c, 1) for c in c2])
    # an instruction behind the gate's target reloads a position, and a cylinder there recomputes the hypot the gated child replaced
    prod = b.Translate(b.Intersection(b.NewCylinder(1, 2, 0), b.Extrude(poly(), 1.0)), 4, 0, 0)
    add("reload-behind", b.Intersection(b.Union(b.NewCylinder(3, 2, 0), prod), b.Translate(b.NewCylinder(8, 2, 0), 0, 0, 0.5)), 3,
        "D_GATE3D", "D_COMBINE_MIN", _cyl(3, 2), behind=("D_LOADP3", "D_CYL0"))
    return out


def pin(case):
    """The gate under test in the lowered program, asserted to be what the case says: dict(code, slots, res, pc, words)."""
    code, slots = hip.lower(case["shape"])
    res = PC.check(code, slots)
    assert not res.violations, res.violations[:3]
    kind, flagged, which = case["gate"]
    gates = [i for i in res.ins if i.name == kind]
    assert len(gates) > which, (kind, [i.name for i in res.ins])
    g = gates[which]
    assert bool(g.word & PC.FLAG_HXY) == flagged
    i0 = PC.GATES[kind]
    at = {i.pc: k for k, i in enumerate(res.ins)}
    t = res.ins[at[g.pc + (int(code[g.pc + 1 + i0 + 5]) & 0xFFFFFF)]]
    comb = res.ins[at[t.pc] + 1] if t.name == "D_LIP_DOM" else t
    assert comb.name == case["target"] and comb.slot == g.slot, (comb, g)
    assert (int(code[g.pc + 1 + i0 + 2]) != 0xFFFF) == (case["c"] is not None)
    if "behind" in case:
        assert [i.name for i in res.ins if i.pc > comb.pc and i.name in case["behind"]] == list(case["behind"])
    if "wide" in case:
        assert res.ins[at[g.pc] - 1].name == "D_SKIP" and sum(i.name == kind for i in res.ins) == len(case["wide"])
        assert any(i.name.startswith("D_UBOUND") and i.slot == g.slot for i in res.ins)
    if "wheel" in case:
        assert [i.name for i in res.ins if i.name in ("D_CIRC_PRE", "D_CIRC_ORDER")] == ["D_CIRC_PRE", "D_CIRC_ORDER"]
    f = code.view(F).astype(np.float64)
    return dict(code=code, slots=slots, res=res, pc=g.pc, region=f[g.pc + 1:g.pc + 1 + i0], sg=f[g.pc + 1 + i0], kk=f[g.pc + 2 + i0],
                ok=f[g.pc + 4 + i0], k4=f[g.pc + 5 + i0], kind=kind, flagged=flagged)


def region_box(g):
    """(centre, half extents) of the gate's region in the gate's frame, 3 components (2-D: z = 0, no extent)."""
    r, k = g["region"], g["kind"]
    if k == "D_GATE2D":
        lo, hi = np.array([r[0], r[1], 0.0]), np.array([r[2], r[3], 0.0])
    elif k == "D_GATE3D":
        lo, hi = r[:3], r[3:6]
    elif k == "D_GATEZC":
        lo, hi = np.array([r[0] - r[2], r[1] - r[2], r[3]]), np.array([r[0] + r[2], r[1] + r[2], r[4]])
    else:   # D_GATEOB: its own frame is turned about z by (c, s); the hull here only places the centres
        e = abs(r[2]) * r[4] + abs(r[3]) * r[5], abs(r[3]) * r[4] + abs(r[2]) * r[5]
        lo, hi = np.array([r[0] - e[0], r[1] - e[1], r[6]]), np.array([r[0] + e[0], r[1] + e[1], r[7]])
    return (lo + hi) / 2, (hi - lo) / 2


def inside_point(g):
    """A point of the region, in the gate's frame, at which a wave that wrongly skipped the child would return wrong bits: nine
    tenths of the way from the region's centre to its -x face (a box turned about z: its own x), an annulus: half way between its
    two radii. Not the centre: there the bound L of an extrusion's or a box's region IS the child's value (the z faces are
    nearest). Not the +x face: in the cases here that side lies outside the minuend's sphere, where a difference returns the
    minuend whatever the child's value is. (Found by running the tests against a wave vote changed to "lane 0 decides".)"""
    c, h = region_box(g)
    r = g["region"]
    if g["kind"] == "D_GATEZC":
        return c - np.array([(r[6] + r[2]) / 2 if r[6] > 0 else 0.9 * r[2], 0, 0])
    if g["kind"] == "D_GATEOB":
        return c - 0.9 * r[4] * np.array([r[2], r[3], 0])
    return c - np.array([0.9 * h[0], 0, 0])


def lower_bound(g, p):
    """L of interp.h's region_lb_* at the points p (n, 3), float64."""
    r, k = g["region"], g["kind"]
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    if k == "D_GATE2D":
        return np.maximum(np.maximum(r[0] - x, x - r[2]), np.maximum(r[1] - y, y - r[3]))
    if k == "D_GATE3D":
        return np.max([r[0] - x, x - r[3], r[1] - y, y - r[4], r[2] - z, z - r[5]], axis=0)
    if k == "D_GATEOB":
        dx, dy = x - r[0], y - r[1]
        return np.max([np.abs(r[2] * dx + r[3] * dy) - r[4], np.abs(r[2] * dy - r[3] * dx) - r[5], r[6] - z, z - r[7]], axis=0)
    cx, cy, rad, z0, z1, rs, rin = r
    if g["flagged"]:
        h = np.hypot(x, y)
        rlo, rhi = h * 0.999999, h * 1.000001
    else:
        ax, ay = np.abs(x - cx), np.abs(y - cy)
        mx, mn = np.maximum(ax, ay), np.minimum(ax, ay)
        rlo, rhi = np.maximum(mx, 0.70710605 * (ax + ay)), (mx + 0.41421402 * mn) * 1.000001
    L = np.max([z0 - z, z - z1, rs * (rlo - rad)], axis=0)
    return np.maximum(L, rs * (rin - rhi)) if rin > 0 else L


_tooth = {}


def frame(case, g, p):
    """(position in the gate's frame, a, c) of the world points p (n, 3), float64. None where the predictor cannot say (the wheel:
    the wave's choice of the first copy is not unanimous)."""
    if "wheel" in case:
        ang = 2 * np.pi / WHEEL_N
        idx = np.floor(np.arctan2(p[:, 1], p[:, 0]) / ang)
        idx = np.where(idx < 0, idx + WHEEL_N, idx)
        i0, i1 = np.where(idx >= WHEEL_N - 1, WHEEL_N - 1, idx), np.where(idx >= WHEEL_N - 1, 0, idx + 1)
        rot = lambda i: np.stack([np.cos(ang * i) * p[:, 0] + np.sin(ang * i) * p[:, 1], -np.sin(ang * i) * p[:, 0] + np.cos(ang * i) * p[:, 1], p[:, 2]], 1)
        p0, p1 = rot(i0), rot(i1)
        r = g["region"]
        d0, d1 = p0[:, 0] * r[0] + p0[:, 1] * r[1], p1[:, 0] * r[0] + p1[:, 1] * r[1]
        swap = (d0 > d1).sum() > (d1 > d0).sum()     # D_CIRC_ORDER: the wave's majority
        if min((d0 > d1).sum(), (d1 > d0).sum()) > 1:  # (one odd point may disagree; a split cluster's waves could decide either way)
            return None
        first, second = (p0, p1) if swap else (p1, p0)
        if "o" not in _tooth:
            _tooth["o"] = OracleSDF(case["wheel"].tree())
        return second, _tooth["o"].Evaluate(np.ascontiguousarray(first, F)).astype(np.float64), None
    if "wide" in case:
        # the running minimum in front of this gate: the D_UBOUND* bound, then the children evaluated so far (in the program's order:
        # the origin's first, then as listed -- each translate clobbers the position)
        res, code = g["res"], g["code"]
        ub = [i for i in res.ins if i.name.startswith("D_UBOUND")][0]
        d = case["dim"]
        box = code.view(F)[ub.pc + 2:ub.pc + ub.n].astype(np.float64).reshape(-1, 2 * d)
        far = np.maximum(np.abs(p[:, None, :d] - box[None, :, :d]), np.abs(p[:, None, :d] - box[None, :, d:]))
        a = 1.001 * np.sqrt((far ** 2).sum(-1).min(1)) + 1e-30
        for c, r in case["wide"][:case["gate"][2]]:
            a = np.minimum(a, np.linalg.norm(p[:, :d] - np.array(c, np.float64), axis=1) - r)
        return p, a, None
    return p, case["a"](p), (case["c"](p) if case["c"] is not None else None)


def classify(case, g, p):
    """(strong pass, strong fail) per point, or None."""
    fr = frame(case, g, np.asarray(p, np.float64))
    if fr is None:
        return None
    q, a, c = fr
    L = lower_bound(g, q)
    pad = 2e-6 * np.abs(q).sum(1)
    m = 1e-3 * (np.abs(L) + np.abs(a)) + pad
    rhs = g["sg"] * a + g["kk"]
    sp = (L > 10 * pad + 1e-12) & (L > rhs + 10 * m)
    sf = (L < -(10 * pad + 1e-12)) | (L < rhs + 0.1 * m)
    if c is not None:
        U = np.maximum(a, -L) + g["k4"]
        m2 = 1e-3 * (np.abs(c) + np.abs(U)) + pad
        sp = sp | ((U < -(10 * pad + 1e-12)) & (c + U <= -g["ok"] - 10 * m2))
        sf = sf & ((U > 10 * pad + 1e-12) | (c + U > -g["ok"] - 0.1 * m2))
    return sp, sf


def to_world(case, q):
    """World position of a position in the gate's frame (the wheel: the frame of the copy in sector 2, turned a little off the
    sector's ray so that no cluster straddles it)."""
    if "wheel" not in case:
        return q
    t = 2 * (2 * np.pi / WHEEL_N) + 0.03
    return np.stack([np.cos(t) * q[:, 0] - np.sin(t) * q[:, 1], np.sin(t) * q[:, 0] + np.cos(t) * q[:, 1], q[:, 2]], 1)


def centres(case, g):
    """[(label, centre in the gate's frame)] from the region words."""
    c, h = region_box(g)
    dim = case["dim"]
    D = 2 * np.linalg.norm(h)
    out = [("centre", inside_point(g))]
    for ax in range(dim):
        for s in (-1.0, 1.0):
            e = np.zeros(3)
            e[ax] = s
            out.append((f"in{'xyz'[ax]}{'+' if s > 0 else '-'}", c + e * (h[ax] - 1e-2 * D)))
            out.append((f"out{'xyz'[ax]}{'+' if s > 0 else '-'}", c + e * (h[ax] + 1e-2 * D)))
    dirs = [("x+", (1, 0, 0)), ("x-", (-1, 0, 0)), ("y+", (0, 1, 0))] + ([("z+", (0, 0, 1)), ("diag", (-1, 1, 1))] if dim == 3 else [("y-", (0, -1, 0)), ("diag", (-1, 1, 0))])
    for name, u in dirs:
        u = np.array(u, np.float64)
        for s in (0.5, 1, 2, 4):
            reach = np.abs(u) @ h if np.abs(u).sum() == 1 else np.linalg.norm(h)    # to the face, resp. beyond the corner
            out.append((f"far{name}*{s}", c + u / np.linalg.norm(u) * (reach + s * D), 0.1 * D * u / np.linalg.norm(u)))
    return out, D


def clusters(case, g, n, odd, seed=5):
    """[(label, class, points (n, dim) float32)]: one cluster of n points per centre, and for every "pass" cluster one copy per
    entry of `odd` with that point replaced by the region's centre. class: "pass" | "fail" | "mixed" | None (unclassified)."""
    cs, D = centres(case, g)
    cs = [tuple(x) for x in cs]
    rng = np.random.default_rng(seed)
    dim = case["dim"]
    # a point inside the region: its centre (the wheel: in the frame of whichever copy the cluster's waves evaluate second)
    inside = [to_world(case, cs[0][1][None, :])[0]]
    if "wheel" in case:
        inside.append(inside[0] * np.array([1, -1, 1]))
        t = 4 * (2 * np.pi / WHEEL_N)
        inside[1] = np.array([np.cos(t) * inside[1][0] - np.sin(t) * inside[1][1], np.sin(t) * inside[1][0] + np.cos(t) * inside[1][1], inside[1][2]])
    out = []
    for label, c, *step in cs:
        d = rng.normal(size=(n, 3))
        d *= (1e-3 * D * rng.random(n) ** (1 / 3) / np.linalg.norm(d, axis=1))[:, None]
        if dim == 2:
            d[:, 2] = 0
        # a far centre that lands where the gate's test is within ten of its own margins (neither class) moves by tenths of the
        # diameter, outwards and then sideways, three times each at the most: decided by the predictor alone, before anything runs
        moves = [np.zeros(3)]
        if step:
            side = np.array([-step[0][1], step[0][0], 0.0]) if step[0][0] or step[0][1] else np.array([np.linalg.norm(step[0]), 0.0, 0.0])
            moves += [j * step[0] for j in (1, 2, 3)] + [j * side for j in (1, 2, 3)]
        for mv in moves:
            pts = np.ascontiguousarray(to_world(case, (c + mv)[None, :] + d), F)
            k = classify(case, g, pts)
            cls = None if k is None else "pass" if k[0].all() else "fail" if k[1].all() else None
            if cls is not None:
                break
        out.append((label, cls, pts[:, :dim].copy()))
        if cls == "pass":
            for w in odd:
                for c0 in inside:
                    q = pts.copy()
                    q[w] = c0
                    kq = classify(case, g, q)
                    ok = kq is not None and kq[1][w] and np.delete(kq[0], w).all()
                    if ok:
                        break
                out.append((f"{label}/odd{w}", "mixed" if ok else None, q[:, :dim].copy()))
    return out
