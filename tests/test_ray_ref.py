"""The numpy twin of the rays contract (tests/rayref.py) over the oracle's evaluator, held to geometry: what a ray against a sphere, a
thin shell and a slab must answer, independent of any device. The sphere has radius 5, tol is 1e-4."""
import numpy as np
import pytest

import rayref as R
from oracle.oracle import OracleSDF
from scaffold.builder import Builder
from test_gpu_nan import degenerate_trees

F = np.float32
TOL = F(1e-4)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def sphere():
    return OracleSDF(Builder().NewSphere(5).tree()).Evaluate


def shell_tree():
    b = Builder()
    return b.Difference(b.NewSphere(5.125), b.NewSphere(4.875)).tree()


def one(sdf, o, r, **kw):
    t, d, s, n, st = R.raycast(sdf, np.array([o], F), np.array([r], F), **{**dict(tol=TOL), **kw})
    return float(t[0]), float(d[0]), int(s[0]), int(n[0]), st


def test_sphere_hand_rays():
    sdf = R.CountingSDF(sphere())
    t, d, s, n, st = one(sdf, (-20, 0.3, 0.1), (1, 0, 0))
    assert s == R.HIT and abs(t - (20 - np.sqrt(25 - 0.1))) <= 2 * TOL and n == 3 and abs(d) <= TOL and sdf.count == st["evals"] == 3
    # from the centre: the first step is |d|, so a start inside the solid works
    t, d, s, n, st = one(sphere(), (0, 0, 0), (0, 0.6, 0.8))
    assert s == R.HIT and t == 5.0 and n == 2
    t, d, s, n, st = one(sphere(), (-20, 7, 0), (1, 0, 0), tmax=100)
    assert s == R.MISS and st["t_min"] == np.inf and st["t_max"] == 0 and d > TOL and t <= 100
    t, d, s, n, st = one(sphere(), (-20, 5.0005, 0), (1, 0, 0), max_steps=64)
    assert s == R.STEPS and n == 64 and st["steps_max"] == 64 and d > TOL
    # the direction is used as given: twice the direction, half the t
    t2 = one(sphere(), (0, 0, 0), (0, 1.2, 1.6))[0]
    assert t2 == 2.5
    # tmax = t0: one evaluation, then the first step passes tmax
    t, d, s, n, st = one(sphere(), (-20, 0, 0), (1, 0, 0), t0=1, tmax=1)
    assert (s, t, d, n) == (R.MISS, 1.0, 14.0, 1)
    t, d, s, n, st = one(sphere(), (-20, 0, 0), (1, 0, 0), max_steps=1)
    assert (s, t, d, n) == (R.STEPS, 0.0, 15.0, 1)


def shell_node_tree():
    """The builder's Shell node over the sphere: t (|s(p / t)| - t), here | |p| - 5 t | - t^2 -- a wall of 2 t^2 = 0.25 about the
    radius 5 t = 1.7678 for t = sqrt(0.125)."""
    b = Builder()
    return b.Shell(b.NewSphere(5), float(F(np.sqrt(F(0.125))))).tree()


def crossed_and_stepped_over(sdf, o, near, wall, step_in, step_over):
    """The caveat of the contract, both ways, for a ray from o along +x inside the cavity of a shell whose wall it meets at t = near:
    a min_step of step_in lands INSIDE the wall (one crossing: CROSSED, and the bisection finds the near face); a min_step of step_over
    lands behind it (two crossings in one step: the ray goes on and leaves through tmax)."""
    got = [one(sdf, o, (1, 0, 0), tmax=100, min_step=step_in, refine=k) for k in (0, 4, 24)]
    assert [g[2] for g in got] == [R.CROSSED] * 3
    ts, ns = [g[0] for g in got], [g[3] for g in got]
    assert ts[0] >= ts[1] >= ts[2] >= near - 2 * TOL and ns[0] < ns[1] <= ns[2]
    assert all(g[1] < 0 or abs(g[1]) <= TOL for g in got)   # the far side of the crossing: inside the wall
    t24, d24 = F(ts[2]), got[2][1]
    # at 24: on the surface within tol, or the bracket is one ulp wide (a one ulp below b evaluates to the near side)
    a = np.nextafter(t24, F(0))
    da = float(sdf(np.array([[F(o[0]) + a, o[1], o[2]]], F))[0])
    assert abs(d24) <= TOL or da > TOL
    assert abs(float(t24) - near) <= 2 * TOL
    t, d, s, n, st = one(sdf, o, (1, 0, 0), tmax=100, min_step=step_over)
    assert s == R.MISS and t > near + wall and st["count"][R.MISS] == 1
    # and without a minimum step the march converges on the inner face
    t, d, s, n, st = one(sdf, o, (1, 0, 0), tmax=100)
    assert s == R.HIT and abs(t - near) <= 2 * TOL


def test_thin_shell_crossed_and_stepped_over():
    """A spherical shell about the sphere of radius 5 with a wall of 0.25 (radii 4.875 .. 5.125), the ray from (1, 2, 0) along +x:
    min_step 1.0 gives CROSSED, 0.5 steps over the wall. The wall is the difference of two spheres. The builder's Shell node cannot
    give this case: Shell(s, t) evaluates t (|s(p / t)| - t), so over the sphere of radius 5 its wall is 2 t^2 wide about the radius
    5 t, a wall of 0.25 lies at 1.64 .. 1.89, and the ray from (1, 2, 0), |o| = 2.24, starts outside it and never meets it. The
    node itself has the case below."""
    crossed_and_stepped_over(OracleSDF(shell_tree()).Evaluate, (1, 2, 0), np.sqrt(4.875 ** 2 - 4) - 1, 0.25, 1.0, 0.5)


def test_shell_node_crossed_and_stepped_over():
    """The same through the Shell node (shell_node_tree: a wall of 0.25 at radii 1.6428 .. 1.8928), the ray from (0.2, 0.4, 0) in its
    cavity along +x. It meets the inner face at t = 1.3933; the march is at t = 1.1955 after two evaluations and the next step there is the minimum, so a
    min_step of 0.3 lands 0.10 inside the wall and one of 0.5 lands at t = 1.70, past the outer face at t = 1.65."""
    t = float(F(np.sqrt(F(0.125))))
    inner, outer = 5 * t - t * t, 5 * t + t * t
    near = np.sqrt(inner ** 2 - 0.16) - 0.2
    crossed_and_stepped_over(OracleSDF(shell_node_tree()).Evaluate, (0.2, 0.4, 0), near, np.sqrt(outer ** 2 - 0.16) - 0.2 - near, 0.3, 0.5)


def test_skipped_and_nonfinite():
    sdf = R.CountingSDF(sphere())
    o = np.array([[np.nan, 0, 0], [0, 0, 0], [0, np.inf, 0], [0, 0, 0]], F)
    r = np.array([[1, 0, 0], [1, 0, np.nan], [1, 0, 0], [-np.inf, 0, 0]], F)
    t, d, s, n, st = R.raycast(sdf, o, r, tol=TOL)
    assert (s == R.SKIPPED).all() and sdf.count == 0 == st["evals"] and (n == 0).all() and (u32(t) == 0x7fc00000).all() and (u32(d) == 0x7fc00000).all()
    assert st["count"].tolist() == [4, 0, 0, 0, 0, 0, 0, 0] and st["t_min"] == np.inf
    # a field that is NaN beyond x = 2: the ray reports the t at which it met the NaN
    field = lambda p: np.where(p[:, 0] > 2, F(np.nan), sphere()(p)).astype(F)
    t, d, s, n, st = R.raycast(field, np.array([[0, 0, 0]], F), np.array([[1, 0, 0]], F), tol=TOL)
    assert s[0] == R.NONFINITE and t[0] == 5.0 and u32(d)[0] == 0x7fc00000 and n[0] == 2
    # the degenerate trees of test_gpu_nan.py: rays from the bounds' corners through the part
    rng = np.random.default_rng(53)
    seen = np.zeros(8, np.int64)
    for name, tree in degenerate_trees():
        bb = np.array(tree.bb[:], F)
        corners = np.array([[bb[3 * ((k >> a) & 1) + a] for a in range(3)] for k in range(8)], F)
        o = corners[rng.integers(0, 8, 96)]
        target = (bb[:3] + rng.random((96, 3), F) * (bb[3:] - bb[:3])).astype(F)
        cnt = R.CountingSDF(OracleSDF(tree).Evaluate)
        t, d, s, n, st = R.raycast(cnt, o, (target - o).astype(F), tmax=4, tol=TOL, max_steps=64)
        assert st["count"].sum() == 96 and cnt.count == st["evals"] == int(n.sum()) and (u32(d)[s == R.NONFINITE] == 0x7fc00000).all(), name
        seen += st["count"]
    assert seen[R.NONFINITE] > 0, seen.tolist()


def test_thickness_of_a_slab_and_a_flat_vertex():
    box = R.CountingSDF(OracleSDF(Builder().NewBox(2, 10, 10, 0).tree()).Evaluate)
    v = np.array([[1, 0, 0], [-1, 0, 0], [1, 3.5, -4], [-1, -4, 4], [1, 4, 4], [np.nan, 0, 0]], F)
    th, s, st = R.thickness(box, v, step=0.01, t0=0.01, tmax=30, tol=TOL, thin=2.5)
    assert s.tolist() == [R.HIT] * 5 + [R.SKIPPED] and (np.abs(th[:5] - 2) <= 2 * TOL).all() and u32(th)[5] == 0x7fc00000
    assert st["count"].sum() == 6 == st["n"] and st["evals"] == box.count and st["below"] == 5 and abs(st["t_min"] - 2) <= 2 * TOL >= abs(st["t_max"] - 2)
    assert R.thickness(box, v, step=0.01, t0=0.01, tmax=30, tol=TOL, thin=1.5)[2]["below"] == 0
    # a ray that leaves through tmax: +Inf
    th, s, st = R.thickness(box, v[:2], step=0.01, t0=0.01, tmax=1.5, tol=TOL)
    assert s.tolist() == [R.MISS] * 2 and np.isposinf(th).all() and st["t_min"] == np.inf
    # the centre of the sphere: the six taps cancel
    sp = R.CountingSDF(sphere())
    th, s, st = R.thickness(sp, np.array([[0, 0, 0], [0, 3, 4]], F), step=0.25, t0=0.01, tmax=30, tol=TOL)
    assert s.tolist() == [R.FLAT, R.HIT] and u32(th)[0] == 0x7fc00000 and abs(th[1] - 10) <= 2 * TOL
    assert st["count"][R.FLAT] == 1 and st["evals"] == sp.count and st["count"].sum() == 2


def test_stats_and_option_checks():
    rng = np.random.default_rng(59)
    sdf = R.CountingSDF(sphere())
    o = (rng.random((300, 3), F) * 14 - 7).astype(F)
    r = (rng.random((300, 3), F) * 2 - 1).astype(F)
    o[7] = np.nan
    t, d, s, n, st = R.raycast(sdf, o, r, tmax=40, tol=TOL, thin=3.0)
    found = (s == R.HIT) | (s == R.CROSSED)
    assert st["count"].sum() == 300 == st["n"] and st["evals"] == sdf.count == int(n.sum()) and st["steps_max"] == n.max()
    assert found.sum() > 50 and (s == R.MISS).sum() > 50 and s[7] == R.SKIPPED
    assert st["t_min"] == t[found].min() and st["t_max"] == t[found].max() and st["below"] == (t[found] < 3).sum()
    assert len(R.stats_bytes(st)) == R.RESULT_BYTES
    # rays that start inside find the surface too: a HIT is within tol of it, |o + t r| = 5 (a direction longer than 1 oversteps: CROSSED,
    # and the far end of its bracket is inside the part or within tol)
    ins = (s == R.HIT) & (np.linalg.norm(o, axis=1) < 5)
    assert ins.sum() > 5 and (np.abs(np.linalg.norm(o[ins].astype(np.float64) + t[ins, None].astype(np.float64) * r[ins], axis=1) - 5) <= 2 * TOL).all()
    assert (np.abs(d[s == R.HIT]) <= TOL).all()
    for bad in (dict(t0=-1), dict(t0=np.inf), dict(t0=np.nan), dict(t0=2, tmax=1), dict(tmax=np.nan), dict(tol=-1), dict(tol=np.inf), dict(min_step=-1),
                dict(min_step=np.nan), dict(max_steps=0), dict(max_steps=4097), dict(refine=-1), dict(refine=33), dict(flags=1)):
        with pytest.raises(R.RayError) as e:
            R.check_opts(**bad)
        assert e.value.code == R.BAD_ARGUMENT, bad
    R.check_opts(t0=0, tmax=0, tol=0, min_step=0, max_steps=4096, refine=32)
    with pytest.raises(R.RayError):
        R.thickness(sphere(), o, step=0, t0=0.01, tmax=1, tol=TOL)
