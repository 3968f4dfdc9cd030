"""gsdf_hip_raycast3 and gsdf_hip_indexed_thickness on the device against the numpy twin of their contract (tests/rayref.py) over the
oracle's evaluator: t and d equal BIT FOR BIT, the status bytes, the steps and the stats' leading block equal as bytes, the program's
evaluation counter grows by exactly st.evals, and a dry run gives the same stats. The twin sees the rays and the options, and no
device result."""
import ctypes as C

import numpy as np
import pytest

import rayref as R
from corpus import shapes3d
from oracle.oracle import OracleSDF
from scaffold.builder import Builder
from test_gpu_nan import degenerate_trees
from test_gpu_project import opts_for, simplified
from test_gpu_weld import SMALL
from test_ray_ref import shell_node_tree, shell_tree

pytestmark = pytest.mark.gpu
F = np.float32
TOL = F(1e-4)
BLOCK = 256
NAN = np.nan

# the hand rays of test_ray_ref.py against the sphere of radius 5: (origin, direction)
HAND = [((-20, 0.3, 0.1), (1, 0, 0)), ((0, 0, 0), (0, 0.6, 0.8)), ((-20, 7, 0), (1, 0, 0)), ((-20, 5.0005, 0), (1, 0, 0)), ((1, 2, 0), (1, 0, 0)),
        ((0, 0, 0), (0, 1.2, 1.6)), ((3, -3, 2), (-2.5, 1.5, 0.25)), ((0, 0, -30), (0, 0, 0.5))]
SKIP = [((NAN, 0, 0), (1, 0, 0)), ((0, 0, 0), (np.inf, 0, 0)), ((0, -np.inf, 0), (0, 1, 0)), ((0, 0, 0), (0, 0, NAN))]


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def sphere_rays(n):
    """n rays: the hand rays in turn, with SKIPPED rays first and last and, from 65 rays on, a whole wave of them (rays 64 .. 127:
    a wave that is all skipped; with n = 65 the one ray of the second wave -- alone in it)."""
    o = np.array([HAND[k % len(HAND)][0] for k in range(n)], F)
    r = np.array([HAND[k % len(HAND)][1] for k in range(n)], F)
    for j, k in enumerate(skipped_of(n)):
        o[k], r[k] = SKIP[j % len(SKIP)]
    return o, r


def skipped_of(n):
    return sorted({0, n - 1} | set(range(64, min(n, 128))))


def same_bits(a, b, what):
    bad = np.flatnonzero(u32(a) != u32(b))
    assert bad.size == 0, (what, bad.size, bad[:6].tolist(), np.asarray(a)[bad[:3]].tolist(), np.asarray(b)[bad[:3]].tolist())


def got_stats(st):
    return {"n": st.n, "count": list(st.count), "evals": st.evals, "steps_max": st.steps_max, "t": (st.t_min, st.t_max), "below": st.below}


def want_stats(ts):
    return {"n": ts["n"], "count": ts["count"].tolist(), "evals": ts["evals"], "steps_max": ts["steps_max"], "t": (float(ts["t_min"]), float(ts["t_max"])),
            "below": ts["below"]}


def check_rays(gpu, sdf, fn, o, r, what="", **kw):
    """Device rays through program `sdf` against the twin's over the distance function `fn`: the four outputs, the stats, the evaluation
    counter, the dry run (stats alone) and a second run. Returns (device outputs, twin outputs)."""
    e0 = sdf.Evaluations()
    t, d, s, n, st = sdf.raycast(o, r, **kw)
    assert sdf.Evaluations() - e0 == st.evals, (what, sdf.Evaluations() - e0, st.evals)
    counted = R.CountingSDF(fn)
    tt, td, ts, tn, tst = R.raycast(counted, o, r, **kw)
    print(what, kw, {R.STATUS[k]: c for k, c in enumerate(st.count) if c}, "evals", st.evals, "steps_max", st.steps_max, "t", (st.t_min, st.t_max), "ms", st.ms_device)
    assert s.tobytes() == ts.tobytes(), (what, np.flatnonzero(s != ts)[:8].tolist(), s[s != ts][:8], ts[s != ts][:8])
    assert n.tobytes() == tn.tobytes(), (what, np.flatnonzero(n != tn)[:8].tolist())
    same_bits(t, tt, (what, "t"))
    same_bits(d, td, (what, "d"))
    assert got_stats(st) == want_stats(tst), (what, got_stats(st), want_stats(tst))
    assert st.result_bytes() == R.stats_bytes(tst) and counted.count == st.evals
    # the dry run: the stats alone; and the same call again gives the same bytes
    rays = np.ascontiguousarray(np.concatenate([np.asarray(o, F).reshape(-1, 3), np.asarray(r, F).reshape(-1, 3)], axis=1))
    full = {**dict(t0=0.0, tmax=np.inf, tol=1e-4, min_step=0.0, max_steps=256, refine=8), **kw}   # (raycast()'s defaults)
    ro = gpu.RayOpts(t0=F(full["t0"]), tmax=F(full["tmax"]), tol=F(full["tol"]), min_step=F(full["min_step"]), max_steps=int(full["max_steps"]), refine=int(full["refine"]))
    dry = gpu.RayStats()
    assert gpu.lib().gsdf_hip_raycast3(sdf._h, rays.ctypes.data, len(rays), C.byref(ro), F(kw.get("thin", 0)), None, None, None, None, C.byref(dry)) == 0
    assert dry.result_bytes() == st.result_bytes()
    again = sdf.raycast(o, r, **kw)
    assert [x.tobytes() for x in again[:4]] == [x.tobytes() for x in (t, d, s, n)] and again[4].result_bytes() == st.result_bytes()
    return (t, d, s, n, st), (tt, td, ts, tn, tst)


@pytest.mark.parametrize("n", [1, 63, 64, 65, BLOCK, BLOCK + 1])
def test_sphere_ray_counts(gpu, n):
    """Padding lanes, a wave that is all SKIPPED, a ray alone in its wave, more than one workgroup."""
    shape = Builder().NewSphere(5)
    sdf, cpu = gpu.SDF3HIP(shape), OracleSDF(shape.tree())
    o, r = sphere_rays(n)
    dev, tw = check_rays(gpu, sdf, cpu.Evaluate, o, r, ("sphere", n), tmax=100, tol=TOL, max_steps=64, thin=6.0)
    s = dev[2]
    assert s[0] == R.SKIPPED and s[-1] == R.SKIPPED and (n < 65 or (s[64:128] == R.SKIPPED).all())
    assert dev[4].count[R.SKIPPED] == len(skipped_of(n)) and np.flatnonzero(s == R.SKIPPED).tolist() == skipped_of(n)
    if n >= 63:
        assert s[1:5].tolist() == [R.HIT, R.MISS, R.STEPS, R.HIT] and dev[0][9] == 5.0


def test_sphere_options(gpu):
    """max_steps = 1, refine = 0 and 32, tmax = t0, tmax = +Inf with rays that hit, a min_step that forces crossings, t0 = -0."""
    shape = Builder().NewSphere(5)
    sdf, cpu = gpu.SDF3HIP(shape), OracleSDF(shape.tree())
    o, r = sphere_rays(200)
    seen = np.zeros(8, np.int64)
    for kw in (dict(max_steps=1), dict(tmax=100, refine=0, min_step=0.75), dict(tmax=100, refine=32, min_step=0.75), dict(t0=1.5, tmax=1.5),
               dict(tmax=np.inf, max_steps=64), dict(tmax=100, tol=0, max_steps=4096, refine=4), dict(t0=-0.0, tmax=0.0), dict(tmax=50, min_step=0.3, refine=8, thin=16.0)):
        dev, tw = check_rays(gpu, sdf, cpu.Evaluate, o, r, "sphere", **{**dict(tol=TOL), **kw})
        seen += tw[4]["count"]
        if kw.get("max_steps") == 1:
            assert set(dev[2]) <= {R.SKIPPED, R.STEPS, R.HIT} and dev[4].steps_max == 1
        if kw.get("tmax") == np.inf:
            assert dev[4].count[R.HIT] > 50 and dev[4].count[R.MISS] == 0
        if "t0" in kw:
            assert dev[4].steps_max == 1 and dev[4].count[R.MISS] > 0
    assert seen[R.CROSSED] > 0 and seen[R.HIT] > 0 and seen[R.MISS] > 0 and seen[R.STEPS] > 0, seen.tolist()


@pytest.mark.parametrize("case", ["two-spheres", "shell-node"])
def test_thin_shell_caveat_on_the_device(gpu, case):
    """The twin's CROSSED / stepped-over pairs of test_ray_ref.py on the device, interpreter and specialised: the wall between two
    spheres, and the builder's Shell node."""
    tree, o0, step_in, step_over = (shell_tree(), (1, 2, 0), 1.0, 0.5) if case == "two-spheres" else (shell_node_tree(), (0.2, 0.4, 0), 0.3, 0.5)
    sdf, cpu = gpu.SDFHIP(tree), OracleSDF(tree)
    o, r = np.array([o0] * 3, F), np.array([[1, 0, 0], [0, 1, 0], [0, 0, -1]], F)
    for form in ("interpreter", "specialised"):
        for refine in (0, 4, 24):
            dev, _ = check_rays(gpu, sdf, cpu.Evaluate, o, r, (case, form), tmax=100, tol=TOL, min_step=step_in, refine=refine)
            assert dev[2][0] == R.CROSSED
        dev, _ = check_rays(gpu, sdf, cpu.Evaluate, o, r, (case, form), tmax=100, tol=TOL, min_step=step_over)
        assert dev[2][0] == R.MISS
        sdf.specialize()


def corner_rays(bb, n, seed):
    """n rays from the corners of the bounds toward jittered interior points."""
    rng = np.random.default_rng(seed)
    bb = np.asarray(bb, F)
    corners = np.array([[bb[3 * ((k >> a) & 1) + a] for a in range(3)] for k in range(8)], F)
    o = corners[rng.integers(0, 8, n)]
    target = (bb[:3] + rng.random((n, 3), F) * (bb[3:] - bb[:3])).astype(F)
    return o, (target - o).astype(F)


def thickness_opts(res):
    return dict(step=F(res / F(4)), t0=F(res / F(4)), tmax=F(F(64) * res), tol=F(res / F(1024)), max_steps=128, refine=8, thin=F(F(2) * res))


def check_thickness(ix, sdf, fn, v, what, **o):
    e0 = sdf.Evaluations()
    th, s, st = ix.thickness(sdf, **o)
    assert sdf.Evaluations() - e0 == st.evals, (what, sdf.Evaluations() - e0, st.evals)
    counted = R.CountingSDF(fn)
    tth, ts, tst = R.thickness(counted, v, **o)
    print(what, {R.STATUS[k]: c for k, c in enumerate(st.count) if c}, "evals", st.evals, "t", (st.t_min, st.t_max), "below", st.below, "ms", st.ms_device)
    assert s.tobytes() == ts.tobytes(), (what, np.flatnonzero(s != ts)[:8].tolist(), s[s != ts][:8], ts[s != ts][:8])
    same_bits(th, tth, (what, "thickness"))
    assert got_stats(st) == want_stats(tst), (what, got_stats(st), want_stats(tst))
    assert st.result_bytes() == R.stats_bytes(tst) and counted.count == st.evals
    none, none2, dry = ix.thickness(sdf, dry=True, **o)
    assert none is None and none2 is None and dry.result_bytes() == st.result_bytes()
    return th, s, st


@pytest.mark.parametrize("name", SMALL)
def test_small_shapes(gpu, name):
    """The SMALL shapes at resdiv 48 (twist: the field that is not 1-Lipschitz -- device and twin agree whatever the answer): rays
    from the bounds' corners, and the thickness of the welded-then-simplified mesh; interpreter and specialised handles give the
    same bytes."""
    sx, v, i, k, res = simplified(gpu, name)
    shape = dict(shapes3d()[1])[name]
    cpu = OracleSDF(shape.tree())
    interp, spec = gpu.SDF3HIP(shape), gpu.SDF3HIP(shape).specialize()
    o, r = corner_rays(shape.Bounds(), 300, 61)
    kw = dict(tmax=F(2), tol=F(res / F(1024)), max_steps=96, refine=8, thin=F(0.5))
    a, _ = check_rays(gpu, interp, cpu.Evaluate, o, r, (name, "interpreter"), **kw)
    b, _ = check_rays(gpu, spec, cpu.Evaluate, o, r, (name, "specialised"), **kw)
    assert [x.tobytes() for x in a[:4]] == [x.tobytes() for x in b[:4]] and a[4].result_bytes() == b[4].result_bytes()
    assert a[4].count[R.HIT] + a[4].count[R.CROSSED] > 0
    to = thickness_opts(res)
    ta = check_thickness(sx, interp, cpu.Evaluate, v, (name, "interpreter"), **to)
    tb = check_thickness(sx, spec, cpu.Evaluate, v, (name, "specialised"), **to)
    assert ta[0].tobytes() == tb[0].tobytes() and ta[1].tobytes() == tb[1].tobytes() and ta[2].result_bytes() == tb[2].result_bytes()
    assert spec.info()["kernels"]["ray"] == "ray_kernel:specialised", spec.info()["kernels"]
    assert interp.info()["kernels"]["ray"] == "ray_kernel:interpreter", interp.info()["kernels"]
    if name == "sphere":   # every inward ray of the unit sphere crosses it: about 2, whatever the vertex
        assert ta[2].count[R.HIT] + ta[2].count[R.CROSSED] == len(v) and 1.9 < ta[2].t_min <= ta[2].t_max < 2.1


@pytest.mark.parametrize("form", ["interpreter", "specialised"])
def test_projection_and_rays_take_turns_on_one_handle(gpu, form):
    """The projection and the rays each keep a counter block on the handle, cleared at every call: a projection, then a dry
    projection, a dry thickness and 64 + 1 rays, then the projection again, all on ONE handle. The second projection's stats and
    outputs are the first's, and the handle's counter grows by the three calls' evaluations, no more."""
    sx, v, _, _, res = simplified(gpu, "sphere")
    shape = dict(shapes3d()[1])["sphere"]
    sdf = gpu.SDF3HIP(shape)
    if form == "specialised":
        sdf.specialize()
    po = opts_for(res)
    first, st1 = sx.project(sdf, **po)
    e0 = sdf.Evaluations()
    _, dry = sx.project(sdf, dry=True, **po)
    _, _, th = sx.thickness(sdf, dry=True, **thickness_opts(res))
    o, r = corner_rays(shape.Bounds(), 64 + 1, 5)
    rays = sdf.raycast(o, r, tmax=F(2), tol=F(res / F(1024)), max_steps=96)
    assert sdf.Evaluations() - e0 == dry.evals + th.evals + rays[4].evals and min(dry.evals, th.evals, rays[4].evals) > 0
    assert th.n == len(v) and rays[4].n == 65 and th.count[R.HIT] + th.count[R.CROSSED] == len(v) and rays[4].count[R.HIT] + rays[4].count[R.CROSSED] > 0
    second, st2 = sx.project(sdf, **po)
    assert dry.result_bytes() == st1.result_bytes() == st2.result_bytes()
    assert [x.tobytes() for x in second.read() + second.fit()] == [x.tobytes() for x in first.read() + first.fit()]
    again = sdf.raycast(o, r, tmax=F(2), tol=F(res / F(1024)), max_steps=96)
    assert again[4].result_bytes() == rays[4].result_bytes() and [x.tobytes() for x in again[:4]] == [x.tobytes() for x in rays[:4]]
    assert sdf.info()["kernels"]["ray"] == ("ray_kernel:specialised" if form == "specialised" else "ray_kernel:interpreter")


def test_slab_thickness_and_flat(gpu):
    """Hand-placed vertices on the two large faces of a 2 x 10 x 10 box: exactly 2 within 2 tol; the centre of a sphere: FLAT; a NaN
    vertex: SKIPPED; rays that leave through tmax: +Inf."""
    shape = Builder().NewBox(2, 10, 10, 0)
    sdf, cpu = gpu.SDF3HIP(shape), OracleSDF(shape.tree())
    v = np.array([[1, 0, 0], [-1, 0, 0], [1, 3.5, -4], [-1, -4, 4], [1, 4, 4], [NAN, 0, 0]], F)
    ix = gpu.IndexedHIP.from_arrays(v, np.array([[0, 1, 2], [3, 4, 5]], np.uint32))
    for form in ("interpreter", "specialised"):
        th, s, st = check_thickness(ix, sdf, cpu.Evaluate, v, ("slab", form), step=0.01, t0=0.01, tmax=30, tol=TOL, thin=2.5)
        assert s.tolist() == [R.HIT] * 5 + [R.SKIPPED] and (np.abs(th[:5] - 2) <= 2 * TOL).all() and u32(th)[5] == 0x7fc00000 and st.below == 5
        th, s, st = check_thickness(ix, sdf, cpu.Evaluate, v, ("slab", form), step=0.01, t0=0.01, tmax=1.5, tol=TOL)
        assert s.tolist() == [R.MISS] * 5 + [R.SKIPPED] and np.isposinf(th[:5]).all() and st.t_min == np.inf and st.t_max == 0
        sdf.specialize()
    ball = Builder().NewSphere(5)
    sdf, cpu = gpu.SDF3HIP(ball), OracleSDF(ball.tree())
    v = np.array([[0, 0, 0], [0, 3, 4], [5, 0, 0]], F)
    ix = gpu.IndexedHIP.from_arrays(v, np.array([[0, 1, 2]], np.uint32))
    th, s, st = check_thickness(ix, sdf, cpu.Evaluate, v, "ball", step=0.25, t0=0.01, tmax=30, tol=TOL)
    assert s.tolist() == [R.FLAT, R.HIT, R.HIT] and u32(th)[0] == 0x7fc00000 and (np.abs(th[1:] - 10) <= 2 * TOL).all()


def test_degenerate_fields(gpu):
    """Trees whose distance is NaN or infinite in places (tests/test_gpu_nan.py). Where the reference's distance is NaN the device
    returns NaN or a stand-in (the relation that file states), so the rays -- every bit -- are held to the twin over the device's own
    evaluator: NONFINITE rays, no hang, finite stats."""
    seen = np.zeros(8, np.int64)
    for j, (name, t) in enumerate(degenerate_trees()):
        sdf = gpu.SDFHIP(t)
        o, r = corner_rays(np.array(t.bb[:], F), 320, 67 + j)
        dev, tw = check_rays(gpu, sdf, lambda p: sdf.Evaluate(p), o, r, name, tmax=4, tol=TOL, max_steps=64, refine=6)
        st = dev[4]
        assert sum(st.count) == 320 and st.evals <= 320 * (64 + 6) and np.isfinite(st.t_max) and not np.isnan(st.t_min)
        assert (u32(dev[1])[dev[2] == R.NONFINITE] == 0x7fc00000).all()
        seen += tw[4]["count"]
    assert seen[R.NONFINITE] > 0, seen.tolist()


def test_errors(gpu):
    b = Builder()
    sdf = gpu.SDF3HIP(b.NewSphere(5))
    o, r = sphere_rays(8)
    good = dict(t0=0.0, tmax=10.0, tol=1e-4, min_step=0.0, max_steps=16, refine=4)
    for bad in (dict(t0=-1.0), dict(t0=float("inf")), dict(t0=float("nan")), dict(t0=2.0, tmax=1.0), dict(tmax=float("nan")), dict(tol=-1e-3), dict(tol=float("inf")),
                dict(tol=float("nan")), dict(min_step=-1.0), dict(min_step=float("inf")), dict(max_steps=0), dict(max_steps=4097), dict(refine=-1), dict(refine=33)):
        with pytest.raises(R.RayError):
            R.check_opts(**{**good, **bad})
        with pytest.raises(gpu.HipError) as e:
            sdf.raycast(o, r, **{**good, **bad})
        assert e.value.code == -3, bad
    rays = np.ascontiguousarray(np.concatenate([o, r], axis=1))
    t, st = np.full(8, 7, F), gpu.RayStats(n=77)
    ro = gpu.RayOpts(**good)
    L = gpu.lib()
    assert L.gsdf_hip_raycast3(sdf._h, rays.ctypes.data, 0, C.byref(ro), 0.0, t.ctypes.data, None, None, None, C.byref(st)) == -1          # GSDF_ERR_EMPTY_BUFFERS
    assert L.gsdf_hip_raycast3(sdf._h, rays.ctypes.data, 1 << 32, C.byref(ro), 0.0, t.ctypes.data, None, None, None, C.byref(st)) == R.CAPACITY
    assert L.gsdf_hip_raycast3(sdf._h, rays.ctypes.data, 8, C.byref(ro), 0.0, None, None, None, None, None) == -3                            # all five outputs NULL
    flat2d = gpu.SDF2HIP(b.NewCircle(1))
    assert L.gsdf_hip_raycast3(flat2d._h, rays.ctypes.data, 8, C.byref(ro), 0.0, t.ctypes.data, None, None, None, C.byref(st)) == -7       # GSDF_ERR_DIMENSION
    ro.flags = 1
    assert L.gsdf_hip_raycast3(sdf._h, rays.ctypes.data, 8, C.byref(ro), 0.0, t.ctypes.data, None, None, None, C.byref(st)) == -3
    assert (t == 7).all() and st.n == 77                                      # on an error nothing is written
    # each output optional
    ro.flags = 0
    assert L.gsdf_hip_raycast3(sdf._h, rays.ctypes.data, 8, C.byref(ro), 0.0, t.ctypes.data, None, None, None, None) == 0
    assert (u32(t) == u32(sdf.raycast(o, r, **good)[0])).all()
    # thickness: the options, a 2-D program, nothing asked for
    v = np.array([[5, 0, 0], [0, 5, 0], [0, 0, 5]], F)
    ix = gpu.IndexedHIP.from_arrays(v, np.array([[0, 1, 2]], np.uint32))
    tgood = dict(step=0.25, t0=0.01, tmax=30.0, tol=1e-4)
    for bad in (dict(step=0.0), dict(step=float("nan")), dict(t0=-1.0), dict(tmax=0.0), dict(tol=-1.0), dict(max_steps=0), dict(refine=40)):
        for dry in (False, True):
            with pytest.raises(gpu.HipError) as e:
                ix.thickness(sdf, dry=dry, **{**tgood, **bad})
            assert e.value.code == -3, bad
    with pytest.raises(gpu.HipError) as e:
        ix.thickness(flat2d, **tgood)
    assert e.value.code == -7
    to = gpu.ThicknessOpts(ray=gpu.RayOpts(t0=0.01, tmax=30.0, tol=1e-4, max_steps=16, refine=4), step=0.25)
    assert L.gsdf_hip_indexed_thickness(ix._h, sdf._h, C.byref(to), None, None, None) == -3
    th, s, st = ix.thickness(sdf, **tgood)
    assert s.tolist() == [R.HIT] * 3 and (np.abs(th - 10) <= 2e-4).all()
