"""The library's side of the rays ABI without a device: the two entry points are exported and declared, the ctypes mirrors are laid out
as the header asserts, the status codes are the header's, the kernel's and the twin's, and the argument checks that need no device
answer GSDF_ERR_BAD_ARGUMENT and write nothing."""
import ctypes as C
import os
import re

import numpy as np

import rayref as R
from gsdf_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = open(os.path.join(ROOT, "include", "gsdf_hip.h")).read()


def size(t):
    return int(re.search(r"GSDF_ABI_ASSERT\(sizeof\(%s\) == (\d+)," % t, HDR).group(1))


def test_symbols_and_layout():
    L = hip.lib()
    for name in ("gsdf_hip_raycast3", "gsdf_hip_indexed_thickness"):
        assert re.search(r"\bint %s\(" % name, HDR) and hasattr(L, name) and name in hip.SYMBOLS
    assert "---- rays (no reference counterpart)" in HDR
    assert C.sizeof(hip.RayOpts) == size("gsdf_ray_opts") == 32
    assert C.sizeof(hip.ThicknessOpts) == size("gsdf_thickness_opts") == 48
    assert C.sizeof(hip.RayStats) == size("gsdf_ray_stats") == 112
    for f, off in (("t0", 0), ("tmax", 4), ("tol", 8), ("min_step", 12), ("max_steps", 16), ("refine", 20), ("flags", 24), ("reserved", 28)):
        assert getattr(hip.RayOpts, f).offset == off, f
        assert off in (0, 28) or re.search(r"offsetof\(gsdf_ray_opts, %s\) == %d\b" % (f, off), HDR), f
    for f, off in (("ray", 0), ("step", 32), ("thin", 36), ("reserved", 40)):
        assert getattr(hip.ThicknessOpts, f).offset == off, f
        assert off in (0, 40) or re.search(r"offsetof\(gsdf_thickness_opts, %s\) == %d\b" % (f, off), HDR), f
    for f, off in (("n", 0), ("count", 8), ("evals", 72), ("steps_max", 80), ("t_min", 84), ("t_max", 88), ("reserved", 92), ("below", 96), ("ms_device", 104)):
        assert getattr(hip.RayStats, f).offset == off, f
        assert off in (0, 92) or re.search(r"offsetof\(gsdf_ray_stats, %s\) == %d\b" % (f, off), HDR), f
    assert hip.RayStats.RESULT_BYTES == hip.RayStats.ms_device.offset == R.RESULT_BYTES == 104
    st = hip.RayStats(n=3, evals=9, steps_max=4, t_min=1.5, t_max=2.5, below=1)
    st.count[1] = 3
    twin = {"n": 3, "count": [0, 3, 0, 0, 0, 0, 0, 0], "evals": 9, "steps_max": 4, "t_min": 1.5, "t_max": 2.5, "below": 1}
    assert st.result_bytes() == R.stats_bytes(twin)


def test_status_codes_agree():
    assert hip.RAY_STATUS == R.STATUS
    kh = open(os.path.join(ROOT, "gsdf_amd", "csrc", "kernels_ray.h")).read()
    for k, n in enumerate(R.STATUS):
        assert re.search(r"GSDF_RAY_%s = %d\b" % (n, k), HDR), n
        assert re.search(r"#define RAY_%s %du\b" % (n, k), kh), n
        assert getattr(R, n) == k


def test_argument_checks_without_a_device():
    L = hip.lib()
    rays = np.zeros((2, 6), np.float32)
    t = np.full(2, 7, np.float32)
    st = hip.RayStats(n=77)

    def cast(p=None, n=2, **kw):
        o = hip.RayOpts(**{**dict(t0=0.0, tmax=10.0, tol=1e-4, min_step=0.0, max_steps=16, refine=4), **kw})
        rc = L.gsdf_hip_raycast3(p, rays.ctypes.data, n, C.byref(o), 0.0, t.ctypes.data, None, None, None, C.byref(st))
        return rc, L.gsdf_hip_last_error().decode()

    rc, msg = cast()
    assert rc == -3 and "null" in msg
    some = C.c_void_p(0x1000)   # never dereferenced: the options are refused first
    for kw, word in ((dict(t0=-1.0), "t0"), (dict(t0=float("inf")), "t0"), (dict(t0=float("nan")), "t0"), (dict(t0=2.0, tmax=1.0), "tmax"),
                     (dict(tmax=float("nan")), "tmax"), (dict(tol=-1.0), "tol"), (dict(tol=float("inf")), "tol"), (dict(min_step=-1.0), "min_step"),
                     (dict(min_step=float("nan")), "min_step"), (dict(max_steps=0), "max_steps"), (dict(max_steps=4097), "max_steps"),
                     (dict(refine=-1), "refine"), (dict(refine=33), "refine"), (dict(flags=1), "flags"), (dict(reserved=1), "reserved")):
        rc, msg = cast(some, **kw)
        assert rc == -3 and word in msg, (kw, msg)
    o = hip.RayOpts(t0=0.0, tmax=10.0, tol=1e-4, min_step=0.0, max_steps=16, refine=4)
    assert L.gsdf_hip_raycast3(some, rays.ctypes.data, 2, C.byref(o), 0.0, None, None, None, None, None) == -3   # all five outputs NULL
    assert L.gsdf_hip_raycast3(some, None, 2, C.byref(o), 0.0, t.ctypes.data, None, None, None, None) == -3
    assert L.gsdf_hip_raycast3(some, rays.ctypes.data, 2, None, 0.0, t.ctypes.data, None, None, None, None) == -3

    def thick(**kw):
        ro = hip.RayOpts(**{**dict(t0=0.01, tmax=10.0, tol=1e-4, min_step=0.0, max_steps=16, refine=4), **kw.pop("ray", {})})
        to = hip.ThicknessOpts(**{**dict(ray=ro, step=0.25, thin=0.0), **kw})
        rc = L.gsdf_hip_indexed_thickness(None, None, C.byref(to), t.ctypes.data, None, C.byref(st))
        return rc, L.gsdf_hip_last_error().decode()

    rc, msg = thick()
    assert rc == -3 and "null" in msg
    for kw, word in ((dict(step=0.0), "step"), (dict(step=float("nan")), "step"), (dict(step=float("inf")), "step"), (dict(ray=dict(max_steps=0)), "max_steps"),
                     (dict(ray=dict(tol=-1.0)), "tol"), (dict(reserved=(C.c_uint32 * 2)(0, 1)), "reserved")):
        rc, msg = thick(**kw)
        assert rc == -3 and word in msg, (kw, msg)
    assert L.gsdf_hip_indexed_thickness(None, None, None, t.ctypes.data, None, C.byref(st)) == -3
    assert (t == 7).all() and st.n == 77   # on an error nothing is written
