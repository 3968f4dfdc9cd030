"""The UI's view, host side (no GPU): the orbit camera helper gsdf_hip_view_orbit against the UI's formulas (gsdfaux/ui.go:18,123,
220,276-297), and the CPU twin of the frame (tests/viewref.py) against geometry it does not share with the device kernel -- a
sphere and a box whose hit depths, normals and silhouettes follow from the camera alone."""
import math

import numpy as np
import pytest

import viewref
from gsdf_amd import hip
from oracle.oracle import OracleSDF
from scaffold.builder import Builder

F = np.float32


def _np_orbit(bb, yaw, pitch, cam_dist=None, target=(0, 0, 0)):
    """numpy float32 transcription of the UI's camera (ui.go:266-297) with the bounds' Diagonal() of scaffold/ms.hpp."""
    bb = np.asarray(bb, F)
    sz = bb[3:] - bb[:3]

    def hyp(p, q):
        p, q = F(abs(p)), F(abs(q))
        if p < q:
            p, q = q, p
        if p == 0:
            return F(0)
        q = F(q / p)
        return F(p * np.sqrt(F(F(1) + F(q * q))))
    diag = hyp(sz[0], hyp(sz[1], sz[2]))
    cd = F(cam_dist) if cam_dist else diag
    pi = F(3.14159265359)
    pitch = min(max(F(pitch), F(-pi / F(2) + F(0.01))), F(pi / F(2) - F(0.01)))
    cp, sp = F(math.cos(float(pitch))), F(math.sin(float(pitch)))
    cy, sy = F(math.cos(float(yaw))), F(math.sin(float(yaw)))
    d = np.array([cp * sy, sp, cp * cy], F)
    ta = np.asarray(target, F)
    ro = ta - d * cd

    def nrm(v):
        return v / np.sqrt((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2])
    ww = nrm(ta - ro)
    uu = nrm(np.cross(ww, np.array([0, 1, 0], F)).astype(F))
    vv = np.cross(uu, ww).astype(F)
    return ro, uu, vv, ww, F(cd + diag), diag, d


def _shapes():
    b = Builder()
    return [("sphere", b.NewSphere(1.0)), ("box", b.NewBox(1.0, 2.0, 0.5, 0.1)), ("npt-flange", b.Scene("npt-flange")),
            ("offset-torus", b.Translate(b.NewTorus(2.0, 0.5), 3.0, -1.0, 0.5))]


@pytest.mark.parametrize("name,shape", _shapes())
def test_orbit_runs_without_a_device_and_matches_the_ui(name, shape):
    bb = shape.Bounds()
    for yaw, pitch in ((0.0, 0.0), (0.7, 0.3), (-2.5, -1.1), (3.9, 1.2)):
        v = hip.view_orbit(bb, yaw, pitch)
        uu, vv, ww = (np.array(getattr(v, k)[:], np.float64) for k in ("uu", "vv", "ww"))
        for a in (uu, vv, ww):
            assert abs(np.linalg.norm(a) - 1) < 1e-6
        assert abs(uu @ vv) < 1e-6 and abs(uu @ ww) < 1e-6 and abs(vv @ ww) < 1e-6
        assert np.allclose(np.cross(uu, vv), -ww, atol=1e-6)  # right-handed as the UI's: ww = vv x uu
        ro, nuu, nvv, nww, cdist, _, _ = _np_orbit(bb, yaw, pitch)
        for got, want in ((v.ro, ro), (v.uu, nuu), (v.vv, nvv), (v.ww, nww)):
            assert np.allclose(np.array(got[:], F), want, rtol=0, atol=4e-7 * max(1.0, float(np.abs(want).max()))), (name, yaw, pitch)
        assert v.char_dist == cdist and v.aa == 1 and v.max_steps == 256


def test_orbit_defaults_are_the_uis():
    b = Builder()
    s = b.Scene("bolt")
    diag = F(s.Diagonal())
    v = hip.view_orbit(s.Bounds(), 0.4, 0.2)
    ro = np.array(v.ro[:], np.float64)
    assert abs(np.linalg.norm(ro) - float(diag)) < 1e-5 * float(diag)  # camDist = diag (ui.go:123), target the origin
    assert v.char_dist == F(diag + diag)  # charDist = camDist + diag (ui.go:220)
    v = hip.view_orbit(s.Bounds(), 0.4, 0.2, cam_dist=7.5)
    assert abs(np.linalg.norm(np.array(v.ro[:], np.float64)) - 7.5) < 1e-5 and v.char_dist == F(F(7.5) + diag)
    t = (1.0, -2.0, 0.5)
    v = hip.view_orbit(s.Bounds(), 0.4, 0.2, cam_dist=3.0, target=t)
    assert abs(np.linalg.norm(np.array(v.ro[:], np.float64) - np.array(t)) - 3.0) < 1e-5


def test_orbit_clamps_pitch():
    bb = Builder().NewSphere(1.0).Bounds()
    pi = F(3.14159265359)
    hi, lo = F(pi / F(2) - F(0.01)), F(-pi / F(2) + F(0.01))
    as_bytes = lambda v: bytes(v)  # noqa: E731
    top = as_bytes(hip.view_orbit(bb, 0.3, float(hi)))
    assert as_bytes(hip.view_orbit(bb, 0.3, 2.0)) == top and as_bytes(hip.view_orbit(bb, 0.3, 40.0)) == top
    bottom = as_bytes(hip.view_orbit(bb, 0.3, float(lo)))
    assert as_bytes(hip.view_orbit(bb, 0.3, -1.58)) == bottom and bottom != top
    assert as_bytes(hip.view_orbit(bb, 0.3, 1.5)) != top  # inside the range: untouched
    v = hip.view_orbit(bb, 0.3, 2.0)
    assert abs(v.ww[1] - math.sin(float(hi))) < 1e-6


def test_orbit_refuses_non_finite_input():
    bb = Builder().NewSphere(1.0).Bounds()
    for args in ((float("nan"), 0.0), (0.0, float("inf"))):
        with pytest.raises(hip.HipError):
            hip.view_orbit(bb, *args)
    with pytest.raises(hip.HipError):
        hip.view_orbit(bb, 0.0, 0.0, target=(0.0, float("nan"), 0.0))


def _twin(shape, view, w, h):
    o = OracleSDF(shape.tree())
    c = viewref.CountingSDF(o.Evaluate)
    out = viewref.render(c, view, w, h)
    return out, c.count


def test_twin_sphere_depth_normal_disc_and_counts():
    r = 1.0
    b = Builder()
    s = b.NewSphere(r)
    w = h = 42  # the sample of aa = 1 sits at fragCoord - 0.5: pixel (row h/2 - 1, column w/2) looks down the axis
    yaw, pitch = 0.6, 0.35
    v = hip.view_orbit(s.Bounds(), yaw, pitch)
    cam = float(np.linalg.norm(np.array(v.ro[:], np.float64)))
    out, count = _twin(s, v, w, h)
    rc, ic = h // 2 - 1, w // 2
    assert abs(float(out["depth"][rc, ic]) - (cam - r)) <= 2e-4
    d = np.array([math.cos(pitch) * math.sin(yaw), math.sin(pitch), math.cos(pitch) * math.cos(yaw)])
    assert np.abs(out["normal"][rc, ic] - (-d)).max() < 1e-3
    # the hit disc: a sample ray at screen offset p makes tan(theta) = |p| / 1.5 with the axis; the sphere subtends sin(alpha) = r / cam
    i = np.arange(w)
    rows = np.arange(h)
    px = (2.0 * i - w) / h
    py = (2.0 * (h - 1 - rows) - h) / h
    pr = np.hypot(px[None, :], py[:, None])
    rho = 1.5 * math.tan(math.asin(r / cam))
    hitmask = np.isfinite(out["depth"])
    ring = np.abs(pr - rho) <= 2.0 / h  # one pixel either side of the predicted edge
    assert not (hitmask & (pr > rho + 2.0 / h)).any() and hitmask[pr < rho - 2.0 / h].all()
    predicted = int((pr < rho).sum())
    assert abs(int(hitmask.sum()) - predicted) <= int(ring.sum())
    assert predicted > 100
    # evals: march steps + 4 per hit, and every one of them reached the distance function
    assert int(out["evals"].astype(np.int64).sum()) == count
    assert (out["evals"][hitmask] >= 5).all() and (out["evals"][~hitmask] >= 1).all()
    # colours: alpha 255; background black; a lit pixel is not
    assert (out["rgba"][..., 3] == 255).all() and (out["rgba"][~hitmask][:, :3] == 0).all() and (out["rgba"][hitmask][:, :3].max(axis=1) > 0).all()


def test_twin_box_face_on_silhouette_columns():
    a, dist = 1.0, 4.0
    b = Builder()
    s = b.NewBox(2 * a, 2 * a, 2 * a, 0.0)
    w, h = 42, 42
    v = hip.view_orbit(s.Bounds(), 0.0, 0.0, cam_dist=dist)
    out, count = _twin(s, v, w, h)
    rc = h // 2 - 1  # the row whose samples have p.y = 0
    cols = np.nonzero(np.isfinite(out["depth"][rc]))[0]
    # the front face z = -a at distance dist - a: a ray with p.x hits it at |x| = (dist - a) |p.x| / 1.5 <= a
    px = (2.0 * np.arange(w) - w) / h
    want = np.nonzero(np.abs(px) * (dist - a) / 1.5 <= a)[0]
    assert cols.tolist() == want.tolist() and len(want) == 21
    centre = out["depth"][rc, w // 2]
    assert abs(float(centre) - (dist - a)) <= 2e-4
    assert int(out["evals"].astype(np.int64).sum()) == count


def test_twin_supersampling_order_and_max_steps():
    b = Builder()
    s = b.NewSphere(1.0)
    v = hip.view_orbit(s.Bounds(), 0.2, 0.1)
    v.aa = 3
    out, count = _twin(s, v, 20, 16)
    assert int(out["evals"].astype(np.int64).sum()) == count
    v1 = hip.view_orbit(s.Bounds(), 0.2, 0.1)
    one, _ = _twin(s, v1, 20, 16)
    # a pixel fully inside the disc at aa = 1 is inside at aa = 3; the edge pixels blend
    assert (np.isfinite(out["depth"]) >= np.isfinite(one["depth"])).all()
    v.max_steps = 0
    none, count = _twin(s, v, 20, 16)
    assert count == 0 and (none["evals"] == 0).all() and np.isinf(none["depth"]).all() and (none["rgba"][..., :3] == 0).all()
