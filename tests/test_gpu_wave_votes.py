"""Wave votes of the evaluator with ONE lane off the short route (dev_math.h: wave_mask / wave_ok).

The evaluator takes a short route -- no division, no square root expansion, a skipped subtree -- where EVERY point of a wave
qualifies, and the long one for the whole wave otherwise: same bits either way for the points that qualify, wrong bits for one that
does not. A vote that comes out wrong therefore shows only when a single lane of a wave leaves the short route, so each case here
is one wave's worth of points that qualify plus one that does not, the odd one placed first, in the middle and last, compared bit
for bit with the oracle's evaluator:

  * through gsdf_hip_eval3 on host buffers -- small calls run one point per lane, point i = lane i: 64 points are one wave;
  * through the device-resident call, which runs K points per lane (point kp of lane t = tile + kp * 256 + t): 1024 points fill every
    point slot of a tile's four waves for K = 1, 2 or 4, so no wave holds padding points the test does not choose;
  * with the interpreter kernels and with the specialised ones (their own votes: the square root and the short atan2 / cos-sin
    routes exist only there); a per-tree build that fails is a failure of the test, as everywhere in the suite;
  * partial last waves, every case: n = 1, 65, 129 and 257 points (64 K + 1 for K = 1, 2 and 4), the odd point last.

One mesh of npt-flange at resdiv 100 through the octree, flat and dual-contouring paths against the oracle's triangle sets covers
the ballots of the brick tail, the prune queue, the polygon culling and the lattice's bit planes.
"""
import numpy as np
import pytest

from scaffold.builder import Builder
from oracle.oracle import OracleSDF

pytestmark = pytest.mark.gpu
F = np.float32
TILE = 1024  # 4 points per lane x 256 lanes: a whole tile of the device-resident kernel for K = 1, 2 or 4


def _cases():
    """name -> (shape, on(rng, n) = n points on the short route, off = one point that leaves it)."""
    b = Builder()
    out = {}

    # hypot_k: hypot(max(dr, 0), max(dz, 0)) of a cylinder (radius 1, z in [-1, 1]). Over the flat face dr < 0 < dz: one argument is 0 for
    # the whole wave, the hypot is the other. Beyond the rim both are positive.
    def cyl_on(rng, n):
        r, a = 0.9 * np.sqrt(rng.random(n)), 2 * np.pi * rng.random(n)
        return np.stack([r * np.cos(a), r * np.sin(a), 1.25 + rng.random(n)], 1).astype(F)
    out["hypot"] = (b.NewCylinder(1.0, 2.0, 0.0), cyl_on, np.array([1.5, 0.25, 1.75], F))

    # smooth_h: the blend weight of a smooth union of two unit spheres 3 apart, k = 0.2. |d1 - d2| >= 0.5005 k away from the bisector
    # plane x = 1.5 (here: |x - 1.5| >= 1); on the plane d1 = d2 and the weight is the quotient's.
    def smooth_on(rng, n):
        p = (rng.random((n, 3)) * 2 - 1).astype(F)
        p[:, 0] = np.where(rng.random(n) < 0.5, -1.0 - rng.random(n), 4.0 + rng.random(n))
        return p.astype(F)
    out["smooth"] = (b.SmoothUnion(0.2, b.NewSphere(1.0), b.Translate(b.NewSphere(1.0), 3.0, 0.0, 0.0)), smooth_on, np.array([1.5, 0.3, 0.1], F))

    # poly_edges: the numerators (p - v1) . e of every edge inside 2^-90 .. 2^90 for generic points; 2^-100 off the vertex at the origin
    # along the edge (1, 0) the numerator is 2^-100 * 4.
    poly = b.Extrude(b.NewPolygon([(0, 0), (4, 0), (4, 3), (1, 3), (0, 2)]), 2.0)

    def poly_on(rng, n):
        return (np.array([-1, -1, -1.5], F) + rng.random((n, 3)) * np.array([6, 5, 3], F)).astype(F) + F(0.0137)
    out["poly-range"] = (poly, poly_on, np.array([2.0 ** -100, -0.5, 0.25], F))
    # sqrt_k (per-tree builds): the polygon's squared distance below 2^-96 -- 2^-70 below the edge y = 0, d = 2^-140, a subnormal the
    # bare v_sqrt_f32 does not take (the numerators stay ordinary: only this vote fails)
    out["sqrt"] = (poly, poly_on, np.array([0.5, -(2.0 ** -70), 0.25], F))

    # div_uniform_k in a screw's thread (the saw of z + lead * theta / 2 pi) and its polygon profile: generic points, and one on the
    # axis plane z = 2^-100, y = 0
    screw = b.ScrewISO(10.0, 1.5, True, 20.0)

    def screw_on(rng, n):
        return (np.array([-6, -6, -9], F) + rng.random((n, 3)) * np.array([12, 12, 18], F)).astype(F) + F(0.0137)
    out["screw-range"] = (screw, screw_on, np.array([4.6, 0.0, 2.0 ** -100], F))

    # region gates (npt-flange: a box gate and a z-cylinder gate in front of the thread and the bolt circle): far outside the part
    # every child is far from every point; one point on the thread
    flange = b.Scene("npt-flange")

    def flange_on(rng, n):
        a = 2 * np.pi * rng.random(n)
        r = 90.0 + 20.0 * rng.random(n)
        return np.stack([r * np.cos(a), r * np.sin(a), 40.0 + 10.0 * rng.random(n)], 1).astype(F)
    out["gate"] = (flange, flange_on, np.array([6.1, 0.2, -3.0], F))
    return out


_CASES = _cases()
_state = {}


def _handles(gpu, name):
    """(oracle, interpreter handle, specialised handle) of a case: built once, shared."""
    if name not in _state:
        shape = _CASES[name][0]
        _state[name] = (OracleSDF(shape.tree()),) + _pair(gpu, shape)
    return _state[name]


def _pair(gpu, shape):
    """An interpreter handle and a specialised one; the per-tree build must succeed and must be what the handle runs."""
    plain, spec = gpu.SDF3HIP(shape), gpu.SDF3HIP(shape)
    spec.specialize()
    assert spec.info()["specialized"] and not plain.info()["specialized"], (spec.info()["kernels"], plain.info()["kernels"])
    return plain, spec


def _points(name, n, where, seed):
    _, on, off = _CASES[name]
    pos = np.ascontiguousarray(on(np.random.default_rng(seed), n), F)
    pos[where] = off
    return pos


def _mismatch(a, b):
    return np.flatnonzero((a.view(np.uint32) != b.view(np.uint32)) & ~(np.isnan(a) & np.isnan(b)))


def _eval_dev(sdf, pos):
    import torch
    tp = torch.from_numpy(pos).to("cuda").contiguous()
    td = torch.empty(len(pos), device="cuda")
    sdf.evaluate_dev(tp.data_ptr(), 12, td.data_ptr(), len(pos))
    torch.cuda.synchronize()
    return td.cpu().numpy()


@pytest.mark.parametrize("name", list(_CASES))
def test_one_lane_off_the_short_route(gpu, name):
    ref, plain, spec = _handles(gpu, name)
    for kind, sdf in (("interpreter", plain), ("specialised", spec)):
        for where in (0, 31, 63):  # one point per lane: the wave of a small host call
            pos = _points(name, 64, where, 100 + where)
            bad = _mismatch(sdf.Evaluate(pos), ref.Evaluate(pos))
            assert bad.size == 0, (name, kind, "host", where, bad[:8].tolist())
        for where in (0, 515, TILE - 1):  # K points per lane: a whole tile of the device-resident kernel
            pos = _points(name, TILE, where, 200 + where)
            bad = _mismatch(_eval_dev(sdf, pos), ref.Evaluate(pos))
            assert bad.size == 0, (name, kind, "device", where, bad[:8].tolist())


@pytest.mark.parametrize("n", [1, 65, 129, 257])
def test_partial_last_wave(gpu, n):
    """The last wave holds one point, and it is the one off the short route."""
    for name in _CASES:
        ref, plain, spec = _handles(gpu, name)
        pos = _points(name, n, n - 1, 300 + n)
        want = ref.Evaluate(pos)
        for kind, sdf in (("interpreter", plain), ("specialised", spec)):
            assert _mismatch(sdf.Evaluate(pos), want).size == 0, (name, kind, "host", n)
            assert _mismatch(_eval_dev(sdf, pos), want).size == 0, (name, kind, "device", n)


def _sorted_bits(tris):
    t = np.ascontiguousarray(tris, F).reshape(-1, 9).view(np.uint32)
    return t[np.lexsort(t.T[::-1])]


def _flange_refs():
    if "refs" not in _state:
        s = Builder().Scene("npt-flange")
        cpu = OracleSDF(s.tree())
        res = F(float(s.Diagonal()) / 100)
        _state["refs"] = (s, res, cpu.render_octree(res), cpu.render_flat(res, 4096, 2), cpu.render_dualcontour(res))
    return _state["refs"]


@pytest.mark.parametrize("path", ["octree", "flat", "dualcontour"])
def test_flange_meshes_like_the_oracle(gpu, path):
    s, res, ref_oct, ref_flat, ref_dc = _flange_refs()
    ref = {"octree": ref_oct, "flat": ref_flat, "dualcontour": ref_dc}[path]
    make = {"octree": gpu.OctreeHIP, "flat": gpu.FlatHIP, "dualcontour": gpu.DualContourHIP}[path]
    want = _sorted_bits(ref.tris)
    plain, spec = _pair(gpu, s)
    for kind, sdf in (("interpreter", plain), ("specialised", spec)):
        m = make(sdf, res)
        assert m.n_tris() == ref.n_tris, (path, kind, m.n_tris(), ref.n_tris)
        got = _sorted_bits(m.RenderAll())
        assert got.shape == want.shape and (got == want).all(), (path, kind)
