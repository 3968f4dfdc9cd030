"""The face form of the box-like primitives (interp.h: face2_k / face3_k) on the device.

Helper level (gsdf_hip_selftest_math, one value per lane, 64 consecutive values = one wave): function 18 / 20 -- the form as the ops
run it, max + 0 where the wave's vote passes, the legacy statements otherwise -- against 19 / 21, the legacy statements always, bit for
bit over
  * whole waves that satisfy the condition (the closed form runs),
  * waves in which exactly one lane fails it (the fallback runs for the 63 that would have passed),
  * every combination of +-0, +-subnormal, +-FLT_MIN, +-1, +-FLT_MAX, +-Inf, +-NaN.
At least a quarter of the waves must be of the first kind; that is asserted from the inputs.

Op level: one small tree per touched op -- cylinder, rounded cylinder, box, rounded box, hex prism, extruded rectangle -- as it is at
Diagonal / 48, and with power-of-two dimensions moved by a multiple of a power-of-two step near Diagonal / 48, so that its faces lie
on lattice planes: slab distances of exactly +0 on the faces, mixed waves along edges and corners. Distances over the lattice through
gsdf_hip_eval3 and the octree mesher's triangles and evaluation count (leaf_eval_kernel's column bricks) equal the oracle's bit for
bit, with the interpreter kernels, the per-tree kernels and the per-tree kernels built with -DGSDF_NO_FACE_FORM.
"""
import numpy as np
import pytest

from scaffold.builder import Builder
from oracle.oracle import OracleSDF

from face_points import F, grid, same

pytestmark = pytest.mark.gpu
WAVE = 64


# ---------------------------------------------------------------------------------------------------------------- helper level
def _values(rng, n, positive):
    """n values of every magnitude: positive, or <= 0 (one in eight a zero of either sign)."""
    mag = np.ldexp(1.0 + rng.random(n), rng.integers(-140, 120, n)).astype(F)
    if positive:
        return np.maximum(mag, F(1e-45))
    out = -mag
    z = rng.random(n) < 0.125
    return np.where(z, np.where(rng.random(n) < 0.5, F(0.0), F(-0.0)), out).astype(F)


def _passing(rng, n, one_positive):
    """n operand pairs, both <= 0 or (if allowed) one of the two positive, of any magnitudes."""
    x, y = _values(rng, n, False), _values(rng, n, False)
    if one_positive:
        sel = rng.integers(0, 3, n)
        x = np.where(sel == 1, _values(rng, n, True), x).astype(F)
        y = np.where(sel == 2, _values(rng, n, True), y).astype(F)
    return x, y


def _helper_inputs(third):
    """x, y and the kind of every wave (0 passes whole, 1 one lane fails, 2 the grid) for a given wave-uniform third term (None: two terms)."""
    rng = np.random.default_rng(7)
    # with a positive third term the two others must both be <= 0; with third <= 0 (or none) one of them may be positive
    nw = 512
    x, y = _passing(rng, 2 * nw * WAVE, third is None or third <= 0)
    kind = np.zeros(2 * nw, int)
    kind[nw:] = 1
    for w in range(nw, 2 * nw):  # exactly one lane beyond the edge, every lane position in turn
        i = w * WAVE + (w % WAVE)
        x[i], y[i] = _values(rng, 1, True)[0], _values(rng, 1, True)[0]
    gx, gy = grid(2)
    pad = (-len(gx)) % WAVE
    gx, gy = np.concatenate([gx, np.full(pad, -1, F)]), np.concatenate([gy, np.full(pad, -1, F)])
    kind = np.concatenate([kind, np.full(len(gx) // WAVE, 2)])
    return np.concatenate([x, gx]), np.concatenate([y, gy]), kind


def _wave_passes(x, y, third):
    with np.errstate(invalid="ignore"):
        a, b = x <= 0, y <= 0
        ok = (a | b) if third is None else ((a & b) | ((a | b) & bool(third <= 0)))
    return ok.reshape(-1, WAVE).all(axis=1)


@pytest.mark.parametrize("third", [None, -0.75, -0.0, 0.0, 1e-42, 0.5, float("inf"), float("nan")], ids=str)
def test_new_form_equals_legacy_sequence(gpu, third):
    x, y, kind = _helper_inputs(third)
    assert len(x) <= 1 << 20 and len(x) % WAVE == 0
    passes = _wave_passes(x, y, third)
    # the layout reaches the closed form: at least a quarter of all waves pass whole; the one-lane waves do not
    assert passes[kind == 0].all() and not passes[kind == 1].any()
    assert passes.sum() * 4 >= len(passes), (int(passes.sum()), len(passes))
    new, old = ("face2", "face2_legacy") if third is None else ("face3", "face3_legacy")
    d = 1.0 if third is None else third
    got, want = gpu.math_apply(new, x, y, divisor=d), gpu.math_apply(old, x, y, divisor=d)
    bad = np.flatnonzero(~same(got, want))
    assert bad.size == 0, (third, bad.size, [(int(i), kind[i // WAVE], float(x[i]), float(y[i]), float(got[i]), float(want[i])) for i in bad[:4]])
    # and the closed form is what it says: max + 0 on the waves that pass (finite operands; the device's max drops a NaN)
    if third is None or np.isfinite(third):
        fin = np.repeat(passes, WAVE) & np.isfinite(x) & np.isfinite(y)
        m = np.maximum(x, y) if third is None else np.maximum(np.maximum(x, y), F(third))
        assert same(got[fin], (m[fin] + F(0.0)).astype(F)).all()


# -------------------------------------------------------------------------------------------------------------------- op level
def _trees(b):
    return {"cylinder": b.NewCylinder(1.0, 2.0, 0.0), "rounded-cylinder": b.NewCylinder(1.0, 2.0, 0.25), "box": b.NewBox(1.0, 1.5, 2.0, 0.0),
            "rounded-box": b.NewBox(1.0, 1.5, 2.0, 0.25), "hex-prism": b.NewHexagonalPrism(1.0, 2.0),
            "extruded-rectangle": b.Extrude(b.NewRectangle(1.0, 2.0), 1.5)}


_NAMES = list(_trees(Builder()))
_refs = {}


def _case(name, aligned):
    """(shape, res, lattice points, oracle distances, oracle octree mesh) of a case: computed once, shared, left unchanged."""
    key = (name, aligned)
    if key not in _refs:
        b = Builder()
        s = _trees(b)[name]
        res = F(float(s.Diagonal()) / 48)
        if aligned:  # a power-of-two step and a shift by whole steps: every coordinate stays exact, the faces sit on lattice planes
            res = F(2.0 ** np.round(np.log2(float(res))))
            s = b.Translate(s, float(3 * res), float(-2 * res), float(5 * res))
        bb = np.asarray(s.Bounds(), F)
        org = bb[:3] - F(2) * res
        n = np.ceil((bb[3:] - org) / res).astype(int) + 3
        ax = [(org[a] + np.arange(n[a]).astype(F) * res).astype(F) for a in range(3)]
        pos = np.ascontiguousarray(np.stack(np.meshgrid(*ax, indexing="ij"), -1).reshape(-1, 3), F)
        cpu = OracleSDF(s.tree())
        ref = cpu.Evaluate(pos)
        if aligned:  # the point of the shift: lattice points with a distance of exactly zero
            assert (ref == 0).any(), name
        ref.setflags(write=False)
        pos.setflags(write=False)
        _refs[key] = (s, res, pos, ref, cpu.render_octree(res))
    return _refs[key]


def _sorted_bits(tris):
    t = np.ascontiguousarray(tris, F).reshape(-1, 9).view(np.uint32)
    return t[np.lexsort(t.T[::-1])]


@pytest.mark.parametrize("build", ["interpreter", "per-tree", "per-tree-legacy"])
@pytest.mark.parametrize("aligned", [False, True], ids=["as-is", "on-lattice"])
@pytest.mark.parametrize("name", _NAMES)
def test_touched_ops_equal_the_oracle(gpu, monkeypatch, name, aligned, build):
    s, res, pos, ref, ref_mesh = _case(name, aligned)
    sdf = gpu.SDF3HIP(s)
    if build != "interpreter":
        if build == "per-tree-legacy":
            monkeypatch.setenv("GSDF_HIP_SPEC_FLAGS", "-DGSDF_NO_FACE_FORM")
        else:
            monkeypatch.delenv("GSDF_HIP_SPEC_FLAGS", raising=False)
        sdf.specialize()
    assert sdf.info()["specialized"] == (build != "interpreter"), sdf.info()["kernels"]
    got = sdf.Evaluate(pos)
    bad = np.flatnonzero(~same(got, ref))
    assert bad.size == 0, (name, build, bad.size, pos[bad[:4]].tolist(), got[bad[:4]].tolist(), ref[bad[:4]].tolist())
    m = gpu.OctreeHIP(sdf, res)
    assert m.n_tris() == ref_mesh.n_tris and int(m.stats.evals) == ref_mesh.evals, (name, build, m.n_tris(), ref_mesh.n_tris, int(m.stats.evals), ref_mesh.evals)
    tg, tc = _sorted_bits(m.RenderAll()), _sorted_bits(ref_mesh.tris)
    assert tg.shape == tc.shape and (tg == tc).all(), (name, build)
