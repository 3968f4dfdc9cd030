"""The late indexed-mesh passes on the device across float32 magnitudes: adaptive simplification, clean, projection and deviation,
rays and thickness, mass -- each held as bytes to the twin of its contract through the neighbouring files' own helpers
(test_gpu_simplify_adaptive.check, test_gpu_clean.check, test_gpu_project.check, test_gpu_ray.check_rays / check_thickness,
test_gpu_mass.check_mesh, test_gpu_topo.check_against_twin: dry runs and evaluation counters included). No tolerance anywhere.

  (a) On MC_RUNGS, two scaled_corpus.mesh_shapes (a difference, the extruded polygon) at res = base diagonal / 32 times u, every
      length among the options times u (tests/test_scale_late_ref.py: indexed_opts): the welded mesh through simplify_adaptive (four
      levels), clean(merge) of from_soup(RenderAll()), project and deviation of the simplified mesh, raycast of 300 corner rays,
      thickness, mass -- each against its twin on that run's OWN arrays, since two welds of one tree differ in their last bits
      (the comment above _chain in tests/test_gpu_scale.py).
      Against the base rung, in the forms that do not depend on a run's order: the rays (no mesh is involved) bit for bit; the cleaned
      soup as the sorted set of its triangles' coordinates; the welded mesh by its keyed vertices and faces over keys
      (test_gpu_scale._keyed); and every mesh pass once more on the BASE rung's arrays times u (IndexedHIP.from_arrays), where
      the twins are covariant bit for bit (test_scale_late_ref.py: INDEXED_COVARIANT and the test on exactly scaled arrays).
  (b) Array meshes with the exponent at 128 and at -125 (the mass test's construction): the sphere, the box and
      test_gpu_clean.contended_soup() through simplify_adaptive, clean, report and mass against the twins.

Time, one run on one MI355X machine: this file 1.5 s (18 cases). Per case: a rung of (a) 0.05 s for one shape (both sets of passes
with their twins; the base rung of both shapes 0.07 s); (b) 0.02 s, the soup 0.3 s (its twins).

Sensitivity, tried once on scratch copies (none committed); test_gpu_simplify_adaptive, _clean, _project and _ray passed with each:
  the host's 2^(30-e) of adaptive_sum_kernel made in float32                    (b) sphere and soup at -125 (nothing clusters: the scale is +Inf)
  clean_word taking every subnormal for 0                                       (b) sphere and soup at -125
  project_kernel calling s < 1e-12 FLAT                                         (a) both shapes at 2^-20 (projection)
  ray_kernel calling s > 1e12 FLAT                                              (a) both shapes at 2^30 and 2^40 (thickness)
  ray_kernel taking |d| < 1e-9 for a hit whatever tol is                        (a) both shapes at 2^-20 (thickness)
"""
import numpy as np
import pytest

import cleanref as K
import scaled_corpus as SC
import test_scale_late_ref as L
import toporef as T
from oracle.oracle import OracleSDF
from scaffold.builder import Builder
from test_gpu_clean import check as clean_check
from test_gpu_clean import raw
from test_gpu_mass import check_mesh
from test_gpu_project import check as project_check
from test_gpu_ray import check_rays, check_thickness
from test_gpu_scale import _keyed
from test_gpu_simplify_adaptive import check as adaptive_check
from test_gpu_topo import check_against_twin as report_check
from test_scale_ref import MC_RUNGS

pytestmark = pytest.mark.gpu
F = np.float32


def sorted_triangles(v, i):
    """An indexed mesh as the sorted rows of its triangles' nine coordinates: independent of vertex numbering and face order."""
    t = np.ascontiguousarray(v[i.astype(np.int64)].reshape(-1, 9), F)
    return t[np.lexsort(t.view(np.uint32).T[::-1])]


def mesh_passes(gpu, ix, v, i, key, sdf, cpu, res, origin, what):
    """simplify_adaptive, project and deviation of its result, thickness and mass on one handle, each against its twin on (v, i, key).
    Returns what two rungs are compared by."""
    o = L.indexed_opts(res)
    simp, st, tw = adaptive_check(gpu, ix, v, i, key, origin=origin, **o["adaptive"])
    assert simp is not None and st.n_tris < st.n_tris_in and sum(st.chosen[1:]) > 0, what
    sv, si, sk = simp.read()
    proj, pst, ptw = project_check(simp, sdf, cpu.Evaluate, sv, (what, "project"), **o["project"])
    _, zero, _ = project_check(simp, sdf, cpu.Evaluate, sv, (what, "no trips"), **{**o["project"], "max_iters": 0})
    dv = simp.deviation(sdf, o["project"]["tol"])
    assert dv.result_bytes() == zero.result_bytes(), what
    th = check_thickness(simp, sdf, cpu.Evaluate, sv, (what, "thickness"), **o["thickness"])
    _, total, shells, _ = check_mesh(gpu, v, i, (what, "mass"), ix)
    return {"simplified": (sv, si, sk), "max_err": st.max_err, "exponent": st.exponent, "projected": (proj.read()[0],) + proj.fit(), "thickness": th[:2],
            "evals": (pst.evals, th[2].evals), "mass": (total, shells)}


def passes_differ(base, got, k):
    bad = [("simplified", x) for x in L.mesh_differ(base["simplified"], got["simplified"], k)]
    bad += [("max_err",)] * int(float(np.ldexp(base["max_err"], k)) != got["max_err"]) + [("exponent",)] * int(got["exponent"] != base["exponent"] + k)
    bad += [("project", x) for x in L.project_differ(base["projected"], got["projected"], k)] + [("thickness", x) for x in L.thickness_differ(base["thickness"], got["thickness"], k)]
    bad += [("evals",)] * (base["evals"] != got["evals"]) + [("mass", x) for x in L.mass_differ(base["mass"][0], got["mass"][0], k)]
    return bad + [("mass", "shell", x) for b, g in zip(base["mass"][1], got["mass"][1]) for x in L.mass_differ(b, g, k)]


def rung(gpu, name, k, base=None):
    """Everything of (a) for one shape at u = 2^k; base: the base rung's result, to be compared against."""
    u = SC.unit(k)
    what = (name, k)
    sh = dict(SC.mesh_shapes(Builder(), u)[1])[name]
    sdf, cpu = gpu.SDF3HIP(sh), OracleSDF(sh.tree())
    res = F(F(float(dict(SC.mesh_shapes(Builder(), 1.0)[1])[name].Diagonal()) / 32) * F(u))
    oc = gpu.OctreeHIP(sdf, res, payload=gpu.PAYLOAD_RECORDS)
    ix = oc.weld()
    v, i, key = ix.read()
    assert len(i) > 1000 and len(np.unique(key)) == len(key), what
    origin = tuple(F(x) - F(0.5) * res for x in oc.stats.origin[:])
    out = {"res": res, "origin": origin, "welded": (v, i, key), "own": mesh_passes(gpu, ix, v, i, key, sdf, cpu, res, origin, what)}
    # the soup of the plain mesher, joined
    tris = gpu.OctreeHIP(sdf, res).RenderAll().reshape(-1, 3, 3)
    sv, si = tris.reshape(-1, 3), np.arange(3 * len(tris), dtype=np.uint32).reshape(-1, 3)
    soup = gpu.IndexedHIP.from_arrays(sv, si)
    cleaned, cst, _ = clean_check(gpu, soup, sv, si, None, None, K.MERGE_POSITIONS)
    joined, jst = gpu.IndexedHIP.from_soup(tris)
    assert raw(*joined.read()) == raw(*cleaned.read()) and jst.result_bytes() == cst.result_bytes() and cst.merged_verts > 0, what
    out["soup"] = sorted_triangles(*cleaned.read()[:2])
    # rays: no mesh is involved
    o0, r0 = L.corner_rays(dict(SC.mesh_shapes(Builder(), 1.0)[1])[name].Bounds())
    dev_rays, _ = check_rays(gpu, sdf, cpu.Evaluate, L.times(o0, k), r0, (what, "rays"), **L.indexed_opts(res)["rays"])
    out["rays"] = dev_rays
    assert dev_rays[4].count[1] + dev_rays[4].count[2] > 100, what         # HIT, CROSSED
    if base is not None:
        assert k in L.INDEXED_COVARIANT
        assert L.rays_differ(base["rays"], dev_rays, k) == [] and base["rays"][4].evals == dev_rays[4].evals, what
        assert L.times(base["soup"], k).tobytes() == out["soup"].tobytes(), (what, "the cleaned soup")
        (key0, _, f0), (key1, _, f1) = _keyed(*base["welded"]), _keyed(v, i, key)
        assert key0.tobytes() == key1.tobytes() and f0.tobytes() == f1.tobytes(), (what, "weld: keyed vertices, faces over keys")
        # the base rung's arrays times u: every pass again, against its twin and against the base rung bit for bit
        v0, i0, key0 = base["welded"]
        vs = L.times(v0, k)
        assert L.is_exact(v0, k)
        scaled = gpu.IndexedHIP.from_arrays(vs, i0, key0)
        again = mesh_passes(gpu, scaled, vs, i0, key0, sdf, cpu, res, tuple(L.length(x, k) for x in base["origin"]), (what, "the base rung's arrays times u"))
        assert passes_differ(base["own"], again, k) == [], what
    return out


@pytest.fixture(scope="module")
def base_rung(gpu):
    return {name: rung(gpu, name, 0) for name in L.INDEXED_SHAPES}


@pytest.mark.parametrize("k", MC_RUNGS)
@pytest.mark.parametrize("name", L.INDEXED_SHAPES)
def test_indexed_passes_on_the_ladder(gpu, base_rung, name, k):
    rung(gpu, name, k, base_rung[name])


# ---- (b) the ends of the exponent range
@pytest.mark.parametrize("top", L.ARRAY_TOPS)
@pytest.mark.parametrize("name", ["sphere", "box", "soup"])
def test_array_meshes_at_the_ends_of_the_exponent_range(gpu, name, top):
    v, i, cell, tol = L.array_meshes()[name]
    s, k, exact = L.mesh_at(v, top)
    assert T.exponent_of(s) == top and exact == (top == 128 or name == "box")
    ix = gpu.IndexedHIP.from_arrays(s, i)
    simp, st, tw = adaptive_check(gpu, ix, s, i, None, L.length(cell, k), L.length(tol, k), L.ADAPTIVE_LEVELS)
    assert simp is not None and st.exponent == top and np.isfinite(st.max_err) and np.isfinite(simp.read()[0]).all()
    for flags in (K.MERGE_POSITIONS, K.FACES, L.CLEAN_FLAGS):
        cleaned, cst, _ = clean_check(gpu, ix, s, i, None, None, flags)
        assert cleaned is not None
    rep, _ = report_check(ix, s, i)
    assert rep.exponent == top
    report_check(simp, tw[0], tw[1])
    report_check(cleaned, *cleaned.read()[:2])
    if name != "soup":                              # (the soup's faces are no surface: the mass test's shapes are closed meshes)
        _, total, _, _ = check_mesh(gpu, s, i, (name, top), ix)
        assert total["exponent"] == top and np.isfinite(total["second"]).all()
    if top == 128:
        # covariant with the unscaled mesh (test_scale_late_ref.py): the device's own results of both
        base, _, _ = adaptive_check(gpu, gpu.IndexedHIP.from_arrays(v, i), v, i, None, F(cell), F(tol), L.ADAPTIVE_LEVELS)
        assert L.mesh_differ(base.read(), simp.read(), k) == [], name
