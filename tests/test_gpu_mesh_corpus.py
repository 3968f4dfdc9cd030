"""Every node type through the meshers on the device: the family of tests/mesh_corpus.py (the 3-D corpus, the 2-D corpus extruded and
revolved, arrays whose child sits off its cell or sector, two screws in one column brick, a gated circular array) through
test_gpu_variants._mesh_checks -- octree with its options, records welded and marched, the flat renderer, dual contouring as soup
and indexed, normals, render3, projection -- once through the interpreter's K = 4 kernels (leaf_eval_kernel<4,3>, the kernels every
real part and the benchmark use) and once through kernels specialised per tree. Beyond _mesh_checks, at the family's own resolution:
TotalPruned against the oracle under every octree option, share_corners = 3, chiseled dual contouring for the 3-D corpus, the
off-seam arrays at Diagonal / 83 too, and the records' distances for the two-screw trees.

That the centre tests are RIGHT (not only the oracle's) is tests/test_mesh_corpus_ref.py's business: oracle and device take the same
decisions cube for cube, wrong ones too.

Time, one run on one MI355X machine: this file 131 s (32 cases), the rest of the GPU suite beside it (364 cases) 632 s. Per case:
ten trees through the interpreter 0.35-2.2 s; eight trees built side by side (tests/par.py, 12 workers) and checked through their own
kernels 4-8 s, the two groups that hold the polygon-heavy programs (translatemulti, the thread outlines) 10 and 13 s -- one such build
alone is a compiler run of 7 s.
"""
import numpy as np
import pytest

import mesh_corpus as MC
import par
from oracle.oracle import OracleSDF
from test_gpu_lattice import check_records
from test_gpu_variants import _mesh_checks, _same_tris

pytestmark = pytest.mark.gpu

NAMES = list(MC.NAMES)
CORPUS3D = set(MC.CORPUS3D)
INTERP_GROUP, SPEC_GROUP = 10, 8
IGROUPS = [NAMES[i:i + INTERP_GROUP] for i in range(0, len(NAMES), INTERP_GROUP)]
SGROUPS = [NAMES[i:i + SPEC_GROUP] for i in range(0, len(NAMES), SPEC_GROUP)]
OPTIONS = ({}, {"prune": False}, {"share_corners": 1}, {"share_corners": 2}, {"share_corners": 3})
K4_LEAF = "leaf_eval_kernel<4,3>"


def _octrees(gpu, name, sh, sdf, res, how):
    """The octree under every option at `res`: the oracle's triangles and its count of pruned cubes."""
    cpu = OracleSDF(sh.tree())
    want = {True: cpu.render_octree(res, 4096, True), False: cpu.render_octree(res, 4096, False)}
    for kw in OPTIONS:
        m = want[kw.get("prune", True)]
        oc = gpu.OctreeHIP(sdf, res, **kw)
        _same_tris(oc.RenderAll(), m.tris, (name, how, "octree", kw, float(res)))
        assert oc.TotalPruned() == m.pruned, (name, how, "TotalPruned", kw, float(res), oc.TotalPruned(), m.pruned)
    return cpu, want[True]


def _tree_checks(gpu, name, sh, sdf, how):
    _mesh_checks(gpu, name, sh, sdf, (name, how))
    res = MC.res_of(name, sh)
    cpu, m = _octrees(gpu, name, sh, sdf, res, how)
    assert m.n_tris > 100, (name, m.n_tris)
    if name in CORPUS3D:
        _same_tris(gpu.DualContourHIP(sdf, res, chiseled=True).RenderAll(), cpu.render_dualcontour(res, True).tris, (name, how, "dual contouring", "chiseled"))
    if MC.off_seam(name):
        _octrees(gpu, name, sh, sdf, MC.res_of(name, sh, 83), how)
    if name.startswith("twoscrew_"):
        rec = gpu.OctreeHIP(sdf, res, payload=gpu.PAYLOAD_RECORDS)
        check_records(rec, cpu, (name, how, "records"))


@pytest.mark.parametrize("group", range(len(IGROUPS)))
def test_corpus_meshes_through_the_interpreter(gpu, group):
    d = MC.meshes()
    for name in IGROUPS[group]:
        sh = d[name][0]
        sdf = gpu.SDF3HIP(sh)
        info = sdf.info()
        # (every tree of the family has at most 11 slots: four points per lane)
        assert info["lds_slots"] <= 11 and info["kernels"]["leaf"] == K4_LEAF + ":interpreter" and info["kernels"]["prune"] == "prune_kernel:interpreter", (name, info)
        _tree_checks(gpu, name, sh, sdf, "interpreter")


@pytest.mark.parametrize("group", range(len(SGROUPS)))
def test_corpus_meshes_through_specialised_kernels(gpu, group):
    d = MC.meshes()

    def check(name):                                         # (one build per tree: side by side, tests/par.py)
        sh = d[name][0]
        sdf = gpu.SDF3HIP(sh)
        try:
            sdf.specialize()
        except gpu.HipError as e:
            return name, str(e)[:200]
        if not sdf.info()["specialized"]:
            return name, "specialized is false"
        kern = sdf.info()["kernels"]
        # (an entry point whose specialised kernel would need scratch keeps the interpreter's: rev_poly's prune_kernel does)
        assert any(v.endswith(":specialised") for v in kern.values()), (name, kern)
        _tree_checks(gpu, name, sh, sdf, "specialised")
        return None
    refused = [r for r in par.pmap(check, SGROUPS[group], workers=12) if r]
    assert not refused and len(refused) + len(MC.OMITTED) <= MC.MAX_OMITTED, ("builds refused", refused)
