"""The meshed corpus (tests/mesh_corpus.py) on the host: which instructions its programs hold, that the interval evaluation of
the octree's centre tests bounds every tree's field over the ball, and that the default octree drops no surface.

The device is compared with the oracle cube for cube (tests/test_gpu_mesh_corpus.py), so a centre test that is wrong in both
is green there; here the oracle's bounds are compared with the field itself, and its pruned octree with its unpruned one. Arrays
whose child sits off its cell or sector (mesh_corpus.offseam_trees) lost up to a quarter of their triangles while the seams of
array nodes were taken as continuous (include/gsdf_seams.h)."""
import numpy as np
import pytest

import mesh_corpus as MC
from gsdf_amd import hip
from oracle.oracle import OracleSDF
from scaffold.builder import Builder
from test_lowering import FLAG_HXY, FLAG_SHXY, FLAG_SHZ, decode
from test_prune_bounds import _violations

GROUP = 12
NAMES = [n for n, _ in MC.family(Builder())]
GROUPS = [NAMES[i:i + GROUP] for i in range(0, len(NAMES), GROUP)]
OFF_SEAM = [n for n in NAMES if MC.off_seam(n)]


def _sorted_bits(t):
    t = np.ascontiguousarray(t, np.float32).reshape(-1, 9)
    return t[np.lexsort(t.view(np.uint32).T[::-1])].view(np.uint32)


def _sign_violations(o, rng, ncentres=200, nsamp=48, fracs=(0.01, 0.05, 0.2)):
    """The decision the octree takes from the bounds, on test_prune_bounds._violations' sampling and with its tolerance: centres
    whose cube would be dropped (lo >= 0 or hi <= 0) although a sampled point of the ball has the other sign."""
    bb = o.bb
    ext = bb[3:] - bb[:3]
    bad = 0
    for fr in fracs:
        h = np.float32(fr * ext.max())
        c = (bb[:3] + rng.uniform(-0.1, 1.1, (ncentres, 3)) * ext).astype(np.float32)
        lo, hi = o.EvaluateBounds(c, h)
        d = rng.normal(size=(ncentres, nsamp, 3))
        d /= np.linalg.norm(d, axis=2, keepdims=True)
        rad = h * rng.uniform(0, 1, (ncentres, nsamp, 1)) ** (1 / 3)
        rad[:, : nsamp // 4] = h * 0.999
        pts = (c[:, None, :] + d * rad).astype(np.float32).reshape(-1, 3)
        f = o.Evaluate(pts).reshape(ncentres, nsamp)
        tol = 1e-4 * (np.abs(f) + h + 1)
        bad += int((((lo >= 0)[:, None] & (f < -tol)) | ((hi <= 0)[:, None] & (f > tol))).any(axis=1).sum())
    return bad


def test_family_caps_and_node_types():
    """mesh_corpus.meshes() asserts them: at most six trees left out, each with its reason, and every one of the 53 node types in
    a tree meshed with more than 100 triangles."""
    m = MC.meshes()
    assert len(MC.OMITTED) <= 6 and all(MC.OMITTED.values())
    assert len(MC.NODE_TYPES) == 53
    ops = set()
    for name, (sh, _, mesh) in m.items():
        if mesh.n_tris > 100:
            ops |= MC.ops_of(sh)
    assert ops == set(MC.NODE_TYPES), sorted(set(MC.NODE_TYPES) - ops)
    assert all(mesh.n_tris > 100 for _, _, mesh in m.values()), sorted(n for n, v in m.items() if v[2].n_tris <= 100)


def test_census_of_the_lowered_programs():
    """Instructions with bodies of their own on the leaf kernels' path, under the flags that select those bodies."""
    b = Builder()
    seen = set()
    for name, sh in MC.family(b):
        code, _ = hip.lower(sh)
        for ins in decode(code):
            w = int(code[ins[4]])
            seen.add((ins[0], "any"))
            for flag, fl in ((FLAG_SHXY, "shxy"), (FLAG_SHZ, "shz"), (FLAG_HXY, "hxy")):
                if w & flag:
                    seen.add((ins[0], fl))
    want = [(n, "shxy") for n in ("D_TORUS", "D_CYL0", "D_CYLR", "D_CIRCLE2D", "D_SCREW_PRE", "D_CIRC_PRE")] + [("D_TWIST", "shz")] + \
           [(n, "any") for n in ("D_GATEZC", "D_GATEOB", "D_SKIP", "D_LIP_WRAP", "D_LIP_SEAM", "D_ARRAY_PRE", "D_ARRAY2D_PRE")]
    assert [w for w in want if w not in seen] == []
    assert any(fl == "hxy" for _, fl in seen)


def test_seam_instruction_only_where_a_seam_may_jump():
    """D_LIP_SEAM is emitted for the arrays whose child is off its cell or sector and for circular arrays with fewer instances than
    divisions, not for the arrays whose seams include/gsdf_seams.h proves continuous: a box repeated about its own centre, the
    knurled cylinder's cutters (a square bar turned a quarter of pi, mirror symmetric in its sector's ray), a full circle of copies."""
    b = Builder()
    d = dict(MC.family(b))

    def count(sh):
        code, _ = hip.lower(sh)
        return [i[0] for i in decode(code)].count("D_LIP_SEAM")
    assert count(d["array"]) == 0 and count(b.Scene("knurled-cylinder")) == 0
    box = b.Translate(b.NewBox(1, 0.61, 0.8, 0.3), 1.5, 0, 0)
    assert count(b.CircularArray(box, 9, 9)) == 0 and count(b.CircularArray(box, 2, 9)) == 0 and count(b.CircularArray(box, 4, 9)) == 1
    assert count(b.Array(b.NewTorus(0.5, 0.1), 0.4, 0.4, 0.4, 3, 1, 1)) == 1       # symmetric but not convex: the end cells
    assert count(b.Array(b.NewTorus(0.5, 0.1), 0.4, 0.4, 0.4, 1, 1, 1)) == 0       # one cell: no seam
    for n in OFF_SEAM:
        assert count(d[n]) >= 1, n


@pytest.mark.parametrize("name", ["offseam_array", "offseam_ext_array2d", "circ_gated"])
def test_specialised_kernels_with_a_seam_instruction_build(name):
    """The specialised build of a program that holds D_LIP_SEAM (3-D cells, 2-D cells, sector rays behind the gate) compiles for
    gfx950 without a device: the generator emits the interpreter's own text for it."""
    import ctypes as C
    t = dict(MC.family(Builder()))[name].tree()
    n = C.c_size_t()
    assert hip.lib().gsdf_hip_specialize_check(C.byref(t), C.byref(n)) == 0, hip.lib().gsdf_hip_last_error().decode()[:2000]
    assert n.value > 10000


@pytest.mark.parametrize("group", range(len(GROUPS)))
def test_bounds_hold_over_the_ball(group):
    b = Builder()
    d = dict(MC.family(b) + MC.bounds_only(b))
    names = GROUPS[group] + ([n for n, _ in MC.bounds_only(b)] if group == len(GROUPS) - 1 else [])
    for k, name in enumerate(names):
        o = OracleSDF(d[name].tree())
        assert _violations(o, np.random.default_rng(1000 + 31 * group + k)) <= 0, name
        assert _sign_violations(o, np.random.default_rng(2000 + 31 * group + k)) == 0, name


@pytest.mark.parametrize("group", range(len(GROUPS)))
def test_default_octree_drops_nothing(group):
    m = MC.meshes()
    for name in GROUPS[group]:
        sh, res, pruned = m[name]
        o = OracleSDF(sh.tree())
        full = o.render_octree(res, 4096, False)
        assert pruned.n_tris == full.n_tris and (_sorted_bits(pruned.tris) == _sorted_bits(full.tris)).all(), (name, pruned.n_tris, full.n_tris)
        if name not in MC.FLAT_DIFFERS:
            assert o.render_flat(res, 4096, 2).n_tris == full.n_tris, name


@pytest.mark.parametrize("div", MC.OFF_SEAM_DIVS)
def test_off_seam_arrays_keep_their_surface_at_other_resolutions(div):
    b = Builder()
    d = dict(MC.family(b))
    for name in OFF_SEAM:
        sh = d[name]
        o = OracleSDF(sh.tree())
        res = MC.res_of(name, sh, div)
        pruned, full = o.render_octree(res, 4096, True), o.render_octree(res, 4096, False)
        assert full.n_tris > 100, (name, div)
        assert pruned.n_tris == full.n_tris and (_sorted_bits(pruned.tris) == _sorted_bits(full.tris)).all(), (name, div, pruned.n_tris, full.n_tris)
        assert pruned.pruned > 0, (name, div)


def test_fuzz_tree_that_lost_surface_at_a_sector_seam():
    """tests/fuzz_trees.py seed 1, tree 2 (meshed on the device by test_gpu_fuzz.py at Diagonal / 48) holds circular arrays whose
    children are not mirror symmetric in their rays: with the seams taken as continuous the pruned octree had 3 049 of the 3 085
    triangles that the unpruned octree and the flat renderer give; oracle and device agreed on the loss."""
    import fuzz_trees
    sh = fuzz_trees.random_shapes(1, 14, depth=4)[1][2]
    assert MC.ops_of(sh) >= {"CIRCARRAY", "CIRCARRAY2D"}
    assert [i[0] for i in decode(hip.lower(sh)[0])].count("D_LIP_SEAM") >= 1
    o = OracleSDF(sh.tree())
    res = np.float32(float(sh.Diagonal()) / 48)
    pruned, full = o.render_octree(res, 4096, True), o.render_octree(res, 4096, False)
    assert pruned.n_tris == full.n_tris == o.render_flat(res, 4096, 2).n_tris == 3085
    assert (_sorted_bits(pruned.tris) == _sorted_bits(full.tris)).all() and pruned.pruned > 0
