"""Lattice-aligned fields with exact zeros (tests/lattice_trees.py) through every marching path of the device, against the oracle
bit for bit: mcInterpolate's snap, t = 0.5 and -0.0 branches in the record marchers (march_vertex, per wave and per workgroup), the
corner-sharing leaf kernels, the flat renderer's own marching (mc_interp), the weld's lattice-point keys, and the same again through
the kernels specialised per tree. Then what a degenerate field hands downstream: zero-area triangles in the STL writer, faces with
repeated indices and non-manifold edges in the report, extract and simplify kernels, simplify's grid ON the lattice planes.

tests/test_lattice_ref.py shows on the CPU that the families reach these branches in numbers and that twin and oracle agree there."""
import numpy as np
import pytest

import lattice_trees as L
import toporef as T
import weldref as W
from oracle import oracle
from oracle.oracle import OracleSDF
from scaffold.builder import Builder
from test_gpu_gather import _loopback_world
from test_gpu_simplify import check as check_simplify
from test_gpu_topo import check_against_twin as check_report
from test_gpu_weld import check_against_twin as check_weld

pytestmark = pytest.mark.gpu

NAMES = [f"spheres{s}" for s in range(4)] + ["boxes" + v for v in L.BOX_VARIANTS] + ["both_tiny", "boxeszero@5"]
REDUCED = "spheres0/7"       # spheres seed 0 over a 7^3 block of centres: the member small enough to compile at run time
SPECIALISED = ["boxes" + v for v in L.BOX_VARIANTS] + ["both_tiny", REDUCED]
_b = Builder()
_members = {}
_ref = {}


def member(name):
    if not _members:
        _members.update(L.members(_b))
        _members[REDUCED] = (L.spheres(_b, 0, block=7), np.float32(2.0 ** -3))
    return _members[name]


class Ref:
    """The oracle's meshes of a member, made once: octree (pruned, unpruned) and flat, sorted by bits."""

    def __init__(self, name):
        self.shape, self.res = member(name)
        self.cpu = OracleSDF(self.shape.tree())
        oc = self.cpu.render_octree(self.res, 4096, True)
        self.levels, self.n_pruned, self.pruned = oc.levels, oc.pruned, L.sorted_bits(oc.tris)
        self.unpruned = L.sorted_bits(self.cpu.render_octree(self.res, 4096, False).tris)
        fl = self.cpu.render_flat(self.res, 4096, 2)
        self.flat, self.flat_evals = L.sorted_bits(fl.tris), fl.evals
        assert len(self.pruned) > 1000 and (self.flat == self.unpruned).all()
        if name == "boxeszero@5":   # the centre tests tie their threshold exactly here and drop point triangles (test_lattice_ref.py)
            assert len(self.unpruned) - len(self.pruned) == 7
        elif name != REDUCED:
            assert (self.pruned == self.unpruned).all()


def ref(name):
    if name not in _ref:
        _ref[name] = Ref(name)
    return _ref[name]


def same(mesh, want, what):
    got = L.sorted_bits(mesh.RenderAll())
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero((got != want).any(axis=1))
    assert len(bad) == 0, (what, len(bad), got[bad[:3]].view(np.float32), want[bad[:3]].view(np.float32))


def check_records(oc, cpu, what):
    """The records of a records mesh against the oracle at the leaves' corners: the eight distances' bits and the case byte."""
    dist, leaves, case = oc.records()
    origin, res = np.array(oc.stats.origin[:], np.float32), np.float32(oc.stats.res)
    want = cpu.Evaluate(W.leaf_corners(leaves, origin, res).reshape(-1, 3)).reshape(-1, 8)
    assert len(dist) == int(oc.stats.cut_leaves) > 0 and len(np.unique(leaves, axis=0)) == len(leaves), what
    assert (dist.view(np.uint32) == want.view(np.uint32)).all(), what     # -0.0 stays -0.0, 1e-13 stays 1e-13
    wcase = ((want < 0) * (1 << np.arange(8))).sum(axis=1)
    assert (case == wcase).all() and ((case != 0) & (case != 255)).all(), what


def check_paths(gpu, name, specialised):
    R = ref(name)
    sh, res = R.shape, R.res
    sdf = gpu.SDF3HIP(sh)
    if specialised:
        sdf.specialize()
        print(name, "specialised in", sdf.info()["specialize_s"], "s")
    oc = gpu.OctreeHIP(sdf, res)
    print(name, "kernels", sdf.info()["kernels"], "triangles", oc.n_tris(), "cut leaves", int(oc.stats.cut_leaves))
    assert oc.stats.levels == R.levels and tuple(oc.stats.origin[:]) == L.ORIGIN and oc.stats.res == res
    same(oc, R.pruned, "default")
    assert oc.TotalPruned() == R.n_pruned
    same(gpu.OctreeHIP(sdf, res, prune=False), R.unpruned, "prune=False")
    for sc in (1, 2, 3):
        m = gpu.OctreeHIP(sdf, res, share_corners=sc)
        same(m, R.pruned, f"share_corners={sc}")
        assert m.TotalPruned() == R.n_pruned
    for sc in (0, 1, 2):
        rec = gpu.OctreeHIP(sdf, res, share_corners=sc, payload=gpu.PAYLOAD_RECORDS)
        assert rec.payload()[0] == gpu.PAYLOAD_RECORDS and rec.n_tris() == len(R.pruned)
        check_records(rec, R.cpu, f"records share_corners={sc}")
        same(rec.march(), R.pruned, f"records share_corners={sc} marched")
    for world in (2, 3):
        parts = [gpu.OctreeHIP(sdf, res, shard_rank=r, shard_count=world) for r in range(world)]
        got = L.sorted_bits(np.concatenate([p.RenderAll() for p in parts]))
        assert got.shape == R.pruned.shape and (got == R.pruned).all(), f"shards of {world}"
    fl = gpu.FlatHIP(sdf, res)
    same(fl, R.flat, "flat")
    assert fl.Evaluations() == R.flat_evals

    def work(r, comm):        # march_dense_kernel over both ranks' records
        mine_sdf = gpu.SDF3HIP(sh)
        if specialised:
            mine_sdf.specialize()
        mine = gpu.OctreeHIP(mine_sdf, res, shard_rank=r, shard_count=2, payload=gpu.PAYLOAD_RECORDS)
        g, counts, gs = mine.gatherv_start(comm, gpu.GATHER_ALL, 0).wait()
        got = L.sorted_bits(g.RenderAll())
        return sum(counts), got.shape == R.pruned.shape and bool((got == R.pruned).all())

    assert _loopback_world(gpu, 2, work) == [(len(R.pruned), True)] * 2


@pytest.mark.parametrize("name", NAMES)
def test_every_marching_path_matches_the_oracle(gpu, name):
    check_paths(gpu, name, specialised=False)


@pytest.mark.parametrize("name", SPECIALISED)
def test_every_marching_path_matches_the_oracle_specialised(gpu, name):
    """The same through the kernels compiled for the tree at run time (built with -fno-honor-nans: the snap and 0.5 branches must
    survive that). The run-time compile is the cost of these cases. Measured on an MI355X host with a cold code-object cache: the
    box variants and both_tiny 1.0-1.2 s in specialize() and 4.2-4.9 s per case; the reduced sphere member (137 spheres)
    17.8 s in specialize() and 92.6 s for the case, the rest being the builds that share_corners = 1 and 2 and the flat renderer
    start on first use. The interpreter cases above take 0.03-1.3 s each."""
    check_paths(gpu, name, specialised=True)


DOWNSTREAM = ["spheres0", "boxeszero"]


@pytest.mark.parametrize("name", DOWNSTREAM)
def test_weld_topology_extract_simplify(gpu, name):
    R = ref(name)
    sh, res = R.shape, R.res
    # weld: vertices, indices and keys equal to the twin's on the device's records, before and after the march
    v, i, k = check_weld(gpu, sh, res)
    kind3 = int((k >> np.uint64(60) == 3).sum())
    c = L.census(R.cpu, sh, res)     # independent of the device's records: every leaf of the lattice (nothing is pruned at 2^-3)
    assert kind3 == len(np.unique(c["keys"][c["keys"] >> np.uint64(60) == 3])) > 0
    print(name, "vertices", len(v), "of them lattice points", kind3, "faces", len(i))
    # topology: this is degenerate and non-manifold input from a real mesher run, and the twin says so
    sdf = gpu.SDF3HIP(sh)
    ix = gpu.OctreeHIP(sdf, res, payload=gpu.PAYLOAD_RECORDS).weld()
    v, i, k = ix.read()              # (this mesh's own: the mesher's record order, and with it the numbering, may differ from run to run)
    rep, tw = check_report(ix, v, i)
    assert tw["report"]["degenerate"] > 0 and tw["report"]["closed_oriented"] == 0
    if name == "spheres0":           # (spheres touching at lattice points; the box family's faces with repeated indices leave a manifold)
        assert tw["report"]["nonmanifold_edges"] > 0
    print(name, {f: tw["report"][f] for f in ("degenerate", "nonmanifold_edges", "boundary_edges", "misoriented_edges", "n_shells", "used_verts")})
    # extract, with and without the degenerate faces
    for drop in (True, False):
        ex = ix.extract(drop_degenerate=drop)
        tv, ti, tk, _ = T.extract(v, i, k, None, tw["shell_of_face"], None, drop)
        v2, i2, k2 = ex.read()
        assert v2.shape == tv.shape and (v2.view(np.uint32) == tv.view(np.uint32)).all() and (i2 == ti).all() and (k2 == tk).all()
        assert ex.n_tris == len(i) - (tw["report"]["degenerate"] if drop else 0)
        check_report(ex, tv, ti)
    # simplify with the grid ON the lattice planes: every snapped vertex sits exactly on a cell boundary (floor of an integer)
    cell = np.float32(2) * res
    on_boundary = int((np.mod((v.astype(np.float64) + 1.0) / float(cell), 1.0) == 0).any(axis=1).sum())
    assert on_boundary > 100
    dev, st, tws = check_simplify(gpu, ix, v, i, cell, L.ORIGIN)
    assert dev is not None and st.n_tris > 0 and st.degenerate_in == tw["report"]["degenerate"]
    check_report(dev, tws[0], tws[1])
    print(name, "simplify: vertices on a cell boundary", on_boundary, "faces", st.n_tris_in, "->", st.n_tris, "clusters", st.cells)


def nan_rule(got, want, what):
    """float32 arrays equal under the contract's rule for 0/0 and Inf * 0: NaN where `want` is NaN (sign and payload unspecified:
    the reference's own differ between amd64 and arm64), else the same bits. Returns the number of NaN."""
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), (what, int(np.isnan(got).sum()), int(nan.sum()))
    assert (got.view(np.uint32)[~nan] == want.view(np.uint32)[~nan]).all(), what
    return int(nan.sum())


@pytest.mark.parametrize("name", DOWNSTREAM)
def test_stl_and_vertex_normals_of_zero_area_triangles(gpu, name):
    R = ref(name)
    sdf = gpu.SDF3HIP(R.shape)
    oc = gpu.OctreeHIP(sdf, R.res)
    tris = oc.RenderAll()
    blob, want = oc.WriteBinarySTL(), oracle.write_stl(tris)
    assert len(blob) == len(want) == 84 + 50 * len(tris) and blob[:84] == want[:84]
    g = np.frombuffer(blob, np.uint8, offset=84).reshape(-1, 50)
    w = np.frombuffer(want, np.uint8, offset=84).reshape(-1, 50)
    assert (g[:, 12:] == w[:, 12:]).all()                          # the 36 vertex bytes and the attribute word
    nan = nan_rule(g[:, :12].copy().view(np.float32), w[:, :12].copy().view(np.float32), "stl normals")
    zero = int(L.zero_area(tris).sum())
    print(name, "zero-area triangles", zero, "NaN normal components", nan)
    assert nan == 3 * zero > 0
    # vertex normals of the welded mesh: the existing comparison (tests/test_gpu_weld.py) unchanged, then the oracle's
    ix = gpu.OctreeHIP(sdf, R.res, payload=gpu.PAYLOAD_RECORDS).weld()
    v, _, _ = ix.read()
    step = np.float32(float(R.res) * 1e-3)
    n = ix.normals(sdf, step)
    assert (n.view(np.uint32) == sdf.normals(v, step).view(np.uint32)).all()
    nn = nan_rule(n, R.cpu.normals_central_diff(v, step), "vertex normals")
    print(name, "NaN vertex-normal components", nn, "of", n.size)


@pytest.mark.parametrize("name", DOWNSTREAM)
def test_dual_contouring_and_minecraft(gpu, name):
    """As tests/test_gpu_mesh.py compares them (test_dualcontour_identical_to_oracle, test_minecraft_render_identical_to_oracle):
    triangle sets bit-identical to the oracle's, no tolerance."""
    R = ref(name)
    sdf = gpu.SDF3HIP(R.shape)
    for chiseled in (False, True):
        dc = gpu.DualContourHIP(sdf, R.res, chiseled=chiseled)
        want = R.cpu.render_dualcontour(R.res, chiseled)
        assert dc.stats.levels == want.levels and dc.n_tris() == want.n_tris > 0, (chiseled, dc.n_tris(), want.n_tris)
        same(dc, L.sorted_bits(want.tris), f"dual contouring chiseled={chiseled}")
        assert dc.stats.evals <= want.evals
    want = R.cpu.render_minecraft(R.res)
    m = gpu.MinecraftHIP(sdf, R.res)
    assert m.n_tris() == want.n_tris > 0 and int(m.stats.evals) == want.evals and int(m.stats.levels) == want.levels
    same(m, L.sorted_bits(want.tris), "minecraft")
