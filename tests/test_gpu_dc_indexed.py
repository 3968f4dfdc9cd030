"""gsdf_hip_mesh_dualcontour_indexed on the device against the numpy twin of its contract (tests/dcref.py) over the oracle: vertices,
faces and keys equal as BYTES, verts[idx] the oracle's triangle list in the oracle's order, the same bytes on every run, through the
per-tree kernels and through the capacity-retry loop; and the indexed-mesh chain (report, simplify, project, extract, normals, PLY)
on the result. The twin sees the tree and the resolution, and no device result."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dcref as D
import projectref as P
from gsdf_amd import ply
from oracle.oracle import OracleSDF
from scaffold.builder import Builder
from test_gpu_simplify import check as check_simplify
from test_gpu_topo import check_against_twin as check_report

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [c[0] for c in D.cases(Builder())]
STAT_FIELDS = ("n_tris", "evals", "leaf_cubes", "active_leaves", "levels")
_twin = {}


def case(name):
    _, shape, res = next(c for c in D.cases(Builder()) if c[0] == name)
    return shape, F(res)


def twin(name, chiseled=False):
    """The twin's (verts, idx, keys, soup, quads, oracle result) of a case: computed once, shared, never written to."""
    if (name, chiseled) not in _twin:
        shape, res = case(name)
        _twin[(name, chiseled)] = D.mesh(OracleSDF(shape.tree()), res, chiseled)
    return _twin[(name, chiseled)]


def same_as_twin(ix, name, chiseled=False):
    v, i, k = ix.read()
    tv, ti, tk, soup, q, ref = twin(name, chiseled)
    assert (ix.n_verts, ix.n_tris) == (len(tv), len(ti)) and ix.n_tris == ref.n_tris, (name, ix.n_verts, ix.n_tris, len(tv), len(ti))
    assert k.tobytes() == tk.tobytes(), (name, "keys", np.flatnonzero(k != tk)[:8].tolist())
    assert i.tobytes() == ti.tobytes(), (name, "faces", np.flatnonzero((i != ti).any(axis=1))[:8].tolist())
    assert v.tobytes() == tv.tobytes(), (name, "vertices", np.flatnonzero((v.view(np.uint32) != tv.view(np.uint32)).any(axis=1))[:8].tolist())
    return v, i, k


@pytest.mark.parametrize("chiseled", [False, True])
@pytest.mark.parametrize("name", NAMES)
def test_identical_to_twin_and_oracle(gpu, name, chiseled):
    shape, res = case(name)
    sdf = gpu.SDF3HIP(shape)
    ix = gpu.IndexedHIP.dual_contour(sdf, res, chiseled=chiseled)
    v, i, k = same_as_twin(ix, name, chiseled)
    # the soup: the oracle's triangles in the oracle's order, not sorted
    ref = twin(name, chiseled)[5]
    assert np.ascontiguousarray(v[i.reshape(-1)]).tobytes() == np.ascontiguousarray(ref.tris, F).tobytes(), name
    # the statistics of gsdf_hip_mesh_dualcontour for the same call; no hash table in the handle's
    dc = gpu.DualContourHIP(sdf, res, chiseled=chiseled)
    assert [int(getattr(ix.mesh_stats, f)) for f in STAT_FIELDS] == [int(getattr(dc.stats, f)) for f in STAT_FIELDS]
    assert ix.mesh_stats.levels == ref.levels and F(ix.mesh_stats.res) == res and list(ix.mesh_stats.origin[:]) == list(dc.stats.origin[:])
    st = ix.stats
    assert (st.has_normals, st.ms_insert, st.probes, st.table_cells, st.attempts) == (0, 0.0, 0, 0, 0) and st.ms_keys > 0 and st.ms_number > 0
    print(name, chiseled, "V", ix.n_verts, "F", ix.n_tris, "ms_keys", st.ms_keys, "ms_number", st.ms_number, "ms_total", ix.mesh_stats.ms_total)


def test_run_to_run_determinism(gpu):
    """Two calls on one handle and one on a second handle of the same tree: byte-identical PLY files."""
    shape, res = case("npt-flange")
    one, two = gpu.SDF3HIP(shape), gpu.SDF3HIP(shape)
    files = [bytes(gpu.IndexedHIP.dual_contour(s, res).ply_view()) for s in (one, one, two)]
    assert files[0] == files[1] == files[2]
    tv, ti = twin("npt-flange")[:2]
    assert files[0] == ply.ply_bytes(tv, ti)


def test_per_tree_kernels_give_the_same_bytes(gpu):
    shape, res = case("bolt")
    sdf = gpu.SDF3HIP(shape).specialize()
    ix = gpu.IndexedHIP.dual_contour(sdf, res)
    same_as_twin(ix, "bolt")
    assert "specialised" in sdf.info()["kernels"]["eval"], sdf.info()["kernels"]


def test_capacity_retry_gives_the_same_bytes(gpu):
    """As tests/test_gpu_mesh.py: test_dualcontour_lists_regrow drives the retry loop: a fine mesh after a coarse one on the same handle
    overflows the lists sized from the coarse one and repeats -- the same bytes as on a fresh handle, whose first guess is ample."""
    s = Builder().Scene("npt-flange")
    res = F(float(s.Diagonal()) / 800)
    used = gpu.SDF3HIP(s)
    assert gpu.IndexedHIP.dual_contour(used, F(float(s.Diagonal()) / 60)).n_tris > 0
    again = gpu.IndexedHIP.dual_contour(used, res)
    fresh = gpu.IndexedHIP.dual_contour(gpu.SDF3HIP(s), res)
    assert again.mesh_stats.leaf_cubes == fresh.mesh_stats.leaf_cubes > (1 << 20)   # (more kept cubes than the floor: the first attempt overflowed)
    assert [a.tobytes() for a in again.read()] == [a.tobytes() for a in fresh.read()]
    assert again.mesh_stats.evals == fresh.mesh_stats.evals and again.n_tris == fresh.n_tris == fresh.mesh_stats.n_tris
    dc = gpu.DualContourHIP(gpu.SDF3HIP(s), res)
    assert [int(getattr(fresh.mesh_stats, f)) for f in STAT_FIELDS] == [int(getattr(dc.stats, f)) for f in STAT_FIELDS]


@pytest.mark.parametrize("name", ["sphere", "long-box"])
def test_the_chain_on_the_result(gpu, name):
    shape, res = case(name)
    sdf, cpu = gpu.SDF3HIP(shape), OracleSDF(shape.tree())
    ix = gpu.IndexedHIP.dual_contour(sdf, res)
    tv, ti, tk, _, q, _ = twin(name)
    rep, _ = check_report(ix, tv, ti)                        # bytes 0 .. 159 of the report, the shell table, the shell numbers
    assert (rep.closed_oriented, rep.euler, rep.boundary_edges) == ((0, -1, 72) if name == "sphere" else (1, 2, 0))   # tests/test_dc_ref.py
    origin = tuple(F(o) - F(0.5) * res for o in q["origin"])
    dev, st, _ = check_simplify(gpu, ix, tv, ti, F(3) * res, origin)
    assert dev is not None and st.n_tris < ix.n_tris
    tol = F(res / F(1024))
    dv = ix.deviation(sdf, tol)
    ts = P.project(cpu.Evaluate, tv, step=1.0, tol=tol, max_move=0.0, max_iters=0)[4]
    assert dv.result_bytes() == P.stats_bytes(ts) and dv.max_abs_before == float(ts["max_abs_before"]) <= 1.5 * float(res)
    back = ix.extract(None, drop_degenerate=True)
    assert [a.tobytes() for a in back.read()] == [tv.tobytes(), ti.tobytes(), tk.tobytes()]
    step = F(float(res) * 1e-3)
    n = ix.normals(sdf, step)
    assert n.tobytes() == sdf.normals(tv, step).tobytes() and ix.stats.has_normals == 1
    assert bytes(ix.ply_view()) == ply.ply_bytes(tv, ti, n)


def test_stats_and_errors(gpu):
    b = Builder()
    sdf = gpu.SDF3HIP(b.NewSphere(1.0))
    L = gpu.lib()
    h, st = C.c_void_p(), gpu.MeshStats()
    assert L.gsdf_hip_mesh_dualcontour_indexed(sdf._h, F(1.0 / 8), 0, None, C.byref(h), None) == 0 and h.value      # st is optional
    L.gsdf_hip_indexed_destroy(h)
    for res, code in ((0.0, -8), (-1.0, -8), (float("nan"), -8), (float("inf"), -8), (0.0001, -8)):    # GSDF_ERR_RESOLUTION; the last: more than 12 levels
        with pytest.raises(gpu.HipError) as e:
            gpu.IndexedHIP.dual_contour(sdf, F(res))
        assert e.value.code == code, (res, e.value.code, e.value.msg)
    with pytest.raises(gpu.HipError) as e:
        gpu.IndexedHIP.dual_contour(gpu.SDF2HIP(b.NewCircle(1.0)), F(0.1))
    assert e.value.code == -7                                                                       # GSDF_ERR_DIMENSION
    with pytest.raises(gpu.HipError) as e:
        gpu.IndexedHIP.dual_contour(gpu.SDF3HIP(b.Offset(b.NewSphere(1.0), 10.0)), F(0.5))          # no surface inside the bounds: no quad
    assert e.value.code == -1                                                                       # GSDF_ERR_EMPTY_BUFFERS
    assert L.gsdf_hip_mesh_dualcontour_indexed(None, F(0.1), 0, None, C.byref(h), None) == -3 and not h.value
    # an octree mesh of the program in flight: the workspace is shared
    flange = b.Scene("npt-flange")
    prog = gpu.SDF3HIP(flange)
    res = F(float(flange.Diagonal()) / 100)
    pending = gpu.OctreeHIP.start(prog, res)
    with pytest.raises(gpu.HipError) as e:
        gpu.IndexedHIP.dual_contour(prog, res)
    assert e.value.code == -3 and "in flight" in e.value.msg
    assert pending.wait().n_tris() > 0
    assert gpu.IndexedHIP.dual_contour(prog, res).n_tris > 0


def test_the_example(gpu, tmp_path):
    out = tmp_path / "bolt.ply"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "examples", "render_ply.py"), "bolt", "--resdiv", "60", "--renderer", "dualcontour", "--report",
                        "--interpreter", "-o", str(out)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"V (\d+) F (\d+); PLY (\d+) bytes", r.stdout)
    assert m and "bolt report:" in r.stdout, r.stdout
    v, idx, nrm = ply.read_ply(out)
    shape = Builder().Scene("bolt")
    ix = gpu.IndexedHIP.dual_contour(gpu.SDF3HIP(shape), F(float(shape.Diagonal()) / 60))
    gv, gi, _ = ix.read()
    assert nrm is None and (len(v), len(idx)) == (int(m.group(1)), int(m.group(2))) == (ix.n_verts, ix.n_tris)
    assert np.ascontiguousarray(v, F).tobytes() == gv.tobytes() and np.ascontiguousarray(idx, np.uint32).tobytes() == gi.tobytes()
    assert os.path.getsize(out) == int(m.group(3))
