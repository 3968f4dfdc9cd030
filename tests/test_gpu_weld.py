"""gsdf_hip_mesh_weld on the device against the numpy twin of its contract (tests/weldref.py), and the contract's own clauses on
the device's output alone. The twin is handed the device's cut leaves in the device's order (gsdf_hip_mesh_read_records: the order
is the mesher's, not the contract's) and evaluates their corners with the oracle."""
import ctypes as C
import os

import numpy as np
import pytest

import weldref as W
from corpus import shapes3d
from gsdf_amd import hip, ply
from oracle.oracle import OracleSDF
from scaffold.builder import Builder
from test_weld_ref import MANIFOLD_SCENES, POSITION_BOUND_DIV, scene_shape

pytestmark = pytest.mark.gpu

SMALL = ["sphere", "box", "boxframe", "cylr", "torus", "union", "diff", "smoothunion", "rotate", "twist", "revolve_off", "array"]


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def records_mesh(gpu, sdf, res, marched):
    oc = gpu.OctreeHIP(sdf, res, payload=gpu.PAYLOAD_RECORDS)
    return oc.march() if marched else oc


def check_against_twin(gpu, shape, res, specialised=False):
    sdf = gpu.SDF3HIP(shape)
    if specialised:
        sdf.specialize()
    cpu = OracleSDF(shape.tree())
    oc = records_mesh(gpu, sdf, res, marched=False)
    dist, leaves, case = oc.records()
    ix_before = oc.weld()          # records not marched yet
    v0, i0, k0 = ix_before.read()
    oc.march()
    soup_dev = oc.RenderAll().reshape(-1, 3)
    ix_after = oc.weld()           # the same records, parked by the march
    v1, i1, k1 = ix_after.read()
    assert ix_before.n_tris == ix_after.n_tris == oc.n_tris() and len(i0) == oc.n_tris()
    assert (u32(v0) == u32(v1)).all() and (i0 == i1).all() and (k0 == k1).all()
    origin, r = np.array(oc.stats.origin[:], np.float32), np.float32(oc.stats.res)
    vt, it, kt, soup = W.weld(cpu, leaves, origin, r)
    assert soup.shape == soup_dev.shape and (u32(soup) == u32(soup_dev)).all()   # the twin's soup is the marched soup
    assert v0.shape == vt.shape and (u32(v0) == u32(vt)).all()
    assert (i0 == it).all() and (k0 == kt).all()
    return v0, i0, k0


@pytest.mark.parametrize("name", SMALL)
def test_weld_matches_twin_small_shapes(gpu, name):
    _, shapes = shapes3d()
    shape = dict(shapes)[name]
    res = np.float32(float(shape.Diagonal()) / 48)
    check_against_twin(gpu, shape, res)


@pytest.mark.parametrize("name,resdiv", [(n, rd) for n, rd, _ in MANIFOLD_SCENES if n not in ("sphere", "torus", "two-spheres")])
def test_weld_matches_twin_example_parts(gpu, name, resdiv):
    shape = scene_shape(Builder(), name)
    res = np.float32(float(shape.Diagonal()) / resdiv)
    a = check_against_twin(gpu, shape, res)
    b = check_against_twin(gpu, shape, res, specialised=True)   # interpreter and per-tree kernels: the same records, the same weld
    # (the two meshes' record ORDER may differ, so compare what does not depend on it: vertices by key)
    oa, ob = np.argsort(a[2]), np.argsort(b[2])
    assert (a[2][oa] == b[2][ob]).all()


@pytest.mark.parametrize("name,resdiv,expect", MANIFOLD_SCENES)
def test_manifold_and_euler(gpu, name, resdiv, expect):
    shape = scene_shape(Builder(), name)
    res = np.float32(float(shape.Diagonal()) / resdiv)
    ix = records_mesh(gpu, gpu.SDF3HIP(shape), res, marched=False).weld()
    _, idx, _ = ix.read()
    rep = W.edge_report(idx)
    print(name, resdiv, rep)
    assert rep["closed_oriented"], rep
    assert (rep["V"], rep["F"], rep["euler"]) == expect, rep
    assert rep["V"] == ix.n_verts


def test_contract_on_device_flange_400(gpu, monkeypatch):
    shape = Builder().Scene("npt-flange")
    sdf = gpu.SDF3HIP(shape)
    res = np.float32(float(shape.Diagonal()) / 400)
    oc = records_mesh(gpu, sdf, res, marched=True)
    F = oc.n_tris()
    assert F == 423852
    ix = oc.weld()
    v, idx, keys = ix.read()
    soup = oc.RenderAll().reshape(-1, 3)
    flat = idx.reshape(-1).astype(np.int64)
    assert len(idx) == F and ix.n_verts == len(v) == len(keys) and len(np.unique(keys)) == len(keys)
    # vertex numbers first appear in increasing order
    uniq, first = np.unique(flat, return_index=True)
    assert (uniq == np.arange(len(v))).all() and (np.diff(first) > 0).all()
    # owners carry the soup's bits, every other slot lies within the bound
    assert (u32(v) == u32(soup[first])).all()
    bound = float(res) / POSITION_BOUND_DIV
    worst = float(np.abs(v[flat].astype(np.float64) - soup.astype(np.float64)).max())
    print("largest |vertex - slot| / res:", worst / float(res))
    assert worst <= bound
    # two welds of the same records: identical bytes; so with a table that has to grow twice
    again = oc.weld()
    assert again.ply() == ix.ply()
    st = ix.stats
    assert st.attempts == 1 and st.table_cells >= 2 * ix.n_verts and st.probes >= 3 * F
    monkeypatch.setenv("GSDF_HIP_WELD_CELLS_MIN", str(ix.n_verts // 2))
    grown = oc.weld()
    assert grown.stats.attempts >= 2 and grown.ply() == ix.ply()
    print("weld ms", ix.ms_device, "keys/insert/number", st.ms_keys, st.ms_insert, st.ms_number, "probes", st.probes, "cells", st.table_cells)


def test_normals_and_ply_bytes(gpu):
    b = Builder()
    shape = b.NewTorus(1.0, 0.47)
    sdf = gpu.SDF3HIP(shape)
    res = np.float32(float(shape.Diagonal()) / 70)
    ix = records_mesh(gpu, sdf, res, marched=False).weld()
    v, idx, keys = ix.read()
    data = ix.ply()
    assert data == ply.ply_bytes(v, idx) and bytes(ix.ply_view()) == data and len(data) == ix.ply_size()
    v2, i2, n2 = ply.parse_ply(data)
    assert n2 is None and (u32(v2) == u32(v)).all() and (i2 == idx).all()
    step = np.float32(float(res) * 1e-3)
    n = ix.normals(sdf, step)
    want = sdf.normals(v, step)
    assert (u32(n) == u32(want)).all()
    data = ix.ply()
    assert data == ply.ply_bytes(v, idx, n) and ix.stats.has_normals == 1 and ix.stats.ms_ply > 0
    v3, i3, n3 = ply.parse_ply(data)
    assert (u32(n3) == u32(n)).all() and (i3 == idx).all()
    # a short buffer reports the size it needs
    ln = C.c_size_t()
    buf = np.empty(16, np.uint8)
    assert gpu.lib().gsdf_hip_indexed_ply(ix._h, buf.ctypes.data, buf.size, C.byref(ln)) == -9 and ln.value == len(data)


def test_refused_meshes(gpu):
    b = Builder()
    shape = b.NewSphere(1)
    sdf = gpu.SDF3HIP(shape)
    res = np.float32(float(shape.Diagonal()) / 40)
    L = gpu.lib()

    def refused(mesh, code=-3):
        h = C.c_void_p()
        assert L.gsdf_hip_mesh_weld(mesh._mesh, C.byref(h)) == code
        assert not h.value
        return L.gsdf_hip_last_error().decode()

    assert "GSDF_PAYLOAD_RECORDS" in refused(gpu.OctreeHIP(sdf, res))                                   # triangle payload
    refused(gpu.FlatHIP(sdf, res))
    refused(gpu.DualContourHIP(sdf, res))
    refused(gpu.MinecraftHIP(sdf, np.float32(float(res) * 4)))
    shard = gpu.OctreeHIP(sdf, res, payload=gpu.PAYLOAD_RECORDS, shard_rank=0, shard_count=2)
    assert "shard_count == 1" in refused(shard)
    refused(shard.march())
    os.environ["GSDF_HIP_COMM"] = "loopback"
    try:
        comm = gpu.CommHIP(gpu.CommHIP.unique_id(), 0, 1)
        whole = gpu.OctreeHIP(sdf, res, payload=gpu.PAYLOAD_RECORDS)
        refused(hip._gatherv(whole, comm))                                                             # gathered
        whole.weld()                                                                                    # its source still welds
    finally:
        os.environ.pop("GSDF_HIP_COMM", None)
    h = C.c_void_p()
    assert L.gsdf_hip_mesh_weld(None, C.byref(h)) == -3
