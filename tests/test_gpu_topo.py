"""gsdf_hip_indexed_report / _shells / _read_shell_of / _extract on the device against the numpy twin of their contract
(tests/toporef.py): integers equal, float64 and float32 fields equal BIT FOR BIT. The twin sees the mesh (verts, idx) and no device
result of the analysis."""
import ctypes as C

import numpy as np
import pytest

import toporef as T
from corpus import shapes3d
from gsdf_amd import ply
from scaffold.builder import Builder
from test_gpu_weld import SMALL, records_mesh
from test_weld_ref import MANIFOLD_SCENES, scene_shape

pytestmark = pytest.mark.gpu

INT_FIELDS = ["n_verts", "n_tris", "degenerate", "nonfinite", "used_verts", "edges", "boundary_edges", "nonmanifold_edges", "misoriented_edges",
              "n_shells", "euler", "closed_oriented", "exponent"]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def check_against_twin(ix, verts, idx):
    """Device report, shell table and shell numbers of handle `ix` against the twin's on (verts, idx); returns (report, twin)."""
    tw = T.analyse(verts, idx)
    rep, want = ix.report(), tw["report"]
    for f in INT_FIELDS:
        assert int(getattr(rep, f)) == int(want[f]), (f, int(getattr(rep, f)), int(want[f]))
    for f in ("area", "volume"):
        assert bits(np.float64(getattr(rep, f))) == bits(np.float64(want[f])), (f, getattr(rep, f), want[f])
    assert (bits(np.array(rep.centroid[:], np.float64)) == bits(want["centroid"])).all(), (rep.centroid[:], want["centroid"])
    assert (bits(np.array(rep.bbox[:], np.float32)) == bits(want["bbox"])).all(), (rep.bbox[:], want["bbox"])
    sh = ix.shells()
    assert sh.dtype == T.SHELL_DTYPE and sh.shape == tw["shells"].shape
    for f in T.SHELL_DTYPE.names:
        a, b = sh[f], tw["shells"][f]
        same = (bits(a) == bits(b)) if a.dtype.kind == "f" else (a == b)
        assert same.all(), (f, a[~same.reshape(len(a), -1).all(axis=1)][:4], b[~same.reshape(len(a), -1).all(axis=1)][:4])
    assert sh.tobytes() == tw["shells"].tobytes()
    sv, sf = ix.shell_of()
    assert (sv == tw["shell_of_vertex"]).all() and (sf == tw["shell_of_face"]).all()
    return rep, tw


@pytest.mark.parametrize("name", sorted(T.hand_meshes()))
def test_hand_meshes(gpu, name):
    v, i = T.hand_meshes()[name]
    ix = gpu.IndexedHIP.from_arrays(v, i)
    v2, i2, k2 = ix.read()
    assert (bits(v2) == bits(v)).all() and (i2 == i).all() and (k2 == 0).all()   # every accessor works; absent keys read as 0
    assert ix.ply() == ply.ply_bytes(v, i)
    check_against_twin(ix, v, i)


def welded(gpu, shape, resdiv):
    res = np.float32(float(shape.Diagonal()) / resdiv)
    oc = records_mesh(gpu, gpu.SDF3HIP(shape), res, marched=False)
    return oc, oc.weld()


@pytest.mark.parametrize("name", SMALL)
def test_small_shapes(gpu, name):
    _, shapes = shapes3d()
    _, ix = welded(gpu, dict(shapes)[name], 48)
    v, i, _ = ix.read()
    check_against_twin(ix, v, i)


@pytest.mark.parametrize("name,resdiv,expect", MANIFOLD_SCENES)
def test_manifold_scenes(gpu, name, resdiv, expect):
    _, ix = welded(gpu, scene_shape(Builder(), name), resdiv)
    v, i, _ = ix.read()
    rep, _ = check_against_twin(ix, v, i)
    assert rep.closed_oriented == 1 and (rep.used_verts, rep.n_tris, rep.euler) == expect
    print(name, resdiv, "shells", rep.n_shells, "volume", rep.volume, "area", rep.area, "ms edges/shells/measure", rep.ms_edges, rep.ms_shells, rep.ms_measure)


def test_random_soup(gpu):
    v, i = T.random_soup()
    ix = gpu.IndexedHIP.from_arrays(v, i)
    rep, tw = check_against_twin(ix, v, i)
    # the soup is what it is meant to be: every class of face and edge, hundreds of shells, waves of 64 faces that mix shells
    assert rep.degenerate > 0 and rep.nonfinite > 0 and rep.boundary_edges > 0 and rep.nonmanifold_edges > 0 and rep.misoriented_edges > 0
    assert rep.n_shells > 200 and rep.used_verts < rep.n_verts
    sf = tw["shell_of_face"].reshape(-1)
    pad = np.full(-len(sf) % 64, T.NONE, np.uint32)
    waves = np.concatenate([sf, pad]).reshape(-1, 64)
    assert sum(len(set(w[w != T.NONE])) > 1 for w in waves) > 100


def test_identical_bytes_across_runs_and_table_sizes(gpu, monkeypatch):
    shape = scene_shape(Builder(), "two-spheres")
    oc, ix = welded(gpu, shape, 60)
    first = ix.report()
    again = ix.report()
    assert bytes(first) == bytes(again)                       # cached on the handle: the very same struct, its times included
    other = oc.weld()
    r2 = other.report()
    assert r2.result_bytes() == first.result_bytes() and other.shells().tobytes() == ix.shells().tobytes()
    assert all((a == b).all() for a, b in zip(other.shell_of(), ix.shell_of()))
    assert first.attempts == 1 and first.table_cells >= 2 * first.edges and first.probes >= first.edges
    monkeypatch.setenv("GSDF_HIP_TOPO_CELLS_MIN", str(int(first.edges) // 4))
    grown = oc.weld()
    r3 = grown.report()
    assert r3.attempts >= 2 and r3.table_cells >= 2 * r3.edges
    assert r3.result_bytes() == first.result_bytes() and grown.shells().tobytes() == ix.shells().tobytes()
    assert all((a == b).all() for a, b in zip(grown.shell_of(), ix.shell_of()))


def test_permuted_faces_report_the_same_totals(gpu):
    v, i = T.random_soup(seed=11)
    perm = np.random.default_rng(5).permutation(len(i))
    a = gpu.IndexedHIP.from_arrays(v, i)
    b = gpu.IndexedHIP.from_arrays(v, i[perm])
    assert a.report().result_bytes() == b.report().result_bytes()
    assert a.shells().tobytes() == b.shells().tobytes()       # labels are vertex numbers: unchanged by a permutation of the faces
    _, ix = welded(gpu, scene_shape(Builder(), "torus"), 60)
    v, i, k = ix.read()
    perm = np.random.default_rng(6).permutation(len(i))
    c = gpu.IndexedHIP.from_arrays(v, i[perm], k)
    assert c.report().result_bytes() == ix.report().result_bytes() and c.shells().tobytes() == ix.shells().tobytes()


def test_extract_all_reproduces_the_ply(gpu):
    shape = scene_shape(Builder(), "torus")
    res = np.float32(float(shape.Diagonal()) / 60)
    sdf = gpu.SDF3HIP(shape)
    ix = records_mesh(gpu, sdf, res, marched=False).weld()
    assert ix.report().degenerate == 0
    assert ix.extract().ply() == ix.ply()
    ix.normals(sdf, np.float32(float(res) * 1e-3))
    ex = ix.extract(keep=None, drop_degenerate=True)
    assert ex.stats.has_normals == 1 and ex.ply() == ix.ply()   # normals carried bit for bit


def test_extract_each_of_two_spheres(gpu):
    _, ix = welded(gpu, scene_shape(Builder(), "two-spheres"), 60)
    rep, sh = ix.report(), ix.shells()
    assert rep.n_shells == 2
    v, i, k = ix.read()
    sv, sf = ix.shell_of()
    faces = 0
    for s in range(2):
        keep = np.arange(2) == s
        ex = ix.extract(keep)
        r = ex.report()
        assert r.exponent == rep.exponent   # the same quantum: the measures below can be compared bit for bit
        one = ex.shells()
        assert len(one) == 1 and one["label"][0] == 0
        for f in T.SHELL_DTYPE.names:
            if f != "label":
                assert bits(one[f]).tobytes() == bits(sh[f][s:s + 1]).tobytes(), f
        assert (r.used_verts, r.n_tris, r.edges, r.euler, r.closed_oriented) == (sh["n_verts"][s], sh["n_tris"][s], sh["edges"][s], sh["euler"][s], 1)
        assert bits(np.float64(r.volume)) == bits(sh["volume"][s]) and bits(np.float64(r.area)) == bits(sh["area"][s])
        tv, ti, tk, _ = T.extract(v, i, k, None, sf, keep)
        v2, i2, k2 = ex.read()
        assert (bits(v2) == bits(tv)).all() and (i2 == ti).all() and (k2 == tk).all()
        _, pi, _ = ply.parse_ply(ex.ply())
        faces += len(pi)
    assert faces == ix.n_tris


def test_extract_random_soup_and_errors(gpu):
    v, i = T.random_soup(seed=3)
    keys = np.random.default_rng(9).integers(0, 2 ** 63, len(v), dtype=np.uint64)
    ix = gpu.IndexedHIP.from_arrays(v, i, keys)
    tw = T.analyse(v, i)
    sf = tw["shell_of_face"]
    ex = ix.extract(drop_degenerate=True)
    tv, ti, tk, _ = T.extract(v, i, keys, None, sf, None, True)
    v2, i2, k2 = ex.read()
    assert (bits(v2) == bits(tv)).all() and (i2 == ti).all() and (k2 == tk).all()
    assert ex.report().degenerate == 0 and ex.n_tris == ix.n_tris - ix.report().degenerate
    check_against_twin(ex, tv, ti)
    # degenerate faces stay only when asked for with every shell kept
    allf = ix.extract(drop_degenerate=False)
    tv, ti, tk, _ = T.extract(v, i, keys, None, sf, None, False)
    v2, i2, k2 = allf.read()
    assert allf.n_tris == ix.n_tris and (bits(v2) == bits(tv)).all() and (i2 == ti).all() and (k2 == tk).all()
    # a selection by criterion: the shells with at least 8 faces
    keep = ix.select_shells(min_tris=8)
    assert 0 < keep.sum() < len(keep)
    some = ix.extract(keep, drop_degenerate=False)
    tv, ti, tk, _ = T.extract(v, i, keys, None, sf, keep, False)
    v2, i2, k2 = some.read()
    assert (bits(v2) == bits(tv)).all() and (i2 == ti).all() and (k2 == tk).all()
    assert (some.shells()["n_tris"] >= 8).all() and len(some.shells()) == keep.sum()
    # nothing kept
    h = C.c_void_p()
    none = np.zeros(len(keep), np.uint8)
    assert gpu.lib().gsdf_hip_indexed_extract(ix._h, none.ctypes.data, 1, C.byref(h)) == -1 and not h.value   # GSDF_ERR_EMPTY_BUFFERS
    # an index past the vertices
    bad = i.copy()
    bad[17, 1] = len(v) + 3
    with pytest.raises(gpu.HipError) as e:
        gpu.IndexedHIP.from_arrays(v, bad)
    assert e.value.code == -3 and str(len(v) + 3) in e.value.msg and "face 17" in e.value.msg
    # a short shell buffer reports the count
    n = C.c_uint64()
    buf = np.zeros(1, T.SHELL_DTYPE)
    assert gpu.lib().gsdf_hip_indexed_shells(ix._h, buf.ctypes.data, 1, C.byref(n)) == -9 and n.value == len(keep)


def test_flange_400(gpu):
    shape = Builder().Scene("npt-flange")
    res = np.float32(float(shape.Diagonal()) / 400)
    ix = records_mesh(gpu, gpu.SDF3HIP(shape), res, marched=False).weld()
    rep = ix.report()
    assert ix.n_tris == 423852 and rep.closed_oriented == 1 and rep.euler == 0 and rep.used_verts == rep.n_verts == 211926
    print("flange 400: weld ms", ix.ms_device, "report ms edges/shells/measure", rep.ms_edges, rep.ms_shells, rep.ms_measure, "shells", rep.n_shells,
          "volume", rep.volume, "area", rep.area, "probes", rep.probes, "cells", rep.table_cells)
