"""gsdf_hip_indexed_simplify on the device against the numpy twin of its contract (tests/simplifyref.py): vertices equal BIT FOR BIT,
faces, keys and the stats' leading block equal as bytes. The twin sees the mesh (verts, idx) and the options, and no device result."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import simplifyref as S
import toporef as T
import weldref as W
from corpus import shapes3d
from gsdf_amd import ply
from scaffold.builder import Builder
from test_gpu_topo import check_against_twin as check_report
from test_gpu_weld import SMALL, records_mesh
from test_weld_ref import POSITION_BOUND_DIV, scene_shape

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check(gpu, ix, v, i, cell, origin=(0, 0, 0)):
    """Device simplify of handle `ix` against the twin's on (v, i): the result (or the same error), the stats, and the dry run.
    Returns (device mesh or None, device stats or None, twin result or None)."""
    try:
        tw = S.simplify(v, i, cell, origin)
    except S.SimplifyError as e:
        with pytest.raises(gpu.HipError) as got:
            ix.simplify(cell, origin)
        assert got.value.code == e.code, (got.value.msg, e.msg)
        if e.code == S.EMPTY_BUFFERS:
            _, st = ix.simplify(cell, origin, dry=True)
            assert st.result_bytes() == S.stats_bytes(S.simplify(v, i, cell, origin, dry=True)[3]) and st.n_tris == 0
        return None, None, None
    dev, st = ix.simplify(cell, origin)
    v2, i2, k2 = dev.read()
    tv, ti, tk, ts = tw
    got = {f: int(getattr(st, f)) for f in S.STAT_FIELDS + ["exponent"]}
    assert got == ts, (got, ts)
    assert st.result_bytes() == S.stats_bytes(ts)
    assert v2.shape == tv.shape and (u32(v2) == u32(tv)).all(), np.flatnonzero((u32(v2) != u32(tv)).any(axis=1))[:8]
    assert i2.tobytes() == ti.tobytes() and k2.tobytes() == tk.tobytes()
    assert (dev.n_verts, dev.n_tris, dev.stats.has_normals) == (ts["n_verts"], ts["n_tris"], 0)
    assert st.table_cells >= 2 * st.cells and st.attempts >= 1 and st.probes >= st.used_verts_in
    none, dry = ix.simplify(cell, origin, dry=True)
    assert none is None and dry.result_bytes() == st.result_bytes()
    return dev, st, tw


@pytest.mark.parametrize("name", sorted(T.hand_meshes()))
def test_hand_meshes(gpu, name):
    v, i = T.hand_meshes()[name]
    ix = gpu.IndexedHIP.from_arrays(v, i)
    for cell in (3.0, 5.0):
        for origin in ((0, 0, 0), (-0.5, 0.25, 1)):
            check(gpu, ix, v, i, cell, origin)


def welded(gpu, shape, resdiv):
    res = np.float32(float(shape.Diagonal()) / resdiv)
    oc = records_mesh(gpu, gpu.SDF3HIP(shape), res, marched=False)
    return oc, oc.weld(), res, tuple(np.array(oc.stats.origin[:], np.float32))


_small = {}


def small(gpu, name):
    """(handle, verts, idx, keys, res, lattice origin) of a SMALL shape at resdiv 48, made once."""
    if name not in _small:
        _, shapes = shapes3d()
        _, ix, res, origin = welded(gpu, dict(shapes)[name], 48)
        _small[name] = (ix,) + ix.read() + (res, origin)
    return _small[name]


@pytest.mark.parametrize("name", SMALL)
def test_small_shapes(gpu, name):
    ix, v, i, _, res, origin = small(gpu, name)
    kept = 0
    for cell, org in ((np.float32(2) * res, origin), (np.float32(4) * res, origin), (np.float32(3.7) * res, (0, 0, 0))):
        dev, st, tw = check(gpu, ix, v, i, cell, org)
        kept += dev is not None
        if dev is not None and name == "torus" and org == origin:
            check_report(dev, tw[0], tw[1])        # the result is an ordinary handle: its report is the twin's report of the twin's result
            print(name, float(cell / res), "res: F", st.n_tris_in, "->", st.n_tris, "clusters", st.cells, "largest", st.largest_cell)
    assert kept == 3


def coarse_soup():
    """20 000 vertices in [-3, 5]^3, numbered so that the vertices of one cell of 4 are consecutive (a wave of 64 vertices is then of
    one cell almost always: the one-atomic-per-wave path), some of them exact duplicates of others; 60 000 random faces, some with
    repeated indices, some repeated whole."""
    rng = np.random.default_rng(21)
    v = rng.uniform(-3, 5, (20000, 3)).astype(np.float32)
    dup = rng.choice(20000, 500, replace=False)
    v[dup] = v[(dup + 7) % 20000]
    c = np.floor(v.astype(np.float64) / 4.0).astype(np.int64)
    v = v[np.lexsort((c[:, 0], c[:, 1], c[:, 2]))]
    i = rng.integers(0, 20000, (60000, 3)).astype(np.uint32)
    i[::41, 2] = i[::41, 0]
    i[5::53] = i[4::53][:len(i[5::53])]
    return v, i


def test_random_soup(gpu):
    v, i = coarse_soup()
    ix = gpu.IndexedHIP.from_arrays(v, i)
    for cell in (0.5, 4.0):
        used, key, _, n_deg = S.cluster(v, i, cell)
        pad = np.zeros(-len(key) % 64, np.uint64)
        one = sum(len(set(w[w != 0])) <= 1 for w in np.concatenate([key, pad]).reshape(-1, 64))
        dev, st, _ = check(gpu, ix, v, i, cell)
        print("soup cell", cell, "waves of one cell:", one, "of", (len(key) + 63) // 64, "clusters", st.cells, "largest", st.largest_cell, "kept", st.n_tris)
        assert dev is not None and n_deg > 0 and st.collapsed > 0
        if cell == 4.0:
            assert st.cells == 27 and one >= 280 and st.largest_cell > 1000          # 313 waves, 26 of them across a boundary
        else:
            assert one < 5 and st.cells > 3000


def keyed(v, i, k):
    """What of a simplified mesh does not depend on numbering: the sorted (key, position bits) rows, the sorted faces as key triples."""
    rows = np.concatenate([k.astype(np.uint64)[:, None], u32(v).astype(np.uint64)], axis=1)
    faces = k[i.astype(np.int64)]
    return rows[np.lexsort(rows.T[::-1])].tobytes(), faces[np.lexsort(faces.T[::-1])].tobytes()


def test_order_independence(gpu):
    ix, v, i, k, res, origin = small(gpu, "smoothunion")
    cell = np.float32(3) * res
    a, sa = ix.simplify(cell, origin)
    want = keyed(*a.read())
    perm = np.random.default_rng(31).permutation(len(i))
    b, sb = gpu.IndexedHIP.from_arrays(v, i[perm], k).simplify(cell, origin)
    assert sb.result_bytes() == sa.result_bytes() and keyed(*b.read()) == want
    vp = np.random.default_rng(32).permutation(len(v))      # new number of old vertex j: vp[j]
    v2 = np.empty_like(v)
    v2[vp] = v
    c, sc = gpu.IndexedHIP.from_arrays(v2, vp[i.astype(np.int64)].astype(np.uint32)).simplify(cell, origin)
    assert sc.result_bytes() == sa.result_bytes() and keyed(*c.read()) == want
    assert sa.n_tris > 0 and sa.collapsed > 0 and sa.largest_cell > 1


def test_identical_bytes_across_runs_and_table_sizes(gpu, monkeypatch):
    ix, v, i, _, res, origin = small(gpu, "torus")
    cell = np.float32(1.5) * res
    assert S.simplify(v, i, cell, origin, dry=True)[3]["cells"] >= 1024      # so that a table of 1024 cells has to grow
    first, st = ix.simplify(cell, origin)
    want = [a.tobytes() for a in first.read()]
    assert st.attempts == 1
    for _ in range(2):
        again, s2 = ix.simplify(cell, origin)
        assert [a.tobytes() for a in again.read()] == want and s2.result_bytes() == st.result_bytes() and again.ply() == first.ply()
    monkeypatch.setenv("GSDF_HIP_SIMPLIFY_CELLS_MIN", "1024")
    grown, s3 = ix.simplify(cell, origin)
    assert s3.attempts > 1 and s3.table_cells >= 2 * s3.cells
    assert [a.tobytes() for a in grown.read()] == want and s3.result_bytes() == st.result_bytes()
    _, s4 = ix.simplify(cell, origin, dry=True)
    assert s4.attempts > 1 and s4.result_bytes() == st.result_bytes()


def test_tiny_cell_is_extract(gpu):
    ix, v, i, _, res, _ = small(gpu, "sphere")
    cell = res * np.float32(2.0 ** -12)
    ts = S.simplify(v, i, cell, dry=True)[3]
    assert ts["cells"] == ts["used_verts_in"]                                 # every cluster is one vertex
    dev, st, _ = check(gpu, ix, v, i, cell)
    ex = ix.extract(None, drop_degenerate=True)
    ve, ie, _ = ex.read()
    v2, i2, _ = dev.read()
    assert (u32(v2) == u32(ve)).all() and (i2 == ie).all() and st.largest_cell == 1 and st.collapsed == 0


def test_dry_run_and_simplify_to(gpu):
    ix, v, i, _, res, origin = small(gpu, "sphere")
    cell = np.float32(3) * res
    none, dry = ix.simplify(cell, origin, dry=True)
    dev, st = ix.simplify(cell, origin)
    assert none is None and dry.result_bytes() == st.result_bytes() and dev.n_tris == dry.n_tris and dev.n_verts == dry.n_verts
    o = gpu.SimplifyOpts(cell=cell, origin=(C.c_float * 3)(*origin))
    assert gpu.lib().gsdf_hip_indexed_simplify(ix._h, C.byref(o), None, None) == -3      # neither a handle nor stats asked for
    max_tris = ix.n_tris // 10
    cell0 = np.float32(2) * res
    out, so, used = ix.simplify_to(max_tris, cell0, origin)
    want = cell0
    while S.simplify(v, i, want, origin, dry=True)[3]["n_tris"] > max_tris:
        want = np.float32(want * np.float32(2))
    assert 0 < out.n_tris == so.n_tris <= max_tris and np.float32(used) == want and want > cell0
    tv, ti, tk, ts = S.simplify(v, i, want, origin)
    v2, i2, k2 = out.read()
    assert (u32(v2) == u32(tv)).all() and (i2 == ti).all() and (k2 == tk).all() and so.result_bytes() == S.stats_bytes(ts)
    with pytest.raises(ValueError):
        ix.simplify_to(0, cell0, origin)                                      # nothing kept before the count falls to 0


def test_errors(gpu):
    v, i = T.hand_meshes()["tet"]
    vn = np.vstack([v, [[np.nan, 0, 0]]]).astype(np.float32)
    ok = gpu.IndexedHIP.from_arrays(vn, i)                                    # NaN in a vertex no face names: fine
    assert check(gpu, ok, vn, i, 3.0)[0] is not None
    also = np.vstack([i, [[4, 4, 0]]]).astype(np.uint32)                     # ... or only a degenerate face names
    assert check(gpu, gpu.IndexedHIP.from_arrays(vn, also), vn, also, 3.0)[0] is not None
    bad = np.vstack([i, [[4, 1, 0]]]).astype(np.uint32)
    with pytest.raises(gpu.HipError) as e:
        gpu.IndexedHIP.from_arrays(vn, bad).simplify(3.0)
    assert e.value.code == -3 and e.value.msg.startswith("simplify: 1 used")
    ix = gpu.IndexedHIP.from_arrays(v, i)
    with pytest.raises(gpu.HipError) as e:
        ix.simplify(6.0 / (1 << 19))
    assert e.value.code == -8 and "vertex 1 " in e.value.msg                  # GSDF_ERR_RESOLUTION
    check(gpu, ix, v, i, 6.0 / (1 << 19))
    with pytest.raises(gpu.HipError) as e:
        ix.simplify(100.0)
    assert e.value.code == -1                                                 # GSDF_ERR_EMPTY_BUFFERS
    none, st = ix.simplify(100.0, dry=True)
    assert none is None and (st.n_tris, st.n_verts, st.cells, st.collapsed, st.largest_cell) == (0, 0, 1, 4, 4)
    check(gpu, ix, v, i, 100.0)
    for cell in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(gpu.HipError) as e:
            ix.simplify(cell)
        assert e.value.code == -3


def test_example_simplify(gpu, tmp_path):
    """examples/render_ply.py --simplify 3 --report as a child process. The mesher's record order differs from run to run and with it
    the last bits of the welded positions (the weld keeps the copy of the smallest slot), so no two processes hold the same bytes:
    the twin's prediction is of the COUNTS, which the example's grid (half a res below the lattice origin: no lattice plane is a
    cell face) makes the same for every run; and the plain run is compared with this process's mesh by its one line of output, the PLY header's bytes, size, topology and
    positions within the weld's bound."""
    name, resdiv = "bolt", 60
    shape = Builder().Scene(name)
    oc, ix, res, lattice = welded(gpu, shape, resdiv)
    origin = tuple(np.float32(o) - np.float32(0.5) * res for o in lattice)
    v, i, _ = ix.read()
    ts = S.simplify(v, i, np.float32(3) * res, origin, dry=True)[3]
    _, other, _, _ = welded(gpu, shape, resdiv)                              # a second mesh of this process: the same counts
    vo, io, _ = other.read()
    assert S.simplify(vo, io, np.float32(3) * res, origin, dry=True)[3] == ts
    cmd = [sys.executable, os.path.join(ROOT, "examples", "render_ply.py"), name, "--resdiv", str(resdiv), "--interpreter"]
    out = tmp_path / "s.ply"
    r = subprocess.run(cmd + ["--simplify", "3", "--report", "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    v2, i2, n2 = ply.read_ply(out)
    assert 0 < ts["n_tris"] < len(i) and (len(v2), len(i2)) == (ts["n_verts"], ts["n_tris"]) and n2 is None
    assert r.stdout.count(" report: ") == 2 and f"{name} simplified report: " in r.stdout and f"F {len(i)} -> {len(i2)} " in r.stdout
    assert f"({ts['cells']} clusters, the largest of {ts['largest_cell']} vertices; {ts['collapsed']} faces collapsed" in r.stdout
    plain = tmp_path / "p.ply"
    r = subprocess.run(cmd + ["-o", str(plain)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "simplified in cells" not in r.stdout and len(r.stdout.strip().splitlines()) == 1
    data, mine = plain.read_bytes(), ix.ply()
    head = len(ply.header(len(v), len(i), False))
    assert data[:head] == mine[:head] == ply.header(len(v), len(i), False)   # the file's header, byte for byte
    vp, ip, _ = ply.read_ply(plain)
    assert plain.stat().st_size == len(ix.ply()) and vp.shape == v.shape and ip.shape == i.shape
    assert W.edge_report(ip) == W.edge_report(i)
    assert np.abs(np.sort(vp, axis=0).astype(np.float64) - np.sort(v, axis=0)).max() <= float(res) / POSITION_BOUND_DIV


def test_flange_400(gpu):
    shape = Builder().Scene("npt-flange")
    oc, ix, res, origin = welded(gpu, shape, 400)
    assert ix.n_tris == 423852
    v, i, _ = ix.read()
    cell = np.float32(4) * res
    dev, st = ix.simplify(cell, origin)
    tv, ti, tk, ts = S.simplify(v, i, cell, origin)
    assert st.result_bytes() == S.stats_bytes(ts)
    v2, i2, k2 = dev.read()
    digest = lambda *a: hashlib.sha256(b"".join(np.ascontiguousarray(x).tobytes() for x in a)).hexdigest()
    assert digest(v2, i2, k2) == digest(tv, ti, tk)
    print("flange 400, cell 4 res: F", st.n_tris_in, "->", st.n_tris, "V", st.n_verts_in, "->", st.n_verts, "clusters", st.cells, "largest", st.largest_cell,
          "ms cells/faces", st.ms_cells, st.ms_faces, "weld ms", ix.ms_device, "probes", st.probes, "cells", st.table_cells, "attempts", st.attempts)
