"""gsdf_hip_indexed_simplify_adaptive on the device against the numpy twin of its contract (tests/adaptiveref.py): vertices equal BIT
FOR BIT, faces, keys and the stats' leading block equal as bytes, the dry run equal to the real run's leading block. The twin sees
the mesh (verts, idx, keys) and the options, and no device result."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import adaptiveref as A
import toporef as T
from gsdf_amd import ply
from test_gpu_dc_indexed import case as dc_case
from test_gpu_simplify import coarse_soup, small
from test_gpu_topo import check_against_twin as check_report
from test_gpu_weld import SMALL

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def stats_dict(st):
    d = {f: int(getattr(st, f)) for f in A.STAT_FIELDS if f not in ("chosen", "max_err")}
    d["chosen"], d["max_err"] = [int(x) for x in st.chosen], float(st.max_err)
    return d


def check(gpu, ix, v, i, k, cell, tol, levels, origin=(0, 0, 0)):
    """Device result of handle `ix` against the twin's on (v, i, k): the mesh (or the same error), the stats, the dry run. Returns
    (device mesh or None, device stats or None, twin result or None)."""
    try:
        tw = A.simplify(v, i, cell, tol, levels, origin, k)
    except A.AdaptiveError as e:
        with pytest.raises(gpu.HipError) as got:
            ix.simplify_adaptive(cell, tol, levels, origin)
        assert got.value.code == e.code, (got.value.msg, e.msg)
        if e.code == A.EMPTY_BUFFERS:
            _, st = ix.simplify_adaptive(cell, tol, levels, origin, dry=True)
            assert st.result_bytes() == A.stats_bytes(A.simplify(v, i, cell, tol, levels, origin, k, dry=True)[3]) and st.n_tris == 0
        return None, None, None
    dev, st = ix.simplify_adaptive(cell, tol, levels, origin)
    v2, i2, k2 = dev.read()
    tv, ti, tk, ts = tw
    assert stats_dict(st) == ts, (stats_dict(st), ts)
    assert st.result_bytes() == A.stats_bytes(ts)
    assert v2.shape == tv.shape and (u32(v2) == u32(tv)).all(), np.flatnonzero((u32(v2) != u32(tv)).any(axis=1))[:8]
    assert i2.tobytes() == ti.tobytes() and k2.tobytes() == tk.tobytes()
    assert (dev.n_verts, dev.n_tris, dev.stats.has_normals) == (ts["n_verts"], ts["n_tris"], 0)
    assert st.table_cells >= 2 * st.cells and st.attempts >= 1 and st.probes >= st.used_verts_in * levels
    none, dry = ix.simplify_adaptive(cell, tol, levels, origin, dry=True)
    assert none is None and dry.result_bytes() == st.result_bytes()
    return dev, st, tw


@pytest.mark.parametrize("name", sorted(T.hand_meshes()))
def test_hand_meshes(gpu, name):
    v, i = T.hand_meshes()[name]
    ix = gpu.IndexedHIP.from_arrays(v, i)
    for cell in (3.0, 5.0):
        for origin in ((0, 0, 0), (-0.5, 0.25, 1)):
            for levels, tol in ((1, 0.0), (1, 0.5), (3, 0.0), (3, 0.5)):
                check(gpu, ix, v, i, None, cell, tol, levels, origin)


@pytest.mark.parametrize("name", SMALL)
def test_small_shapes(gpu, name):
    ix, v, i, k, res, lattice = small(gpu, name)
    grid = tuple(F(o) - F(0.5) * res for o in lattice)
    faces = []
    for tol in (res / F(8), res / F(2)):
        dev, st, tw = check(gpu, ix, v, i, k, res, tol, 5, grid)
        assert dev is not None and st.n_tris < st.n_tris_in
        faces.append(st.n_tris)
        if name == "torus":
            check_report(dev, tw[0], tw[1])        # the result is an ordinary handle: its report is the twin's report of the twin's result
            print(name, "tol", float(tol / res), "res: F", st.n_tris_in, "->", st.n_tris, "chosen", list(st.chosen[:5]), "singles", st.singles,
                  "largest", st.largest_cluster, "max_err/res", st.max_err / float(res))
    assert faces[1] <= faces[0]


def test_random_soup(gpu):
    """Waves of one cell at the upper levels and of many cells at level 0: both paths of every per-wave reduction."""
    v, i = coarse_soup()
    ix = gpu.IndexedHIP.from_arrays(v, i)
    for tol in (0.0, 0.05, 8.0):
        dev, st, _ = check(gpu, ix, v, i, None, 0.5, tol, 4)
        s = A.solve(v, i, 0.5, tol, 4)
        one = [sum(len(set(w[w >= 0])) <= 1 for w in np.concatenate([c, np.full(-len(c) % 64, -1)]).reshape(-1, 64)) for c in s["cell_of"]]
        print("soup tol", tol, "waves of one cell per level:", one, "of", (len(v) + 63) // 64, "chosen", list(st.chosen[:4]), "singles", st.singles,
              "kept", st.n_tris)
        assert dev is not None and st.degenerate_in > 0 and one[3] >= 280 and one[0] < 5
        if tol == 8.0:
            assert st.chosen[3] == 27 and st.singles == 0 and st.largest_cluster > 1000 and st.collapsed > 0
        if tol == 0.0:
            assert sum(st.chosen) < 300                                              # only exact duplicates and flukes merge


def test_identical_bytes_across_runs_and_table_sizes(gpu, monkeypatch):
    ix, v, i, k, res, lattice = small(gpu, "torus")
    grid = tuple(F(o) - F(0.5) * res for o in lattice)
    args = (res, res / F(4), 5, grid)
    assert A.simplify(v, i, *args, k, dry=True)[3]["cells"] >= 1024              # so that a table of 1024 cells has to grow
    first, st = ix.simplify_adaptive(*args)
    want = [a.tobytes() for a in first.read()]
    assert st.attempts == 1
    for _ in range(2):
        again, s2 = ix.simplify_adaptive(*args)
        assert [a.tobytes() for a in again.read()] == want and s2.result_bytes() == st.result_bytes() and again.ply() == first.ply()
    monkeypatch.setenv("GSDF_HIP_SIMPLIFY_CELLS_MIN", "1024")
    grown, s3 = ix.simplify_adaptive(*args)
    assert s3.attempts > 1 and s3.table_cells >= 2 * s3.cells
    assert [a.tobytes() for a in grown.read()] == want and s3.result_bytes() == st.result_bytes()
    _, s4 = ix.simplify_adaptive(*args, dry=True)
    assert s4.attempts > 1 and s4.result_bytes() == st.result_bytes()


def test_dual_contouring_handle_is_reproducible(gpu):
    """Two builds of the long box's handle: byte-identical adaptive results, and the twin's."""
    shape, res = dc_case("long-box")
    results = []
    for _ in range(2):
        ix = gpu.IndexedHIP.dual_contour(gpu.SDF3HIP(shape), res)
        grid = tuple(F(o) - F(0.5) * res for o in ix.mesh_stats.origin[:])
        dev, st = ix.simplify_adaptive(res, res / F(8), 5, grid)
        results.append([a.tobytes() for a in dev.read()] + [st.result_bytes(), dev.ply()])
    assert results[0] == results[1]
    v, i, k = ix.read()
    dev, st, _ = check(gpu, ix, v, i, k, res, res / F(8), 5, grid)
    assert st.n_tris < ix.n_tris and sum(st.chosen[1:]) > 0
    rep = dev.report()
    print("long box: F", ix.n_tris, "->", st.n_tris, "chosen", list(st.chosen[:5]), "singles", st.singles, "closed", rep.closed_oriented)


def test_simplify_adaptive_to(gpu):
    ix, v, i, k, res, lattice = small(gpu, "sphere")
    grid = tuple(F(o) - F(0.5) * res for o in lattice)
    max_tris = ix.n_tris // 6
    tol0 = res / F(64)
    out, so, used = ix.simplify_adaptive_to(max_tris, res, tol0, 5, grid)
    want = tol0
    while A.simplify(v, i, res, want, 5, grid, k, dry=True)[3]["n_tris"] > max_tris:
        want = F(want * F(2))
    assert 0 < out.n_tris == so.n_tris <= max_tris and F(used) == want and want > tol0
    tv, ti, tk, ts = A.simplify(v, i, res, want, 5, grid, k)
    v2, i2, k2 = out.read()
    assert (u32(v2) == u32(tv)).all() and (i2 == ti).all() and (k2 == tk).all() and so.result_bytes() == A.stats_bytes(ts)
    with pytest.raises(ValueError):
        ix.simplify_adaptive_to(0, res, tol0, 5, grid)
    with pytest.raises(ValueError):
        ix.simplify_adaptive_to(max_tris, res, 0.0, 5, grid)
    with pytest.raises(ValueError):
        ix.simplify_adaptive_to(8, res, tol0, 1, grid)                              # one level of cells of res never gets there


def test_errors(gpu):
    v, i = T.hand_meshes()["tet"]
    vn = np.vstack([v, [[np.nan, 0, 0]]]).astype(np.float32)
    ok = gpu.IndexedHIP.from_arrays(vn, i)                                    # NaN in a vertex no face names: fine
    assert check(gpu, ok, vn, i, None, 3.0, 0.5, 3)[0] is not None
    bad = np.vstack([i, [[4, 1, 0]]]).astype(np.uint32)
    with pytest.raises(gpu.HipError) as e:
        gpu.IndexedHIP.from_arrays(vn, bad).simplify_adaptive(3.0, 0.5, 3)
    assert e.value.code == -3 and e.value.msg.startswith("adaptive simplify: 1 used")
    ix = gpu.IndexedHIP.from_arrays(v, i)
    with pytest.raises(gpu.HipError) as e:
        ix.simplify_adaptive(6.0 / (1 << 17), 0.0, 2)
    assert e.value.code == -8 and "vertex 1 " in e.value.msg                  # GSDF_ERR_RESOLUTION
    check(gpu, ix, v, i, None, 6.0 / (1 << 17), 0.0, 2)
    with pytest.raises(gpu.HipError) as e:
        ix.simplify_adaptive(100.0, 100.0, 1)
    assert e.value.code == -1                                                 # GSDF_ERR_EMPTY_BUFFERS
    none, st = ix.simplify_adaptive(100.0, 100.0, 1, dry=True)
    assert none is None and (st.n_tris, st.n_verts, st.cells, st.collapsed, st.largest_cluster, st.chosen[0], st.singles) == (0, 0, 1, 4, 4, 1, 0)
    check(gpu, ix, v, i, None, 100.0, 100.0, 1)
    check(gpu, ix, v, i, None, 1.0, 100.0, 4)                                 # the top level swallows the tetrahedron
    for kw in (dict(cell=0.0), dict(cell=float("nan")), dict(tol=-1.0), dict(tol=float("inf")), dict(levels=0), dict(levels=17)):
        with pytest.raises(gpu.HipError) as e:
            ix.simplify_adaptive(**{**dict(cell=1.0, tol=0.0, levels=2), **kw})
        assert e.value.code == -3, kw


def test_example_adaptive(gpu, tmp_path):
    """examples/render_ply.py --adaptive as a child process: the PLY reads back with the counts the example printed, for a fixed
    tolerance with --project --report and for --max-tris. (A welded mesh's last bits differ from process to process, so the counts
    are the child's own: the contract says they may.)"""
    cmd = [sys.executable, os.path.join(ROOT, "examples", "render_ply.py"), "bolt", "--resdiv", "60", "--interpreter"]
    out = tmp_path / "a.ply"
    r = subprocess.run(cmd + ["--adaptive", "0.25", "--levels", "5", "--project", "--report", "-o", str(out)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"simplified adaptively within 0\.25 res, cells of 1 res x 1 \.\. 16: V (\d+) -> (\d+), F (\d+) -> (\d+) ", r.stdout)
    assert m, r.stdout
    v2, i2, n2 = ply.read_ply(out)
    assert (len(v2), len(i2)) == (int(m.group(2)), int(m.group(4))) and 0 < len(i2) < int(m.group(3)) and n2 is None
    assert r.stdout.count(" report: ") == 3 and "bolt projected report: " in r.stdout and "bolt deviation: " in r.stdout
    r = subprocess.run(cmd + ["--adaptive", "0.125", "--levels", "5", "--max-tris", str(len(i2) // 2), "-o", str(out)], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    m = re.search(r"simplified adaptively within (\S+) res, .*: V (\d+) -> (\d+), F (\d+) -> (\d+) ", r.stdout)
    v3, i3, _ = ply.read_ply(out)
    assert m and float(m.group(1)) > 0.25 and (len(v3), len(i3)) == (int(m.group(3)), int(m.group(5))) and 0 < len(i3) <= len(i2) // 2
