"""gsdf_hip_indexed_clean on the device against the numpy twin of its contract (tests/cleanref.py): vertices, faces, keys, normals and
the stats' leading block equal AS BYTES, the dry run's bytes equal to the real run's, the same error code where the twin raises. The
twin sees the mesh and the flags, and no device result."""
import ctypes as C
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import cleanref as K
import simplifyref as S
import toporef as T
from corpus import shapes3d
from gsdf_amd import ply
from scaffold.builder import Builder
from test_clean_ref import FLAGS, NEG0, hand_cases, pair_balance
from test_gpu_simplify import small, welded
from test_gpu_topo import check_against_twin as check_report

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EDGE_FIELDS = ("nonmanifold_edges", "misoriented_edges", "boundary_edges")


def raw(*arrays):
    return [None if a is None else np.ascontiguousarray(a).tobytes() for a in arrays]


def read_all(dev):
    return dev.read() + ((dev.read_normals() if dev.stats.has_normals else None),)


def check(gpu, ix, v, i, k, n, flags):
    """Device clean of handle `ix` against the twin's on (v, i, k, n): the result (or the same error), the stats, and the dry run.
    Returns (device mesh or None, device stats, twin result or None)."""
    merge, faces = bool(flags & K.MERGE_POSITIONS), bool(flags & K.FACES)
    _, dry = ix.clean(merge, faces, dry=True)
    want = K.clean(v, i, k, n, flags, dry=True)[4]
    assert {f: int(getattr(dry, f)) for f in K.STAT_FIELDS} == want
    assert dry.result_bytes() == K.stats_bytes(want)
    try:
        tw = K.clean(v, i, k, n, flags)
    except K.CleanError as e:
        with pytest.raises(gpu.HipError) as got:
            ix.clean(merge, faces)
        assert got.value.code == e.code == K.EMPTY_BUFFERS and dry.n_tris == 0, (got.value.msg, e.msg)
        return None, dry, None
    dev, st = ix.clean(merge, faces)
    assert st.result_bytes() == dry.result_bytes()
    assert raw(*read_all(dev)) == raw(*tw[:4])
    assert (dev.n_verts, dev.n_tris, dev.stats.has_normals) == (want["n_verts"], want["n_tris"], int(n is not None))
    finite = int(np.isfinite(v).all(axis=1).sum())
    assert (st.vert_attempts >= 1 and st.vert_table_cells >= 2 * (finite - st.merged_verts) and st.vert_probes >= finite) if merge else \
        (st.vert_attempts, st.vert_table_cells, st.vert_probes) == (0, 0, 0)
    assert (st.face_attempts >= 1 and st.face_table_cells >= 2 * st.face_sets and st.face_probes >= (st.face_sets > 0)) if faces else \
        (st.face_attempts, st.face_table_cells, st.face_probes) == (0, 0, 0)
    return dev, st, tw


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_cases(gpu, name):
    v, i = hand_cases()[name]
    k = (np.arange(len(v), dtype=np.uint64) * np.uint64(0x100000001) + np.uint64(7))
    ix = gpu.IndexedHIP.from_arrays(v, i, k)
    for flags in FLAGS:
        dev, st, _ = check(gpu, ix, v, i, k, None, flags)
        if dev is not None and st.duplicate_faces == 0:                       # (iii) on the device result: the keys name the classes
            _, i2, k2 = dev.read()
            assert pair_balance(k2[i2.astype(np.int64)].tolist()) == pair_balance(k[K.classes(v, flags)[i.astype(np.int64)]].tolist())


@pytest.mark.parametrize("name", sorted(T.hand_meshes()))
def test_hand_meshes(gpu, name):
    v, i = T.hand_meshes()[name]
    ix = gpu.IndexedHIP.from_arrays(v, i)
    for flags in FLAGS:
        check(gpu, ix, v, i, None, None, flags)


def test_bad_arguments(gpu):
    v, i = T.hand_meshes()["tet"]
    ix = gpu.IndexedHIP.from_arrays(v, i)
    st, h = gpu.CleanStats(), C.c_void_p()
    marker = bytes(st)
    for flags, reserved in ((0, (0, 0, 0)), (4, (0, 0, 0)), (7, (0, 0, 0)), (2, (0, 1, 0)), (1, (0, 0, 9))):
        o = gpu.CleanOpts(flags=flags, reserved=(C.c_uint32 * 3)(*reserved))
        for handle in (ix._h, None):                                            # refused before the handle is looked at
            h.value = 1
            assert gpu.lib().gsdf_hip_indexed_clean(handle, C.byref(o), C.byref(h), C.byref(st)) == K.BAD_ARGUMENT
            assert h.value is None and bytes(st) == marker
        if not any(reserved):                                                   # (the twin has flags only)
            with pytest.raises(K.CleanError):
                K.clean(v, i, None, None, flags)
    o = gpu.CleanOpts(flags=2)
    assert gpu.lib().gsdf_hip_indexed_clean(ix._h, C.byref(o), None, None) == K.BAD_ARGUMENT      # neither a handle nor stats asked for
    assert gpu.lib().gsdf_hip_indexed_clean(ix._h, None, C.byref(h), C.byref(st)) == K.BAD_ARGUMENT
    assert gpu.lib().gsdf_hip_indexed_clean(ix._h, C.byref(o), C.byref(h), None) == 0 and h.value
    gpu.IndexedHIP(h).close()


def test_normals_and_keys_are_carried(gpu):
    """A welded mesh with normals: nothing merges (what the twin says of it), and normals and keys come through bit for bit."""
    name = "torus"
    ix, v, i, k, res, _ = small(gpu, name)
    _, shapes = shapes3d()
    n = ix.normals(gpu.SDF3HIP(dict(shapes)[name]), res)
    dev, st, tw = check(gpu, ix, v, i, k, n, K.MERGE_POSITIONS)
    assert raw(*read_all(dev)) == raw(v, i, k, n) and st.merged_verts == tw[4]["merged_verts"]
    assert dev.ply() == ix.ply()
    check(gpu, ix, v, i, k, n, K.MERGE_POSITIONS | K.FACES)


def thin_wall():
    """A box 8 x 8 x 8 with a fin 8 x 0.5 x 8 standing on it: at resdiv 48 the fin is 1.2 res thick, thinner than a cell of 4 res."""
    b = Builder()
    return b.Union(b.NewBox(8, 8, 8, 0), b.Translate(b.NewBox(8, 0.5, 8, 0), 0, 0, 8))


def test_thin_wall_after_simplify(gpu):
    """What the pass exists for: clustering folds the fin's two sides onto each other, clean removes the opposite faces."""
    _, ix, res, lattice = welded(gpu, thin_wall(), 48)
    origin = tuple(np.float32(o) - np.float32(0.5) * res for o in lattice)
    cell = np.float32(4) * res
    v, i, _ = ix.read()
    sv, si, sk, _ = S.simplify(v, i, cell, origin)
    want = K.clean(sv, si, sk, None, K.FACES, dry=True)[4]
    assert want["opposite_faces"] > 0 and want["n_tris"] > 0, want             # (the condition the shape is a means to; 64 and 284 on the CPU weld)
    simp, _ = ix.simplify(cell, origin)
    assert raw(*simp.read()) == raw(sv, si, sk)
    dev, st, tw = check(gpu, simp, sv, si, sk, None, K.FACES)
    before, _ = check_report(simp, sv, si)
    after, _ = check_report(dev, tw[0], tw[1])
    print("thin wall: F", st.n_tris_in, "->", st.n_tris, "opposite", st.opposite_faces, "duplicate", st.duplicate_faces, "cancelled sets", st.cancelled_sets,
          {f: (int(getattr(before, f)), int(getattr(after, f))) for f in EDGE_FIELDS})
    # (iii) on the device result: a simplified mesh's keys are one per vertex, so they name the vertices across the two meshes
    v2, i2, k2 = dev.read()
    assert len(np.unique(sk)) == len(sk)
    if st.duplicate_faces == 0:                                                # (so on the CPU weld of this shape)
        assert pair_balance(k2[i2.astype(np.int64)].tolist()) == pair_balance(sk[si.astype(np.int64)].tolist())


def contended_soup():
    """20 000 vertices of which 5 000 are exact copies of others (every third copy with its zeros' signs flipped), a few non-finite;
    60 000 faces over a pool of 300 vertex numbers in runs of 64 consecutive faces of one set (rotated and reversed inside a run: the
    one-atomic-per-wave path), every tenth run balanced, some runs repeating another run's set, some faces degenerate."""
    rng = np.random.default_rng(41)
    v = rng.uniform(-3, 5, (20000, 3)).astype(np.float32)
    v[rng.random((20000, 3)) < 0.1] = 0
    dup = rng.choice(20000, 5000, replace=False)
    src = rng.integers(0, 20000, 5000)
    v[dup] = v[src]
    flip = dup[::3]
    v[flip] = np.where(v[flip] == 0, NEG0, v[flip])
    v[rng.choice(20000, 6, replace=False), rng.integers(0, 3, 6)] = [np.nan, np.inf, -np.inf, np.nan, np.inf, np.nan]
    pool = rng.choice(20000, 300, replace=False)
    n_runs = (60000 + 63) // 64
    sets = pool[np.array([rng.choice(300, 3, replace=False) for _ in range(n_runs)])]
    again = rng.choice(n_runs, n_runs // 8, replace=False)
    sets[again] = sets[(again * 7 + 3) % n_runs]
    i = np.repeat(sets, 64, axis=0)[:60000]
    rot = rng.integers(0, 3, 60000)
    i = np.take_along_axis(i, (np.arange(3)[None, :] + rot[:, None]) % 3, axis=1)
    rev = rng.random(60000) < 0.3
    run = np.arange(60000) // 64
    rev = np.where(run % 10 == 0, np.arange(60000) % 2 == 1, rev)               # every tenth run: 32 + and 32 -, a set that cancels
    i[rev] = i[rev][:, ::-1]
    i[::97, 1] = i[::97, 0]
    return v, np.ascontiguousarray(i, np.uint32)


CHILD = """
import hashlib, os, sys
sys.path[:0] = [%r, %r]
import numpy as np
from gsdf_amd import hip as gpu
from test_gpu_clean import contended_soup, raw
gpu.init(0)
v, i = contended_soup()
dev, st = gpu.IndexedHIP.from_arrays(v, i).clean(merge=True, faces=True)
print("DIGEST", hashlib.sha256(b"".join(raw(*dev.read())) + st.result_bytes()).hexdigest(), st.vert_attempts, st.face_attempts)
"""


def test_contended_soup_across_runs_and_table_sizes(gpu):
    v, i = contended_soup()
    ix = gpu.IndexedHIP.from_arrays(v, i)
    for flags in FLAGS:
        dev, st, tw = check(gpu, ix, v, i, None, None, flags)
        assert dev is not None and st.degenerate > 0
    assert st.merged_verts > 3000 and st.duplicate_faces > 10000 and st.opposite_faces > 10000 and st.cancelled_sets > 0 and st.largest_set >= 64
    assert st.vert_attempts == 1 and st.face_attempts == 1
    want = raw(*dev.read()) + [st.result_bytes()]
    again, s2 = ix.clean(merge=True, faces=True)
    assert raw(*again.read()) + [s2.result_bytes()] == want
    print("soup: merged", st.merged_verts, "sets", st.face_sets, "largest", st.largest_set, "probes per vertex", st.vert_probes / len(v), "face probes", st.face_probes,
          "ms", st.ms_merge, st.ms_faces, st.ms_result)
    env = dict(os.environ, GSDF_HIP_CLEAN_CELLS_MIN="64")
    r = subprocess.run([sys.executable, "-c", CHILD % (ROOT, os.path.join(ROOT, "tests"))], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [x for x in r.stdout.splitlines() if x.startswith("DIGEST")][0].split()
    assert line[1] == hashlib.sha256(b"".join(want)).hexdigest()
    assert int(line[2]) > 1 and int(line[3]) > 1                               # both tables grew in the child


def test_from_soup_of_a_minecraft_mesh(gpu):
    """The minecraft mesher's soup through from_soup: byte for byte what the twin makes of it. Its corners are lattice points, but
    formed per cube (origin + res i + res in one, origin + res (i + 1) in the next), so only the copies with equal bits join and the
    result need not be closed: the report is printed, not asserted. A cube soup on exact coordinates does close."""
    _, shapes = shapes3d()
    shape = dict(shapes)["sphere"]
    mc = gpu.MinecraftHIP(gpu.SDF3HIP(shape), np.float32(float(shape.Diagonal()) / 24))
    tris = np.array(mc.triangles_view())
    assert 100 < len(tris) < 40000
    dev, st = gpu.IndexedHIP.from_soup(tris)
    sv, si = tris.reshape(-1, 3), np.arange(3 * len(tris), dtype=np.uint32).reshape(-1, 3)
    tv, ti, tk, _, ts = K.clean(sv, si, None, None, K.MERGE_POSITIONS)
    assert raw(*dev.read()) == raw(tv, ti, tk) and st.result_bytes() == K.stats_bytes(ts) and dev.stats.has_normals == 0
    rep, _ = check_report(dev, tv, ti)
    print("minecraft soup: V", st.n_verts_in, "->", st.n_verts, "F", st.n_tris, "closed_oriented", rep.closed_oriented, "shells", rep.n_shells, "euler", rep.euler,
          {f: int(getattr(rep, f)) for f in EDGE_FIELDS})
    assert st.merged_verts > 0 and st.n_verts + st.merged_verts == st.n_verts_in
    cube, cs = gpu.IndexedHIP.from_soup(T.cube(0, 6)[0][T.cube(0, 6)[1].astype(np.int64)])
    crep = cube.report()
    assert (cs.n_verts_in, cs.n_verts, cs.n_tris, crep.closed_oriented, crep.euler, crep.volume) == (36, 8, 12, 1, 2, 216.0)


def test_result_is_an_ordinary_handle(gpu, tmp_path):
    name = "smoothunion"
    ix, v, i, k, res, origin = small(gpu, name)
    _, shapes = shapes3d()
    sdf = gpu.SDF3HIP(dict(shapes)[name])
    dev, st, tw = check(gpu, ix, v, i, k, None, K.MERGE_POSITIONS | K.FACES)
    cv, ci, ck = tw[:3]
    check_report(dev, cv, ci)
    simp, ss = dev.simplify(np.float32(3) * res, origin)
    sv, si, sk, want = S.simplify(cv, ci, np.float32(3) * res, origin)
    assert raw(*simp.read()) == raw(sv, si, sk) and ss.result_bytes() == S.stats_bytes(want)
    ex = dev.extract(None, drop_degenerate=True)
    assert raw(*ex.read()) == raw(*T.extract(cv, ci, ck, None, T.analyse(cv, ci)["shell_of_face"])[:3])
    dv = dev.deviation(sdf, np.float32(0.01) * res)
    assert dv.result_bytes() == gpu.IndexedHIP.from_arrays(cv, ci, ck).deviation(sdf, np.float32(0.01) * res).result_bytes()
    out = tmp_path / "c.ply"
    out.write_bytes(dev.ply())
    pv, pi, pn = ply.read_ply(out)
    assert raw(pv, pi) == raw(cv, ci) and pn is None


def test_same_bytes_whatever_the_handle_ran_before(gpu):
    name = "union"
    ix, v, i, k, res, origin = small(gpu, name)
    _, shapes = shapes3d()
    sdf = gpu.SDF3HIP(dict(shapes)[name])
    fresh = gpu.IndexedHIP.from_arrays(v, i, k)
    first, st = fresh.clean(merge=True, faces=True)
    want = raw(*first.read()) + [st.result_bytes()]
    acts = [lambda h: h.report(), lambda h: h.simplify(np.float32(3) * res, origin), lambda h: h.simplify_adaptive(res, np.float32(0.05) * res, 4, origin),
            lambda h: h.project(sdf, res, np.float32(0.001) * res, res), lambda h: h.clean(merge=False, faces=True, dry=True), lambda h: h.ply()]
    for act in acts:
        kept = act(fresh)
        again, s2 = fresh.clean(merge=True, faces=True)
        assert raw(*again.read()) + [s2.result_bytes()] == want
        del kept
    assert raw(*fresh.read()) == raw(v, i, k)                                   # and the handle's own mesh is what it was
