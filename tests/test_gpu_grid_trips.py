"""Every grid-stride kernel through three trips or more of its loop, at sizes a test can afford.

A launch sized by grid_for(n, CUs, workgroups per CU) takes a second trip on an MI355X only above half a million elements, so
the twin comparisons of the other modules run every such loop once. GSDF_HIP_GRID_CUS=1 (read at every handle creation) sizes the
grids for one CU: a trip is then 2 048 .. 65 536 elements long. Each case below creates handles with the knob unset, sets it,
proves it took hold (hip.grid_cus() == 1), creates the same handles again and holds their results to
  (a) the oracle or CPU twin the entry point's own module uses, bit for bit, and
  (b) the handles made with the knob unset: the same bytes (triangle soups as sorted sets).
It asserts its own size condition from tests/grid_trips.py: n >= 3 trip + 1 and n % trip != 0 for the kernels the table gives it.
The two kernels on a constant grid are reached with synthetic input instead (the last two cases)."""
import os
import struct

import numpy as np
import pytest

import corpus
from grid_trips import check_trips, trips_of
from oracle import oracle
from oracle.oracle import OracleSDF
from scaffold.builder import Builder

pytestmark = pytest.mark.gpu
KNOB = "GSDF_HIP_GRID_CUS"
F = np.float32


class Knob:
    def __init__(self, gpu, monkeypatch):
        self.gpu, self.mp = gpu, monkeypatch
        self.unset()

    def unset(self):
        self.mp.delenv(KNOB, raising=False)
        n, real = self.gpu.grid_cus(real=True)
        assert n == real > 1
        return real

    def one(self):
        self.mp.setenv(KNOB, "1")
        assert self.gpu.grid_cus() == 1
        return 1


@pytest.fixture
def knob(gpu, monkeypatch):
    return Knob(gpu, monkeypatch)


def u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def mismatch(a, b):
    return int(((u32(a) != u32(b)) & ~(np.isnan(a) & np.isnan(b))).sum())


def srt(t):
    t = np.ascontiguousarray(t, F).reshape(-1, 9)
    return t[np.lexsort(t.view(np.uint32).T[::-1])]


def same_set(a, b, what):
    a, b = srt(a), srt(b)
    assert a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all(), what


def same_cost(a, b):
    """A probe count against the knob-unset handle's. The order in which equal keys reach a table moves keys within their clusters,
    and the count with them, by a little; a per-lane sum flushed once per trip instead of once per kernel counts the first of T trips
    T times -- a factor (T + 1) / 2 >= 2 from three trips on -- and one flushed for the last trip alone leaves 1 / T <= 1 / 3."""
    return 2 * a > b and 2 * a < 3 * b


def points(shape, n):
    dim = 2 if shape.is2d else 3
    p = corpus.sample_points(shape, n_grid=4, n_rand=n - 4 ** dim - 1 - 2 * dim)
    assert len(p) == n
    return p


# ---- the knob ------------------------------------------------------------------------------------------------------------------------
def test_the_knob_is_read_per_handle_and_clamped(gpu, monkeypatch):
    monkeypatch.delenv(KNOB, raising=False)
    n, real = gpu.grid_cus(real=True)
    assert n == real > 1
    for text, want in (("1", 1), ("2", 2), ("0", real), ("-3", real), ("abc", real), ("100000", real), ("", real), (str(real), real)):
        monkeypatch.setenv(KNOB, text)
        assert gpu.grid_cus(real=True) == (want, real), text
    assert gpu.grid_cus(0) == real and gpu.lib().gsdf_hip_grid_cus(10 ** 6, None) == 0
    # a handle keeps the count it was created with, and so do the handles made from it: the knob set AFTER creation changes nothing
    s = Builder().Scene("bolt")
    res = F(float(s.Diagonal()) / 60)
    monkeypatch.delenv(KNOB)
    wide = gpu.SDF3HIP(s)
    monkeypatch.setenv(KNOB, "1")
    a, b = gpu.OctreeHIP(wide, res), gpu.OctreeHIP(gpu.SDF3HIP(s), res)
    same_set(a.RenderAll(), b.RenderAll(), "a program made before the knob was set, one made after")
    assert a.stats.evals == b.stats.evals and a.WriteBinarySTL() == oracle.write_stl(a.RenderAll())


# ---- evaluation ----------------------------------------------------------------------------------------------------------------------
def test_evaluate(gpu, knob):
    """Evaluate in 3-D with a 16-byte position stride and in 2-D (the staged path: K points per lane), evaluate_dev, and two
    submit / wait calls in flight (the host-mapped path: one point per lane) -- interpreter, then the per-tree kernels."""
    import torch
    b = Builder()
    s3, s2 = b.Scene("npt-flange"), dict(corpus.shapes2d()[1])["hexagon"]
    n = 3 * max(trips_of("eval_kernel", 1)) + 77
    nsub = 3 * min(trips_of("eval_kernel", 1)) + 77            # (a submit takes 2^18 points / 1 MiB of positions at most: one point per lane)
    check_trips("test_evaluate", 1, {"eval_kernel": n})
    assert nsub >= 3 * 64 * 256 + 1 and nsub % (64 * 256) != 0 and nsub * 12 <= 1 << 20
    p3, p2 = points(s3, n), points(s2, n)
    p16 = np.full((n, 4), 123.0, F)
    p16[:, :3] = p3
    want3, want2 = OracleSDF(s3.tree()).Evaluate(p3), OracleSDF(s2.tree()).Evaluate(p2)
    subs = [np.ascontiguousarray(p3[k * 1000:k * 1000 + nsub]) for k in range(2)]
    wide3, wide2 = gpu.SDF3HIP(s3), gpu.SDF2HIP(s2)
    ref3, ref2 = wide3.Evaluate(p16), wide2.Evaluate(p2)
    knob.one()
    for spec in (False, True):
        a3, a2 = gpu.SDF3HIP(s3), gpu.SDF2HIP(s2)
        if spec:
            a3.specialize(), a2.specialize()
        d3, d2 = a3.Evaluate(p16), a2.Evaluate(p2)
        assert mismatch(d3, want3) == 0 and mismatch(d2, want2) == 0, spec
        assert d3.tobytes() == ref3.tobytes() and d2.tobytes() == ref2.tobytes(), spec
        tp = torch.from_numpy(p3).cuda().contiguous()
        td = torch.full((n,), float("nan"), device="cuda")
        a3.evaluate_dev(tp.data_ptr(), 12, td.data_ptr(), n)
        torch.cuda.synchronize()
        assert td.cpu().numpy().tobytes() == ref3.tobytes(), spec
        outs = [np.full(nsub, np.nan, F) for _ in subs]
        tickets = [a3.submit(p_, d_) for p_, d_ in zip(subs, outs)]
        for k in (1, 0):
            a3.wait(tickets[k])
            assert outs[k].tobytes() == ref3[k * 1000:k * 1000 + nsub].tobytes(), (spec, k)
        assert a3.Evaluations() == 2 * n + 2 * nsub and a2.Evaluations() == n


def test_block_cache(gpu, knob):
    """BlockCachedSDF3 in front of a one-CU evaluator: the misses of one batch go to the program's Evaluate together."""
    from oracle.oracle import OracleBlockCachedSDF3
    s = Builder().Scene("bolt")
    n = 3 * max(trips_of("eval_kernel", 1)) + 77
    pos = points(s, n)
    pos[::7] = pos[1::7][:pos[::7].shape[0]]                   # exact repeats inside the batch: both miss
    co = OracleBlockCachedSDF3(OracleSDF(s.tree()), 0.01, 0.015, 0.005)
    want = co.Evaluate(pos)
    wide = gpu.BlockCachedSDF3HIP(gpu.SDF3HIP(s), 0.01, 0.015, 0.005)
    ref = wide.Evaluate(pos)
    knob.one()
    cg = gpu.BlockCachedSDF3HIP(gpu.SDF3HIP(s), 0.01, 0.015, 0.005)
    d = cg.Evaluate(pos)
    assert mismatch(d, want) == 0 and d.tobytes() == ref.tobytes()
    assert (cg.CacheHits(), cg.Evaluations()) == (co.hits, co.evals) == (wide.CacheHits(), wide.Evaluations())
    check_trips("test_block_cache", 1, {"eval_kernel": cg.Evaluations()})     # the misses: what the kernel was launched over
    again = cg.Evaluate(pos)                                                   # mostly hits now: the lossy cache answers
    assert mismatch(again, co.Evaluate(pos)) == 0 and cg.CacheHits() == co.hits > 0


def test_normals(gpu, knob):
    s = Builder().Scene("npt-flange")
    n = 3 * trips_of("normals_kernel", 1)[0] + 77
    check_trips("test_normals", 1, {"normals_kernel": n})
    pos = points(s, n)
    want = OracleSDF(s.tree()).normals_central_diff(pos, 1e-3)
    ref = gpu.SDF3HIP(s).normals(pos, 1e-3)
    knob.one()
    for spec in (False, True):
        sdf = gpu.SDF3HIP(s)
        if spec:
            sdf.specialize()
        got = sdf.normals(pos, 1e-3)
        assert mismatch(got.ravel(), want.ravel()) == 0 and got.tobytes() == ref.tobytes(), spec


# ---- pictures ------------------------------------------------------------------------------------------------------------------------
def test_images(gpu, knob):
    """render_image and render_picture (every conversion) of a 2-D part, 257 x 131 pixels: 33 667, ragged against every trip length."""
    from test_gpu_picture import _check_picture, _conversions, _example
    s = _example().scene("text")
    w, h = 257, 131
    check_trips("test_images", 1, {"image2_kernel": w * h, "image2_color_kernel": w * h})
    cpu = OracleSDF(s.tree())
    dc, cc = cpu.render_image(w, h)
    wide = gpu.SDF2HIP(s)
    ref_img = wide.render_image(w, h)
    ref_pic = [wide.render_picture(w, h, conv) for _, conv in _conversions(gpu, wide.Bounds())]
    knob.one()
    for spec in (False, True):
        sdf = gpu.SDF2HIP(s)
        if spec:
            sdf.specialize()
        dg, cg = sdf.render_image(w, h)
        assert mismatch(dg.ravel(), dc.ravel()) == 0 and (cg == cc).all(), spec
        assert dg.tobytes() == ref_img[0].tobytes() and cg.tobytes() == ref_img[1].tobytes(), spec
        _check_picture(gpu, sdf, s.tree(), w, h, ("text", spec))                     # the twin of every conversion, the oracle's distances
        for (name, conv), (rgba, dist) in zip(_conversions(gpu, sdf.Bounds()), ref_pic):
            a = sdf.render_picture(w, h, conv)
            assert a[0].tobytes() == rgba.tobytes() and a[1].tobytes() == dist.tobytes(), (name, spec)


def test_view_refill(gpu, knob, monkeypatch):
    """render3 in the refilling form (persistent workgroups, up to 4 per CU, whose lanes claim pixels): 83 x 47 pixels are 66 tiles of
    64 claims, four to every lane of the 1 024 that one CU holds; aa = 1 and aa = 2. The plain form launches a lane per claim (no
    cap): it runs beside it and must say the same."""
    import viewref
    s = Builder().Scene("bolt")
    w, h = 83, 47
    claims = -(-w // 8) * -(-h // 8) * 64
    check_trips("test_view_refill", 1, {"view_kernel": claims})
    wide = gpu.SDF3HIP(s)
    knob.one()
    narrow = [gpu.SDF3HIP(s), gpu.SDF3HIP(s).specialize()]
    for aa in (1, 2):
        v = gpu.view_orbit(s.Bounds(), 0.5, 0.4, aa=aa)
        tw = viewref.render(OracleSDF(s.tree()).Evaluate, v, w, h)
        monkeypatch.setenv("GSDF_HIP_VIEW_REFILL", "1")
        ref = wide.render3(v, w, h)
        for sdf in narrow:
            for refill in ("1", "0"):
                monkeypatch.setenv("GSDF_HIP_VIEW_REFILL", refill)
                e0 = sdf.Evaluations()
                rgba, depth, evals = sdf.render3(v, w, h)
                assert sdf.Evaluations() - e0 == int(tw["evals"].astype(np.int64).sum()), (aa, refill)
                assert (rgba == tw["rgba"]).all() and (u32(depth) == u32(tw["depth"])).all() and (evals == tw["evals"]).all(), (aa, refill)
                assert [x.tobytes() for x in (rgba, depth, evals)] == [x.tobytes() for x in ref], (aa, refill)
        assert 0.02 < np.isfinite(tw["depth"]).mean() < 0.98                          # rays that hit and rays that miss


# ---- meshers -------------------------------------------------------------------------------------------------------------------------
def _stats(m, fields=("n_tris", "evals", "pruned_leaves", "leaf_cubes", "active_leaves", "levels", "evals_prune", "evals_leaf", "cut_leaves")):
    return [int(getattr(m.stats, f)) for f in fields]


def test_octree(gpu, knob):
    """npt-flange and bolt at Diagonal() / 100: prune on and off, share_corners 0 / 1 / 2, two shards, the binary STL; records then
    march() where the packing kernel gets its three trips (npt-flange at / 140, bolt at / 200)."""
    b = Builder()
    for scene, rd_rec in (("npt-flange", 140), ("bolt", 200)):
        s = b.Scene(scene)
        cpu = OracleSDF(s.tree())
        res, res_rec = F(float(s.Diagonal()) / 100), F(float(s.Diagonal()) / rd_rec)
        ref, ref_rec = cpu.render_octree(res, 4096, True), cpu.render_octree(res_rec, 4096, True)
        knob.unset()
        wide = gpu.SDF3HIP(s)
        w_oc, w_rec = gpu.OctreeHIP(wide, res), gpu.OctreeHIP(wide, res_rec, payload=gpu.PAYLOAD_RECORDS)
        w_stats, w_rec_stats = _stats(w_oc), _stats(w_rec)
        w_tris, w_rec_tris = w_oc.RenderAll(), w_rec.march().RenderAll()
        knob.one()
        sdf = gpu.SDF3HIP(s)
        oc = gpu.OctreeHIP(sdf, res)
        assert oc.stats.levels == ref.levels == 8 and oc.TotalPruned() == ref.pruned and _stats(oc) == w_stats
        same_set(oc.RenderAll(), ref.tris, (scene, "oracle"))
        same_set(oc.RenderAll(), w_tris, (scene, "knob unset"))
        blob = oc.WriteBinarySTL()
        assert blob == oracle.write_stl(oc.RenderAll()) and struct.unpack_from("<I", blob, 80)[0] == oc.n_tris()
        off = gpu.OctreeHIP(sdf, res, prune=False)
        same_set(off.RenderAll(), ref.tris, (scene, "prune off"))                     # (pruning does not change the surface)
        assert off.TotalPruned() == 0 and int(off.stats.leaf_cubes) == 8 ** (oc.stats.levels - 1)
        evals = [int(oc.stats.evals_leaf)]
        for share in (1, 2):
            m = gpu.OctreeHIP(sdf, res, share_corners=share)
            same_set(m.RenderAll(), ref.tris, (scene, "share_corners", share))
            assert m.TotalPruned() == ref.pruned and _stats(m)[:1] + _stats(m)[2:6] == w_stats[:1] + w_stats[2:6]
            evals.append(int(m.stats.evals_leaf))
        assert sdf.info()["leaf_k"] == 4 and (evals[1], evals[2]) == (ref.evals_points_256, ref.evals_rows) and evals[2] < evals[0]   # (leaf_dense_kernel and the row form ran)
        parts = [gpu.OctreeHIP(sdf, res, shard_rank=r, shard_count=2) for r in range(2)]
        assert sum(p.n_tris() for p in parts) == ref.n_tris
        same_set(np.concatenate([p.RenderAll() for p in parts]), ref.tris, (scene, "two shards"))
        rec = gpu.OctreeHIP(sdf, res_rec, payload=gpu.PAYLOAD_RECORDS)
        assert rec.payload()[:2] == (gpu.PAYLOAD_RECORDS, int(rec.stats.cut_leaves)) and _stats(rec) == w_rec_stats and rec.TotalPruned() == ref_rec.pruned
        rec.march()
        same_set(rec.RenderAll(), ref_rec.tris, (scene, "records, oracle"))
        same_set(rec.RenderAll(), w_rec_tris, (scene, "records, knob unset"))
        S = min(oc.stats.levels - 3 + 1, 7)
        sizes = {"prune_spec_kernel": (8 ** S - 1) // 7, "leaf_eval_kernel": int(oc.stats.leaf_cubes), "leaf_dense_kernel": int(oc.stats.leaf_cubes),
                 "march_records_kernel": int(oc.stats.cut_leaves), "stl_kernel": oc.n_tris(), "pack_records_kernel": int(rec.stats.leaf_cubes),
                 "march_dense_kernel": int(rec.stats.cut_leaves)}
        print(scene, check_trips("test_octree", 1, sizes))


def test_octree_prune_chain(gpu, knob):
    """The per-level centre tests behind the speculative top run from ten levels on: npt-flange at Diagonal() / 400 (level 3:
    two workgroups per CU, 512 candidates a trip)."""
    import hashlib
    import json
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "mesh_digests.json")))["npt_flange_resdiv400"]
    s = Builder().Scene("npt-flange")
    res = np.uint32(gold["res_bits"]).view(F)
    ref = OracleSDF(s.tree()).render_octree(res, 4096, True)
    wide = gpu.OctreeHIP(gpu.SDF3HIP(s), res)
    knob.one()
    oc = gpu.OctreeHIP(gpu.SDF3HIP(s), res)
    assert oc.stats.levels == gold["levels"] == 10 and oc.n_tris() == gold["n_tris"] and oc.TotalPruned() == ref.pruned
    tg = srt(oc.RenderAll())
    assert hashlib.sha256(tg.tobytes()).hexdigest() == gold["sha256_sorted"]
    assert tg.tobytes() == srt(ref.tris).tobytes() == srt(wide.RenderAll()).tobytes() and _stats(oc) == _stats(wide)
    print(check_trips("test_octree_prune_chain", 1, {"prune_kernel": int(oc.stats.leaf_cubes) // 64}))


def test_flat(gpu, knob):
    """The flat renderer of npt-flange at Diagonal() / 200, whole and in three slabs."""
    s = Builder().Scene("npt-flange")
    res = F(float(s.Diagonal()) / 200)
    ref = OracleSDF(s.tree()).render_flat(res)
    nx, ny, nz = ref.grid
    wide = gpu.FlatHIP(gpu.SDF3HIP(s), res)
    knob.one()
    sdf = gpu.SDF3HIP(s)
    fl = gpu.FlatHIP(sdf, res)
    assert fl.Evaluations() == (nx + 1) * (ny + 1) * (nz + 1) and int(fl.stats.leaf_cubes) == nx * ny * nz and _stats(fl) == _stats(wide)
    same_set(fl.RenderAll(), ref.tris, "oracle")
    same_set(fl.RenderAll(), wide.RenderAll(), "knob unset")
    parts = [gpu.FlatHIP(sdf, res, shard_rank=r, shard_count=3) for r in range(3)]
    assert sum(p.n_tris() for p in parts) == ref.n_tris
    same_set(np.concatenate([p.RenderAll() for p in parts]), ref.tris, "three slabs")
    sizes = {"flat_grid_kernel": -(-(nx + 1) * (ny + 1) // 256) * -(-(nz + 1) // 4), "flat_cut_scan_kernel": -(-(nx + 1) * ny // 4096) * nz,
             "flat_march_list_kernel": -(-fl.n_tris() // 5)}
    print(check_trips("test_flat", 1, sizes))


def _span_blocks(tris, res, cells):
    """How many aligned blocks of cells[a] lattice cells per axis the bounding box of a mesh's vertices spans at least."""
    v = np.asarray(tris, np.float64).reshape(-1, 3)
    ext = (v.max(axis=0) - v.min(axis=0)) / float(res)
    return int(np.prod([max(1, int(ext[a] // cells[a])) for a in range(3)]))


def test_dual_contour(gpu, knob):
    """Dual contouring of npt-flange and bolt at Diagonal() / 100, plain and chiseled, against the oracle's triangle sets."""
    b = Builder()
    for scene in ("npt-flange", "bolt"):
        s = b.Scene(scene)
        cpu = OracleSDF(s.tree())
        res = F(float(s.Diagonal()) / 100)
        knob.unset()
        wide = gpu.SDF3HIP(s)
        refs = {ch: gpu.DualContourHIP(wide, res, chiseled=ch) for ch in (False, True)}
        knob.one()
        sdf = gpu.SDF3HIP(s)
        for ch in (False, True):
            want = cpu.render_dualcontour(res, ch)
            dc = gpu.DualContourHIP(sdf, res, chiseled=ch)
            assert dc.n_tris() == want.n_tris and dc.stats.levels == want.levels and _stats(dc) == _stats(refs[ch])
            same_set(dc.RenderAll(), want.tris, (scene, ch, "oracle"))
            same_set(dc.RenderAll(), refs[ch].RenderAll(), (scene, ch, "knob unset"))
        if scene == "npt-flange":
            k = int(sdf.info()["kernels"]["dc"].split("<")[1].split(",")[0])         # points per lane of the origin sweep: a tile is 8 x 8 x 4 K origins
            cubes, edges = int(dc.stats.leaf_cubes), int(dc.stats.active_leaves)
            tiles = max(_span_blocks(dc.RenderAll(), res, (8, 8, 4 * k)), -(-int(dc.stats.evals_prune) // (256 * k)))   # (an evaluated origin lies in a swept tile of 256 K)
            sizes = {"dc_origin_kernel": tiles, "dc_edges_kernel": -(-cubes // 1024), "dc_normals_kernel": -(-edges // 64),
                     "dc_place_kernel": cubes, "dc_quads_kernel": edges}
            print(scene, check_trips("test_dual_contour", 1, sizes))


def test_dc_grid_clear(gpu, knob):
    """The two kernels in front of dual contouring's origin sweep work on blocks of tiles: a lattice of nine levels gives them their
    trips -- a unit sphere at res 0.01, whose oracle is cheap."""
    s = Builder().NewSphere(1.0)
    res = F(0.01)
    want = OracleSDF(s.tree()).render_dualcontour(res)
    wide = gpu.DualContourHIP(gpu.SDF3HIP(s), res)
    knob.one()
    sdf = gpu.SDF3HIP(s)
    dc = gpu.DualContourHIP(sdf, res)
    assert dc.n_tris() == want.n_tris and dc.stats.levels == want.levels == 9 and _stats(dc) == _stats(wide)
    assert int(dc.stats.evals_prune) < 0.25 * 2 ** 24                                 # the block test cleared most of the lattice: there are tiles to fill
    same_set(dc.RenderAll(), want.tris, "oracle")
    same_set(dc.RenderAll(), wide.RenderAll(), "knob unset")
    k = int(sdf.info()["kernels"]["dc"].split("<")[1].split(",")[0])
    sizes = {"dc_block_test_kernel": 4 * _span_blocks(want.tris, res, (8, 8, 4 * k)), "dc_grid_clear_kernel": _span_blocks(want.tris, res, (32, 32, 16 * k))}
    print(check_trips("test_dc_grid_clear", 1, sizes))


def test_dual_contour_indexed(gpu, knob):
    """IndexedHIP.dual_contour of npt-flange at Diagonal() / 100 against tests/dcref.py, plain and chiseled."""
    import dcref as D
    s = Builder().Scene("npt-flange")
    res = F(float(s.Diagonal()) / 100)
    cpu = OracleSDF(s.tree())
    wide = gpu.SDF3HIP(s)
    refs = {ch: gpu.IndexedHIP.dual_contour(wide, res, chiseled=ch) for ch in (False, True)}
    knob.one()
    sdf = gpu.SDF3HIP(s)
    for ch in (False, True):
        tv, ti, tk, soup, q, ref = D.mesh(cpu, res, ch)
        ix = gpu.IndexedHIP.dual_contour(sdf, res, chiseled=ch)
        v, i, k = ix.read()
        assert (ix.n_verts, ix.n_tris) == (len(tv), len(ti)) and ix.n_tris == ref.n_tris
        assert k.tobytes() == tk.tobytes() and i.tobytes() == ti.tobytes() and v.tobytes() == tv.tobytes(), ch
        assert np.ascontiguousarray(v[i.reshape(-1)]).tobytes() == np.ascontiguousarray(ref.tris, F).tobytes(), ch    # the oracle's triangles in the oracle's order
        assert [a.tobytes() for a in ix.read()] == [a.tobytes() for a in refs[ch].read()] and ix.ply() == refs[ch].ply(), ch
        assert [int(getattr(ix.mesh_stats, f)) for f in ("n_tris", "evals", "leaf_cubes", "active_leaves", "levels")] == \
               [int(getattr(refs[ch].mesh_stats, f)) for f in ("n_tris", "evals", "leaf_cubes", "active_leaves", "levels")]
    edges = int(ix.mesh_stats.active_leaves)
    print(check_trips("test_dual_contour_indexed", 1, {"dci_count_kernel": edges, "dci_scatter_kernel": edges}))


def test_minecraft(gpu, knob):
    b = Builder()
    for scene in ("npt-flange", "bolt"):
        s = b.Scene(scene)
        res = F(float(s.Diagonal()) / 25)
        want = OracleSDF(s.tree()).render_minecraft(res)
        knob.unset()
        wide = gpu.MinecraftHIP(gpu.SDF3HIP(s), res)
        knob.one()
        mc = gpu.MinecraftHIP(gpu.SDF3HIP(s), res)
        assert mc.n_tris() == want.n_tris > 0 and mc.stats.levels == want.levels and _stats(mc) == _stats(wide)
        same_set(mc.RenderAll(), want.tris, (scene, "oracle"))
        same_set(mc.RenderAll(), wide.RenderAll(), (scene, "knob unset"))
        assert mc.WriteBinarySTL() == oracle.write_stl(mc.RenderAll())               # (stl_kernel on a mesh that is not the octree's)
        cubes = 8 ** (mc.stats.levels - 1)
        assert int(mc.stats.leaf_cubes) == cubes
        print(scene, check_trips("test_minecraft", 1, {"mcr_positions_kernel": cubes, "mcr_faces_kernel": cubes}))


# ---- the indexed chain ---------------------------------------------------------------------------------------------------------------
def _by_key(v, i, k):
    """An indexed mesh without its numbering: the keys in order, the positions in that order, the faces as sorted rows of keys."""
    order = np.argsort(k)
    faces = k[i.astype(np.int64)]
    return k[order], v[order], faces[np.lexsort(faces.T[::-1])]


def test_indexed_chain(gpu, knob):
    """bolt at Diagonal() / 200 (31 088 vertices, 62 168 faces, two shells, one of them the 24-face speck): weld before and after the
    march, normals, PLY, report / shells / shell_of / extract, simplify at 4 res, simplify_adaptive(res, res / 8, 5 levels) and a clean
    of the simplified mesh, each against its twin with every statistic its own module compares. Against the knob unset: a weld numbers
    its vertices in the order of its mesh's records, which is the mesher's own, so the two welds are compared by key (positions within the weld's own bound); everything after
    the weld runs once more on a handle of the SAME arrays made with the knob unset and gives the same bytes, table sizes and attempts
    (a probe count depends on the order in which equal keys reach the table: the twins' modules hold it to its lower bound)."""
    import cleanref as K
    import toporef as T
    import weldref as W
    from gsdf_amd import ply
    from test_gpu_clean import check as check_clean
    from test_gpu_simplify import check as check_simplify
    from test_gpu_simplify_adaptive import check as check_adaptive
    from test_gpu_topo import check_against_twin as check_report
    from test_weld_ref import POSITION_BOUND_DIV
    s = Builder().Scene("bolt")
    cpu = OracleSDF(s.tree())
    res = F(float(s.Diagonal()) / 200)
    step = F(float(res) * 1e-3)
    w_sdf = gpu.SDF3HIP(s)
    w_weld = gpu.OctreeHIP(w_sdf, res, payload=gpu.PAYLOAD_RECORDS).weld()
    knob.one()
    sdf = gpu.SDF3HIP(s)
    oc = gpu.OctreeHIP(sdf, res, payload=gpu.PAYLOAD_RECORDS)
    before = oc.weld()
    leaves = oc.records()[1]
    oc.march()
    ix = oc.weld()
    origin = tuple(F(o) - F(0.5) * res for o in oc.stats.origin[:])
    assert (ix.n_verts, ix.n_tris) == (31088, 62168)                               # tests/test_weld_ref.py: MANIFOLD_SCENES
    # weld: the twin over the device's records, before and after the march
    vt, it, kt, soup = W.weld(cpu, leaves, np.array(oc.stats.origin[:], F), F(oc.stats.res))
    assert (u32(soup) == u32(oc.RenderAll().reshape(-1, 3))).all()
    for h in (before, ix):
        v, i, k = h.read()
        assert v.shape == vt.shape and (u32(v) == u32(vt)).all() and (i == it).all() and (k == kt).all()
        assert h.ply() == ply.ply_bytes(vt, it)
        assert (h.stats.table_cells, h.stats.attempts) == (w_weld.stats.table_cells, w_weld.stats.attempts) and h.stats.probes >= 3 * h.n_tris and same_cost(h.stats.probes, w_weld.stats.probes)
    v, i, k = ix.read()
    # (a welded vertex has the position of its first slot, and the slots of one lattice edge agree within res / 64: tests/test_weld_ref.py)
    (ka, va, fa), (kb, vb, fb) = _by_key(v, i, k), _by_key(*w_weld.read())
    assert ka.tobytes() == kb.tobytes() and fa.tobytes() == fb.tobytes() and float(np.abs(va.astype(np.float64) - vb.astype(np.float64)).max()) <= float(res) / POSITION_BOUND_DIV
    # the same arrays on a handle made with the knob unset
    knob.unset()
    wide = gpu.IndexedHIP.from_arrays(v, i, k)
    w_plain = wide.ply()
    w_normals = wide.normals(w_sdf, step)
    w_ply, w_rep, w_shells, w_shell_of = wide.ply(), wide.report(), wide.shells(), wide.shell_of()
    w_simp, w_sst = wide.simplify(F(4) * res, origin)
    w_adap, w_ast = wide.simplify_adaptive(res, res / F(8), 5, origin)
    w_clean, w_cst = w_simp.clean(True, True)
    knob.one()
    assert ix.ply() == w_plain
    # normals and the PLY with them
    n = ix.normals(sdf, step)
    assert mismatch(n.ravel(), cpu.normals_central_diff(v, step).ravel()) == 0 and n.tobytes() == w_normals.tobytes()
    assert ix.ply() == ply.ply_bytes(v, i, n) == w_ply
    # report, shells, shell numbers, extract
    rep, tw = check_report(ix, v, i)
    assert rep.n_shells == 2 and rep.closed_oriented == 1 and (rep.used_verts, rep.n_tris, rep.euler) == (31088, 62168, 4)
    assert 24 in ix.shells()["n_tris"].tolist()
    assert rep.result_bytes() == w_rep.result_bytes() and (rep.table_cells, rep.attempts) == (w_rep.table_cells, w_rep.attempts) and rep.probes >= rep.edges and same_cost(rep.probes, w_rep.probes)
    assert ix.shells().tobytes() == w_shells.tobytes() and all((a == b).all() for a, b in zip(ix.shell_of(), w_shell_of))
    for keep in (np.array([True, False]), np.array([False, True])):
        ex = ix.extract(keep)
        tv, ti, tk, _ = T.extract(v, i, k, None, tw["shell_of_face"], keep)
        assert [a.tobytes() for a in ex.read()] == [tv.tobytes(), ti.tobytes(), tk.tobytes()]
        assert [a.tobytes() for a in ex.read()] == [a.tobytes() for a in wide.extract(keep).read()]
    # simplify, adaptive simplify, clean of the simplified mesh: the twins with their statistics, then the knob-unset handle's
    simp, sst, stw = check_simplify(gpu, ix, v, i, F(4) * res, origin)
    assert simp is not None and sst.result_bytes() == w_sst.result_bytes() and (sst.table_cells, sst.attempts) == (w_sst.table_cells, w_sst.attempts) and same_cost(sst.probes, w_sst.probes)
    assert [a.tobytes() for a in simp.read()] == [a.tobytes() for a in w_simp.read()]
    adap, ast, _ = check_adaptive(gpu, ix, v, i, k, res, res / F(8), 5, origin)
    assert adap is not None and ast.result_bytes() == w_ast.result_bytes() and (ast.table_cells, ast.attempts) == (w_ast.table_cells, w_ast.attempts) and same_cost(ast.probes, w_ast.probes)
    assert [a.tobytes() for a in adap.read()] == [a.tobytes() for a in w_adap.read()]
    cl, cst, _ = check_clean(gpu, simp, stw[0], stw[1], stw[2], None, K.MERGE_POSITIONS | K.FACES)
    assert cl is not None and cst.opposite_faces > 0 and cst.result_bytes() == w_cst.result_bytes()
    assert (cst.vert_table_cells, cst.face_table_cells, cst.vert_attempts, cst.face_attempts) == (w_cst.vert_table_cells, w_cst.face_table_cells, w_cst.vert_attempts, w_cst.face_attempts)
    assert [a.tobytes() for a in cl.read()] == [a.tobytes() for a in w_clean.read()] and same_cost(cst.vert_probes, w_cst.vert_probes) and same_cost(cst.face_probes, w_cst.face_probes)
    print("probes, one CU / knob unset:", [(int(a), int(b)) for a, b in ((ix.stats.probes, w_weld.stats.probes), (rep.probes, w_rep.probes), (sst.probes, w_sst.probes), (ast.probes, w_ast.probes), (cst.vert_probes, w_cst.vert_probes), (cst.face_probes, w_cst.face_probes))])
    V, Fc = ix.n_verts, ix.n_tris
    sizes = {"weld_keys_kernel": int(oc.stats.cut_leaves), "weld_insert_kernel": 3 * Fc, "ply_verts_kernel": 3 * V, "ply_faces_kernel": -(-13 * Fc // 4),
             "topo_maxbits_kernel": 3 * V, "simplify_insert_kernel": V, "simplify_place_kernel": int(sst.table_cells), "adaptive_insert_kernel": V,
             "adaptive_place_kernel": int(ast.table_cells), "adaptive_named_kernel": int(ast.n_verts)}
    print(check_trips("test_indexed_chain", 1, sizes))
    check_trips("test_indexed_chain", 1, dict(sizes, ply_verts_kernel=6 * V))      # (and the vertex block with normals)


def test_clean_from_soup(gpu, knob):
    """from_soup -- a clean that merges equal positions -- of the bolt's soup at Diagonal() / 200: 186 504 vertices through the vertex
    table's three capped kernels, against tests/cleanref.py."""
    import cleanref as K
    from test_gpu_clean import check as check_clean
    s = Builder().Scene("bolt")
    res = F(float(s.Diagonal()) / 200)
    soup = np.ascontiguousarray(OracleSDF(s.tree()).render_octree(res).tris, F)
    v = soup.reshape(-1, 3)
    i = np.arange(len(v), dtype=np.uint32).reshape(-1, 3)
    wide, w_st = gpu.IndexedHIP.from_soup(soup)
    knob.one()
    raw = gpu.IndexedHIP.from_arrays(v, i)
    dev, st, tw = check_clean(gpu, raw, v, i, None, None, K.MERGE_POSITIONS)
    ix, st2 = gpu.IndexedHIP.from_soup(soup)
    assert st2.result_bytes() == st.result_bytes() == w_st.result_bytes() and st.merged_verts > 0
    assert (st2.vert_table_cells, st2.vert_attempts) == (w_st.vert_table_cells, w_st.vert_attempts) and same_cost(st2.vert_probes, w_st.vert_probes) and same_cost(st.vert_probes, w_st.vert_probes)
    assert [a.tobytes() for a in ix.read()] == [a.tobytes() for a in dev.read()] == [a.tobytes() for a in wide.read()]
    print(check_trips("test_clean_from_soup", 1, {"clean_vert_insert_kernel": len(v), "clean_vert_class_kernel": len(v), "clean_named_kernel": len(v)}))


def test_rays_and_projection(gpu, knob):
    """raycast, IndexedHIP.thickness and project (dry and not) on one-CU handles. ray_kernel and project_kernel are launched with one
    workgroup per 256 rays or vertices whatever the CU count (tests/test_grid_census.py holds them to that), so there is no trip to
    count: the case is here for the entry points' statistics -- evals, the status counts, steps_max -- against tests/rayref.py and
    tests/projectref.py on the bolt's 31 088 vertices, and against the knob unset."""
    from test_gpu_project import check as check_project, opts_for
    from test_gpu_ray import check_rays, check_thickness, corner_rays, thickness_opts
    s = Builder().Scene("bolt")
    cpu = OracleSDF(s.tree())
    res = F(float(s.Diagonal()) / 200)
    soup = np.ascontiguousarray(cpu.render_octree(res).tris, F)
    welded, _ = gpu.IndexedHIP.from_soup(soup)
    v, i, k = welded.read()
    o, r = corner_rays(s.Bounds(), 3 * 2048 + 77, 61)
    r = (r / np.linalg.norm(r, axis=1, keepdims=True)).astype(F)                      # (unit directions: t is a length, tmax the bounds' diagonal)
    kw = dict(tmax=F(s.Diagonal()), tol=F(res / F(1024)), max_steps=96, refine=8, thin=F(0.5))
    w_sdf = gpu.SDF3HIP(s)
    w_rays = w_sdf.raycast(o, r, **kw)
    w_thick = welded.thickness(w_sdf, **thickness_opts(res))
    w_proj, w_pst = welded.project(w_sdf, **opts_for(res))
    knob.one()
    sdf, ix = gpu.SDF3HIP(s), gpu.IndexedHIP.from_arrays(v, i, k)
    dev, _ = check_rays(gpu, sdf, cpu.Evaluate, o, r, "bolt", **kw)
    assert [x.tobytes() for x in dev[:4]] == [x.tobytes() for x in w_rays[:4]] and dev[4].result_bytes() == w_rays[4].result_bytes()
    th = check_thickness(ix, sdf, cpu.Evaluate, v, "bolt", **thickness_opts(res))
    assert th[0].tobytes() == w_thick[0].tobytes() and th[1].tobytes() == w_thick[1].tobytes() and th[2].result_bytes() == w_thick[2].result_bytes()
    pr, pst, _ = check_project(ix, sdf, cpu.Evaluate, v, "bolt", **opts_for(res))
    assert pst.result_bytes() == w_pst.result_bytes() and [x.tobytes() for x in pr.read() + pr.fit()] == [x.tobytes() for x in w_proj.read() + w_proj.fit()]
    assert dev[4].count[1] + dev[4].count[2] > 0 and pst.steps_max > 1


# ---- the gather ----------------------------------------------------------------------------------------------------------------------
def test_gather(gpu, knob):
    """Two ranks (threads of this process, the loopback transport) mesh their shards as records and gather them: the communicator's own
    CU count sizes the march of the gathered records, and it is created with the knob set."""
    from test_gpu_gather import _loopback_world
    s = Builder().Scene("npt-flange")
    res = F(float(s.Diagonal()) / 100)
    want = OracleSDF(s.tree()).render_octree(res, 4096, True)
    whole = gpu.OctreeHIP(gpu.SDF3HIP(s), res)
    knob.one()

    def work(r, comm):
        mine = gpu.OctreeHIP(gpu.SDF3HIP(s), res, shard_rank=r, shard_count=2, payload=gpu.PAYLOAD_RECORDS)
        g, counts, gs = mine.gatherv_start(comm, gpu.GATHER_ALL, 0).wait()
        return g.RenderAll(), counts, int(mine.stats.cut_leaves)

    outs = _loopback_world(gpu, 2, work)
    for tris, counts, _ in outs:
        assert sum(counts) == want.n_tris
        same_set(tris, want.tris, "oracle")
        same_set(tris, whole.RenderAll(), "knob unset")
    print(check_trips("test_gather", 1, {"march_dense_kernel": sum(o[2] for o in outs)}))


# ---- contours: evaluated through the one-CU Evaluate; their own capped kernels are on constant grids (below) ------------------------------
def test_contours(gpu, knob):
    """outline, slices, simplify and measures with the knob set: the text plate at Diagonal() / 120, seven slices of the bolt. Of the
    contour kernels only cmeas_maxbits_kernel is capped, by a constant (the next case); the knob reaches the program's Evaluate under
    the lattices, which stay below three of its trips here -- its own case is test_evaluate. No size condition: parity alone."""
    import contourref
    import contoursimpref as CS
    from test_gpu_contour import same, same_handles
    from test_gpu_contour_simplify import check, check_measures
    from test_gpu_picture import _example
    s2, s3 = _example().scene("text"), Builder().Scene("bolt")
    bb = s3.Bounds()
    res3 = F(float(s3.Diagonal()) / 60)
    z = contourref.layer_heights(bb, F(F(bb[5] - bb[2]) / F(7)))
    knob.unset()
    wide2 = gpu.SDF2HIP(s2)
    res2 = contourref.res_for(wide2.Bounds(), 120)
    w_out, w_sl = gpu.ContourHIP.outline(wide2, res2), gpu.ContourHIP.slices(gpu.SDF3HIP(s3), res3, z)
    knob.one()
    for what, dev, ref, wide, res in (("text", gpu.ContourHIP.outline(gpu.SDF2HIP(s2), res2), contourref.of_oracle(s2.tree(), res2), w_out, res2),
                                      ("bolt", gpu.ContourHIP.slices(gpu.SDF3HIP(s3), res3, z), contourref.of_oracle(s3.tree(), res3, z), w_sl, res3)):
        same(dev, ref, what)
        same_handles(dev, wide, (what, "knob unset"))
        loops = CS.Loops.of(dev)
        got, want, _ = check(gpu, dev, loops, F(res / F(8)), 8, 1, what)
        check_measures(dev, loops, what)
        check_measures(got, want, (what, "simplified"))
        assert dev.n_loops >= 7


# ---- the two constant caps, reached without the knob ----------------------------------------------------------------------------------------
def test_contour_measures_past_the_cap(gpu):
    """cmeas_maxbits_kernel runs on 1 024 workgroups at most: 140 003 vertices (280 006 coordinates) take it into a second, ragged
    trip. Seven regular polygons of unequal size on a grid of 1 / 64: measures() and the dry simplify against tests/contoursimpref.py."""
    import contoursimpref as CS
    from test_gpu_contour_simplify import check, check_measures, upload
    sizes = [50001, 40002, 30000, 12000, 5000, 2000, 1000]
    loops = [(np.round(np.asarray(CS.circle(n, 100.0 + 37 * k), np.float64) * 64) / 64).astype(F) for k, n in enumerate(sizes)]
    ref = CS.pack(loops)
    V = len(ref.xy)
    trip = trips_of("cmeas_maxbits_kernel", 0)[0]
    assert V == 140003 and V % 64 != 0 and 2 * V > trip == 1024 * 256 and (2 * V) % trip != 0
    dev = upload(gpu, ref)
    check_measures(dev, ref, "polygons")
    got, want, st = check(gpu, dev, ref, F(0.05), 8, 1, "polygons")
    assert st["n_verts_out"] < V
    check_measures(got, want, "polygons, simplified")


def test_block_scan_three_counts_per_thread(gpu):
    """block_scan_kernel is one workgroup of 1 024 threads that take ceil(n / 1 024) block counts each: more than 3 072 counts -- the
    slots of a clean that keeps 263 238 faces of a grid mesh, 256 to a count -- give every thread four. A 363 x 363 grid of quads with
    700 faces said twice and 300 said once more the other way round, against tests/cleanref.py."""
    import cleanref as K
    from test_gpu_clean import check as check_clean
    n = 363
    g = np.arange(n + 1, dtype=F)
    X, Y = np.meshgrid(g, g, indexing="xy")
    v = np.stack([X.ravel(), Y.ravel(), np.zeros((n + 1) ** 2, F)], 1).astype(F)
    q = (np.arange(n)[:, None] * (n + 1) + np.arange(n)[None, :]).ravel()
    i = np.concatenate([np.stack([q, q + 1, q + n + 2], 1), np.stack([q, q + n + 2, q + n + 1], 1)]).astype(np.uint32)
    rng = np.random.default_rng(4)
    pick = rng.permutation(len(i))
    i = np.concatenate([i, i[pick[:700]], i[pick[700:1000]][:, ::-1]])
    i = np.ascontiguousarray(i[rng.permutation(len(i))])
    dev, st, tw = check_clean(gpu, gpu.IndexedHIP.from_arrays(v, i), v, i, None, None, K.FACES)
    assert (st.duplicate_faces, st.opposite_faces, st.cancelled_sets) == (700, 600, 300) and dev.n_tris == 2 * n * n - 300
    counts = -(-3 * dev.n_tris // 256)
    print(check_trips("test_block_scan_three_counts_per_thread", 0, {"block_scan_kernel": counts}))
