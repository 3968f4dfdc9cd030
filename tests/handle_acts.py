"""A table of acts on a program handle, for tests/test_gpu_handle_history.py.

A program handle (gsdf_program, gsdf_amd/csrc/abi_program.h) outlives every call made on it: three grow-only octree workspaces that
dual contouring and the flat renderer borrow from, the dc_* and flat_* arenas, four staging slots with tickets, a counter block each
for projection and rays, the per-tree kernels a background build swaps in, and the size hints one mesh leaves for the next
(last_tris, last_recs, rec_blocks, last_dc_cubes). Finished meshes hand their triangle buffers to a process-wide pool.

An ACT is one use of the public binding (gsdf_amd/hip.py) on a handle at one RUNG of a resolution ladder. It returns a Result:

  canon   {label: bytes} that the oracle (OracleSDF) also gives -- want(tree, rung), computed once per (tree, rung) and shared:
          triangles sorted by bit pattern, arrays by tobytes(), the statistics the oracle reports as int64;
  more    {label: bytes} that only the device has: compared with the same act on a FRESH handle (the property is independence
          of history; the CPU twins of these entry points are held to the device elsewhere). Times are never in either;
  live    the result objects the act leaves behind (mesh, indexed mesh, contour) with the bytes of their first read, for a
          second read after whatever came next;
  evals   what the handle's Evaluations() must have grown by, where the existing tests state that (Evaluate, submit / wait,
          projection, rays); None elsewhere.

The CPU tests at the end check the table itself: every oracle-backed expectation exists, the ladder's counts, the sizing rule that
sends an upward step through overflow -> rerun, the size bound, and that the comparators fail on another rung's expectation and on
one flipped bit."""
import threading

import numpy as np
import pytest

import fuzz_trees
from contourref import res_for
from oracle.oracle import OracleSDF
from scaffold.builder import Builder

F = np.float32
LADDER = (12, 33, 96, 150)          # Diagonal / these: octree (and all its forms), flat
DC_LADDER = (20, 60)                # dual contouring, plain, chiseled and indexed: rungs 0, 1 -> 20; 2, 3 -> 60
MC_LADDER = (12, 33)                # minecraft (every cube of the lattice is evaluated: at most 9 levels)
SLICE_LADDER = (16, 40, 96, 150)    # contour lattices: xy diagonal / these
EVAL_SIZES = (1, 257, 4097, 87383)  # ragged; 87 381 positions of 12 bytes are the last small call (1 MiB, abi_eval.hip: kSmallPos)
NORMAL_SIZES = (1, 257, 1025, 4097)
IMAGE_SIZES = ((17, 13), (64, 48), (257, 131), (300, 200))
MAX_TRIS = 80000
# the oracle's counts the ladder was chosen for (every upward step overflows the buffer the smaller mesh asks for)
COUNTS = {"bolt": (160, 1412, 13808, 34668), "fuzz": (400, 3368, 30872, 74452)}
DC_COUNTS_BOLT = (496, 5140)
BAD_ARGUMENT, DIMENSION, RESOLUTION = -3, -7, -8
IN_FLIGHT = "an octree mesh of this program is in flight"


# ---------------- trees ----------------
class Tree:
    def __init__(self, name, shape, builder):
        self.name, self.shape, self._b = name, shape, builder
        self.bb = np.asarray(shape.Bounds(), F)
        self.dim = 2 if float(self.bb[5] - self.bb[2]) == 0 else 3
        self.diag = float(shape.Diagonal()) if self.dim == 3 else float(res_for(self.bb, 1))

    def res(self, div):
        return F(self.diag / div)

    def points(self, n, seed):
        """n points of a box 1.2 times the bounds, the same for every caller."""
        rng = np.random.default_rng([seed, n, self.dim])
        d = self.dim
        lo, hi = self.bb[:d], self.bb[3:3 + d]
        c, h = (lo + hi) * F(0.5), (hi - lo) * F(0.6)
        return np.ascontiguousarray(c + (rng.random((n, d), F) * F(2) - F(1)) * h, F)


_LOCK = threading.RLock()
_TREES, _ORACLES, _WANT = {}, {}, {}


def tree(name):
    with _LOCK:
        if name not in _TREES:
            if name == "bolt":                  # a screw: column bricks with the kept atan2
                b = Builder()
                _TREES[name] = Tree(name, b.Scene("bolt"), b)
            elif name == "fuzz":                # a CSG tree
                b, shapes = fuzz_trees.random_shapes(3, 6, depth=4)
                _TREES[name] = Tree(name, shapes[0], b)
            elif name == "flat2d":
                b, shapes = fuzz_trees.random_shapes2d(3, 4, depth=3)
                _TREES[name] = Tree(name, shapes[0], b)
            else:
                raise KeyError(name)
        return _TREES[name]


TREES3, TREE2 = ("bolt", "fuzz"), "flat2d"


def _cached(key, make):
    """make() once per key, under the lock (the oracle's evaluator is not shared between threads); the value is never written to."""
    with _LOCK:
        if key not in _WANT:
            _WANT[key] = make()
        return _WANT[key]


def oracle(t):
    with _LOCK:
        if t.name not in _ORACLES:
            _ORACLES[t.name] = OracleSDF(t.shape.tree())
        return _ORACLES[t.name]


# ---------------- canonical forms ----------------
def ints(*v):
    return np.array([int(x) for x in v], np.int64).tobytes()


def sorted_tris(t):
    t = np.ascontiguousarray(t, F).reshape(-1, 9)
    return t[np.lexsort(t.view(np.uint32).T[::-1])]


def tri_bytes(t):
    return sorted_tris(t).tobytes()


def differing(got, want):
    """The labels at which two canonical forms differ (a label only one of them has differs)."""
    return sorted(k for k in set(got) | set(want) if got.get(k) != want.get(k))


def check(got, want, what):
    bad = differing(got, want)
    assert not bad, (what, "differs at", bad, {k: (len(got.get(k, b"")), len(want.get(k, b""))) for k in bad})


class Live:
    """A result object left behind, how to read it again, and the bytes of its first read."""

    def __init__(self, obj, read):
        self.obj, self._read = obj, read
        self.first = read(obj)

    def reread(self, what):
        check(self._read(self.obj), self.first, (what, "second read of a live result"))

    def close(self):
        o, self.obj = self.obj, None
        if o is not None:
            o._free() if hasattr(o, "_free") else o.close()


class Result:
    def __init__(self, canon=None, more=None, live=(), evals=None):
        self.canon, self.more, self.live, self.evals = dict(canon or {}), dict(more or {}), list(live), evals

    def both(self):
        return {**self.canon, **{"+" + k: v for k, v in self.more.items()}}

    def close(self):
        for l in self.live:
            l.close()


class Ctx:
    """What an act runs on: the binding, the tree, the handle, and the fixed small indexed mesh of the tree (made on another handle)."""

    def __init__(self, gpu, t, sdf, fixed=None):
        self.gpu, self.t, self.sdf, self.fixed = gpu, t, sdf, fixed


def make_fixed(gpu, t):
    """The welded octree mesh of the tree at the ladder's second rung, made on a handle of its own that is then dropped."""
    other = gpu.SDF3HIP(t.shape)
    oc = gpu.OctreeHIP(other, t.res(LADDER[1]), payload=gpu.PAYLOAD_RECORDS)
    ix = oc.weld()
    oc._free()
    other.close()
    return ix


def fresh_ctx(gpu, t, fixed=None):
    return Ctx(gpu, t, gpu.SDFHIP(t.shape), fixed)


# ---------------- reading live objects ----------------
def read_mesh(gpu):
    def read(m):
        st = gpu.MeshStats()
        gpu._check(gpu.lib().gsdf_hip_mesh_stats_get(m._mesh, st))
        return {"raw": m.RenderAll().tobytes(), "stats": bytes(st)}
    return read


def read_indexed(ix):
    v, i, k = ix.read()
    return {"verts": v.tobytes(), "idx": i.tobytes(), "keys": k.tobytes()}


def read_projected(ix):
    return {**read_indexed(ix), **{"fit%d" % n: a.tobytes() for n, a in enumerate(ix.fit())}}


def read_contour(gpu):
    def read(c):
        xy, keys = np.empty((c.n_verts, 2), F), np.empty(c.n_verts, np.uint32)
        start, layer = np.empty(c.n_loops + 1, np.uint32), np.empty(c.n_loops, np.uint32)
        gpu._check(gpu.lib().gsdf_hip_contour_read(c._h, xy.ctypes.data, keys.ctypes.data, start.ctypes.data, layer.ctypes.data))
        return {"xy": xy.tobytes(), "keys": keys.tobytes(), "loop_start": start.tobytes(), "loop_layer": layer.tobytes(), "stats": c.stats.result_bytes()}
    return read


# ---------------- the oracle's meshes ----------------
def oracle_mesh(t, kind, div, flag=False):
    def make():
        o, res = oracle(t), t.res(div)
        if kind == "octree":
            r = o.render_octree(res, 4096, flag)       # flag: prune
        elif kind == "flat":
            r = o.render_flat(res, 4096, 1)
        elif kind == "dc":
            r = o.render_dualcontour(res, flag)        # flag: chiseled
        else:
            r = o.render_minecraft(res)
        r.sorted_bytes = tri_bytes(r.tris)
        return r
    return _cached((t.name, kind, div, bool(flag)), make)


MESH_MORE = ("evals", "leaf_cubes", "active_leaves", "cut_leaves", "evals_prune", "evals_leaf", "pruned_leaves", "levels")


def mesh_result(cx, m, canon_fields, extra=None):
    st = m.stats
    canon = {"tris": tri_bytes(m.RenderAll()), **{f: ints(getattr(st, f)) for f in canon_fields}}
    more = {f: ints(getattr(st, f)) for f in MESH_MORE if f not in canon_fields}
    more.update(extra or {})
    return Result(canon, more, [Live(m, read_mesh(cx.gpu))])


# ---------------- acts ----------------
class Act:
    name, dim, family, error = "", 3, None, False
    oracle_backed = True

    def want(self, t, rung):
        """The oracle's canonical answer, or None where the answer is the same act's on a fresh handle."""
        return None

    def run(self, cx, rung):
        raise NotImplementedError

    def n_tris(self, t, rung):
        """Triangles of the largest mesh this act makes at this rung (0: none)."""
        return 0


class Evaluate(Act):
    """Pageable host buffers through gsdf_hip_eval3 / eval2, below and above the small-call threshold."""

    def __init__(self, name, dim=3):
        self.name, self.dim = name, dim

    def want(self, t, rung):
        n = EVAL_SIZES[rung]
        return _cached((t.name, "eval", n), lambda: {"dist": oracle(t).Evaluate(t.points(n, 1)).tobytes()})

    def run(self, cx, rung):
        pos = cx.t.points(EVAL_SIZES[rung], 1)
        keep = pos.copy()
        dist = np.full(len(pos), np.nan, F)
        cx.sdf.Evaluate(pos, dist)
        assert pos.tobytes() == keep.tobytes()
        return Result({"dist": dist.tobytes()}, evals=len(pos))


class Pipelined(Act):
    """submit / wait with two calls in flight, waited for in the other order."""
    name = "submit_wait"
    sizes = ((1, 65), (257, 1), (4097, 513), (20001, 4097))

    def want(self, t, rung):
        return _cached((t.name, "pipe", rung), lambda: {"d%d" % k: oracle(t).Evaluate(t.points(n, 2 + k)).tobytes() for k, n in enumerate(self.sizes[rung])})

    def run(self, cx, rung):
        pos = [cx.t.points(n, 2 + k) for k, n in enumerate(self.sizes[rung])]
        dist = [np.full(len(p), np.nan, F) for p in pos]
        tickets = [cx.sdf.submit(p, d) for p, d in zip(pos, dist)]
        for k in (1, 0):
            cx.sdf.wait(tickets[k])
        return Result({"d%d" % k: d.tobytes() for k, d in enumerate(dist)}, evals=sum(len(p) for p in pos))


class EvaluateDev(Act):
    name = "evaluate_dev"

    def want(self, t, rung):
        n = EVAL_SIZES[rung]
        return _cached((t.name, "evaldev", n), lambda: {"dist": oracle(t).Evaluate(t.points(n, 4)).tobytes()})

    def run(self, cx, rung):
        import torch
        pos = cx.t.points(EVAL_SIZES[rung], 4)
        tp = torch.from_numpy(pos).cuda().contiguous()
        td = torch.full((len(pos),), float("nan"), device="cuda")
        torch.cuda.synchronize()
        cx.sdf.evaluate_dev(tp.data_ptr(), 12, td.data_ptr(), len(pos))
        torch.cuda.synchronize()
        return Result({"dist": td.cpu().numpy().tobytes()})


class Normals(Act):
    name = "normals"

    def want(self, t, rung):
        n = NORMAL_SIZES[rung]
        return _cached((t.name, "normals", n), lambda: {"nrm": oracle(t).normals_central_diff(t.points(n, 5), 1e-3).tobytes()})

    def run(self, cx, rung):
        return Result({"nrm": cx.sdf.normals(cx.t.points(NORMAL_SIZES[rung], 5), 1e-3).tobytes()})


class Octree(Act):
    """OctreeHIP in one of its forms. share_corners 0 evaluates the reference's points, so the oracle's evaluation count is the
    device's; 1 and 2 evaluate fewer (gsdf_hip.h: gsdf_mesh_opts.share_corners), a count that only the fresh handle gives."""
    family = "octree"

    def __init__(self, name, prune=True, share=0, records=False):
        self.name, self.prune, self.share, self.records = name, prune, share, records
        if records:
            self.family = "records"

    def fields(self):
        return ("n_tris", "pruned_leaves", "levels") + (("evals",) if self.share == 0 else ())

    def want(self, t, rung):
        r = oracle_mesh(t, "octree", LADDER[rung], self.prune)
        w = {"tris": r.sorted_bytes, "n_tris": ints(r.n_tris), "pruned_leaves": ints(r.pruned), "levels": ints(r.levels)}
        if self.share == 0:
            w["evals"] = ints(r.evals)
        return w

    def n_tris(self, t, rung):
        return oracle_mesh(t, "octree", LADDER[rung], self.prune).n_tris

    def kw(self, cx):
        return dict(prune=self.prune, share_corners=self.share, payload=cx.gpu.PAYLOAD_RECORDS if self.records else cx.gpu.PAYLOAD_TRIANGLES)

    def start(self, cx, rung):
        return cx.gpu.OctreeHIP.start(cx.sdf, cx.t.res(LADDER[rung]), **self.kw(cx))

    def finish(self, cx, m):
        extra = {}
        if self.records:
            kind, nrec, nbytes = m.payload()
            assert kind == cx.gpu.PAYLOAD_RECORDS and nrec == int(m.stats.cut_leaves), (kind, nrec, int(m.stats.cut_leaves))
            extra["records"] = ints(nrec, nbytes)
            m.march()
            m._adopt(m._mesh)   # (the statistics once more, after the march)
        return mesh_result(cx, m, self.fields(), extra)

    def run(self, cx, rung):
        return self.finish(cx, cx.gpu.OctreeHIP(cx.sdf, cx.t.res(LADDER[rung]), **self.kw(cx)))


class OctreeStart3(Act):
    """OctreeHIP.start three times at three different rungs, waited for in a permuted order."""
    name, family = "octree_start3", "octree"
    ORDER = (1, 2, 0)

    def __init__(self, form):
        self.form = form

    def rungs(self, rung):
        return (rung, (rung + 2) % 4, (rung + 1) % 4)

    def want(self, t, rung):
        return {"%d.%s" % (k, f): v for k, r in enumerate(self.rungs(rung)) for f, v in self.form.want(t, r).items()}

    def n_tris(self, t, rung):
        return max(self.form.n_tris(t, r) for r in self.rungs(rung))

    def run(self, cx, rung):
        pend = [self.form.start(cx, r) for r in self.rungs(rung)]
        parts = {}
        for k in self.ORDER:
            parts[k] = self.form.finish(cx, pend[k].wait())
        out = Result()
        for k in sorted(parts):
            out.canon.update({"%d.%s" % (k, f): v for f, v in parts[k].canon.items()})
            out.more.update({"%d.%s" % (k, f): v for f, v in parts[k].more.items()})
            out.live += parts[k].live
        return out


class Flat(Act):
    name, family = "flat", "flat"

    def want(self, t, rung):
        r = oracle_mesh(t, "flat", LADDER[rung])
        return {"tris": r.sorted_bytes, "n_tris": ints(r.n_tris), "evals": ints(r.evals), "leaf_cubes": ints(r.grid[0] * r.grid[1] * r.grid[2])}

    def n_tris(self, t, rung):
        return oracle_mesh(t, "flat", LADDER[rung]).n_tris

    def run(self, cx, rung):
        return mesh_result(cx, cx.gpu.FlatHIP(cx.sdf, cx.t.res(LADDER[rung])), ("n_tris", "evals", "leaf_cubes"))


class DualContour(Act):
    """Plain or chiseled. The device skips blocks of cells that the oracle sweeps: its evaluation count is the fresh handle's."""
    family = "dc"

    def __init__(self, name, chiseled):
        self.name, self.chiseled = name, chiseled

    def div(self, rung):
        return DC_LADDER[rung // 2]

    def want(self, t, rung):
        r = oracle_mesh(t, "dc", self.div(rung), self.chiseled)
        return {"tris": r.sorted_bytes, "n_tris": ints(r.n_tris), "levels": ints(r.levels)}

    def n_tris(self, t, rung):
        return oracle_mesh(t, "dc", self.div(rung), self.chiseled).n_tris

    def run(self, cx, rung):
        return mesh_result(cx, cx.gpu.DualContourHIP(cx.sdf, cx.t.res(self.div(rung)), chiseled=self.chiseled), ("n_tris", "levels"))


class DualContourIndexed(DualContour):
    """IndexedHIP.dual_contour: verts[idx] is the oracle's triangle list in the oracle's order (tests/test_gpu_dc_indexed.py)."""
    family = "dcix"

    def want(self, t, rung):
        r = oracle_mesh(t, "dc", self.div(rung), False)
        return {"soup": np.ascontiguousarray(r.tris, F).tobytes(), "n_tris": ints(r.n_tris), "levels": ints(r.levels)}

    def run(self, cx, rung):
        ix = cx.gpu.IndexedHIP.dual_contour(cx.sdf, cx.t.res(self.div(rung)))
        v, i, k = ix.read()
        st = ix.mesh_stats
        canon = {"soup": np.ascontiguousarray(v[i.reshape(-1)]).tobytes(), "n_tris": ints(ix.n_tris), "levels": ints(st.levels)}
        more = {**read_indexed(ix), "stats": ints(ix.n_verts, st.n_tris, st.evals, st.leaf_cubes, st.active_leaves)}
        return Result(canon, more, [Live(ix, read_indexed)])


class Minecraft(Act):
    name, family = "minecraft", "mc"

    def div(self, rung):
        return MC_LADDER[rung // 2]

    def want(self, t, rung):
        r = oracle_mesh(t, "mc", self.div(rung))
        return {"tris": r.sorted_bytes, "n_tris": ints(r.n_tris), "evals": ints(r.evals), "levels": ints(r.levels)}

    def n_tris(self, t, rung):
        return oracle_mesh(t, "mc", self.div(rung)).n_tris

    def run(self, cx, rung):
        return mesh_result(cx, cx.gpu.MinecraftHIP(cx.sdf, cx.t.res(self.div(rung))), ("n_tris", "evals", "levels"))


class View(Act):
    name, oracle_backed = "render_view", False

    def run(self, cx, rung):
        rgba, depth, evals = cx.sdf.render_view(64, 48, yaw=0.4 * rung, pitch=0.2 * (rung - 1), aa=1 + rung % 2)
        return Result(more={"rgba": rgba.tobytes(), "depth": depth.tobytes(), "evals": evals.tobytes()})


class Slices(Act):
    name, oracle_backed = "slices", False

    def run(self, cx, rung):
        t = cx.t
        z = (t.bb[2] + (t.bb[5] - t.bb[2]) * np.array([0.23, 0.5, 0.81], F)).astype(F)
        c = cx.gpu.ContourHIP.slices(cx.sdf, res_for(t.bb, SLICE_LADDER[rung]), z)
        read = read_contour(cx.gpu)
        return Result(more=read(c), live=[Live(c, read)])


def corner_rays(t, n, seed):
    """n rays from the corners of the bounds toward interior points (tests/test_gpu_ray.py: corner_rays)."""
    rng = np.random.default_rng([seed, 77])
    corners = np.array([[t.bb[3 * ((k >> a) & 1) + a] for a in range(3)] for k in range(8)], F)
    o = corners[rng.integers(0, 8, n)]
    target = (t.bb[:3] + rng.random((n, 3), F) * (t.bb[3:] - t.bb[:3])).astype(F)
    return o, (target - o).astype(F)


class Rays(Act):
    name, oracle_backed = "raycast", False

    def run(self, cx, rung):
        o, r = corner_rays(cx.t, 65, rung)
        res = cx.t.res(LADDER[1])
        t, d, s, n, st = cx.sdf.raycast(o, r, tmax=F(2), tol=F(res / F(1024)), max_steps=96, refine=8, thin=F(0.5))
        return Result(more={"t": t.tobytes(), "d": d.tobytes(), "status": s.tobytes(), "steps": n.tobytes(), "stats": st.result_bytes()}, evals=int(st.evals))


class FixedNormals(Act):
    name, oracle_backed = "ix_normals", False

    def run(self, cx, rung):
        return Result(more={"nrm": cx.fixed.normals(cx.sdf, F(cx.t.res(LADDER[1]) / F(2 + rung))).tobytes()})


def project_opts(t, rung):
    res = t.res(LADDER[1])
    return dict(step=F(res / F(4)), tol=F(res / F(1024)), max_move=F(F(4) * res), max_iters=2 + 2 * rung)


class Project(Act):
    name, oracle_backed = "project", False

    def run(self, cx, rung):
        px, st = cx.fixed.project(cx.sdf, **project_opts(cx.t, rung))
        return Result(more={**read_projected(px), "stats": st.result_bytes()}, live=[Live(px, read_projected)], evals=int(st.evals))


class Deviation(Act):
    name, oracle_backed = "deviation", False

    def run(self, cx, rung):
        st = cx.fixed.deviation(cx.sdf, F(cx.t.res(LADDER[1]) / F(1 << (2 * rung))))
        return Result(more={"stats": st.result_bytes()}, evals=int(st.evals))


class Thickness(Act):
    name, oracle_backed = "thickness", False

    def run(self, cx, rung):
        res = cx.t.res(LADDER[1])
        th, s, st = cx.fixed.thickness(cx.sdf, step=F(res / F(4)), t0=F(res / F(4)), tmax=F(F(16 * (1 + rung)) * res), tol=F(res / F(1024)), max_steps=128, refine=8,
                                       thin=F(F(2) * res))
        return Result(more={"th": th.tobytes(), "status": s.tobytes(), "stats": st.result_bytes()}, evals=int(st.evals))


# ---- the 2-D handle ----
class Image(Act):
    name, dim, oracle_backed = "render_image", 2, False

    def run(self, cx, rung):
        dist, rgba = cx.sdf.render_image(*IMAGE_SIZES[rung])
        return Result(more={"dist": dist.tobytes(), "rgba": rgba.tobytes()})


class Picture(Act):
    name, dim, oracle_backed = "render_picture", 2, False

    def run(self, cx, rung):
        w, h = IMAGE_SIZES[rung]
        conv = (None, cx.gpu.color_default(), cx.gpu.color_gradient(0.25), None)[rung]
        rgba, dist = cx.sdf.render_picture(w, h, conv)
        return Result(more={"dist": dist.tobytes(), "rgba": rgba.tobytes()})


class Outline(Act):
    name, dim, oracle_backed = "outline", 2, False

    def run(self, cx, rung):
        c = cx.gpu.ContourHIP.outline(cx.sdf, res_for(cx.t.bb, SLICE_LADDER[rung]))
        read = read_contour(cx.gpu)
        return Result(more=read(c), live=[Live(c, read)])


# ---- error acts: the documented code, and nothing changed ----
class Refused(Act):
    """A call that must fail with `code` (and `text` in its message) and leave the handle's evaluation count where it was."""
    error = True

    def __init__(self, name, code, call, text="", dim=3):
        self.name, self.code, self.call, self.text, self.dim = name, code, call, text, dim

    def want(self, t, rung):
        return {"code": ints(self.code)}

    def run(self, cx, rung):
        e0 = cx.sdf.Evaluations()
        with pytest.raises(cx.gpu.HipError) as e:
            self.call(cx, rung)
        assert self.text in e.value.msg, (self.name, e.value.msg)
        assert cx.sdf.Evaluations() == e0, (self.name, "a refused call counted evaluations")
        return Result({"code": ints(e.value.code)})


class StaleTicket(Act):
    """wait() on a ticket that has been waited for: refused; the call it belonged to is counted once."""
    name, error = "stale_ticket", True
    sizes = (1, 257, 4097, 513)

    def want(self, t, rung):
        n = self.sizes[rung]
        return {"code": ints(BAD_ARGUMENT), **_cached((t.name, "stale", n), lambda: {"dist": oracle(t).Evaluate(t.points(n, 6)).tobytes()})}

    def run(self, cx, rung):
        pos = cx.t.points(self.sizes[rung], 6)
        dist = np.full(len(pos), np.nan, F)
        ticket = cx.sdf.submit(pos, dist)
        cx.sdf.wait(ticket)
        e0 = cx.sdf.Evaluations()
        with pytest.raises(cx.gpu.HipError) as e:
            cx.sdf.wait(ticket)
        assert cx.sdf.Evaluations() == e0
        return Result({"code": ints(e.value.code), "dist": dist.tobytes()}, evals=len(pos))


class WhileInFlight(Act):
    """FlatHIP, DualContourHIP or MinecraftHIP while an octree job of the handle is in flight: GSDF_ERR_BAD_ARGUMENT with the
    documented text; the job is then waited for and is the oracle's mesh."""
    error, family = True, "octree"

    def __init__(self, name, call, form):
        self.name, self.call, self.form = name, call, form

    def want(self, t, rung):
        return {"code": ints(BAD_ARGUMENT), **self.form.want(t, rung)}

    def n_tris(self, t, rung):
        return self.form.n_tris(t, rung)

    def run(self, cx, rung):
        pend = self.form.start(cx, rung)
        try:
            with pytest.raises(cx.gpu.HipError) as e:
                self.call(cx, rung)
            assert IN_FLIGHT in e.value.msg, e.value.msg
        finally:
            m = pend.wait()
        out = self.form.finish(cx, m)
        out.canon["code"] = ints(e.value.code)
        return out


def _table():
    default = Octree("octree")
    acts = [Evaluate("evaluate"), Pipelined(), EvaluateDev(), Normals(),
            default, Octree("octree_noprune", prune=False), Octree("octree_share1", share=1), Octree("octree_share2", share=2),
            Octree("octree_records_march", records=True), OctreeStart3(default),
            Flat(), DualContour("dualcontour", False), DualContour("dualcontour_chiseled", True), DualContourIndexed("dualcontour_indexed", False), Minecraft(),
            View(), Slices(), Rays(), FixedNormals(), Project(), Deviation(), Thickness(),
            Evaluate("evaluate2", dim=2), Image(), Picture(), Outline()]
    g = lambda cx: cx.gpu
    errors = [Refused("res_zero", RESOLUTION, lambda cx, r: (g(cx).OctreeHIP, g(cx).FlatHIP, g(cx).DualContourHIP, g(cx).MinecraftHIP)[r](cx.sdf, F(0)), "invalid renderer cube resolution"),
              Refused("res_too_coarse", RESOLUTION, lambda cx, r: (g(cx).OctreeHIP, g(cx).MinecraftHIP)[r % 2](cx.sdf, F(100 * cx.t.diag)), "not fine enough"),
              Refused("minecraft_10_levels", RESOLUTION, lambda cx, r: g(cx).MinecraftHIP(cx.sdf, cx.t.res(600)), "more than 9 octree levels"),
              Refused("image_of_3d", DIMENSION, lambda cx, r: cx.sdf.render_image(8 + r, 8)),
              StaleTicket(),
              WhileInFlight("flat_while_in_flight", lambda cx, r: g(cx).FlatHIP(cx.sdf, cx.t.res(LADDER[0])), default),
              WhileInFlight("dualcontour_while_in_flight", lambda cx, r: g(cx).DualContourHIP(cx.sdf, cx.t.res(DC_LADDER[0])), default),
              WhileInFlight("minecraft_while_in_flight", lambda cx, r: g(cx).MinecraftHIP(cx.sdf, cx.t.res(MC_LADDER[0])), default),
              Refused("octree_of_2d", DIMENSION, lambda cx, r: (g(cx).OctreeHIP, g(cx).FlatHIP, g(cx).DualContourHIP, g(cx).MinecraftHIP)[r](cx.sdf, F(0.1)), "2D", dim=2),
              Refused("outline_too_fine", BAD_ARGUMENT, lambda cx, r: g(cx).ContourHIP.outline(cx.sdf, F(1e-30)), dim=2)]
    return acts + errors


ACTS = _table()
BY_NAME = {a.name: a for a in ACTS}
assert len(BY_NAME) == len(ACTS)
ACTS3 = [a for a in ACTS if a.dim == 3]
ACTS2 = [a for a in ACTS if a.dim == 2]
MESHERS = ("octree", "records", "flat", "dc", "dcix", "mc")


def pair_rungs(ia, ib, variant):
    """The rungs of the ordered pair (act number ia, then ib): variant 0 small -> large, variant 1 large -> small, so that every
    ordered pair of mesher families sees both; which small and which large rung turns with the pair."""
    small, large = (ia + ib) % 2, 2 + ((ia + 2 * ib) // 2) % 2
    return (small, large) if variant == 0 else (large, small)


# ---------------- the code's own sizing rule ----------------
def first_guess(last):
    """Triangles (cut-leaf records) the output buffer of a mesh starts with, from the count the handle's previous mesh left
    (abi_mesh.hip: prepare_outputs and gsdf_hip_mesh_flat; a fresh handle starts with 2^20)."""
    return last + last // 16 + 1024 if last else 1 << 20


def takes_rerun(n_prev, n_next):
    """Whether the mesh of n_next triangles after one of n_prev overflows its first buffer and is repeated at the exact size. Necessary,
    not sufficient: the pool of idle buffers hands out the smallest one that is large ENOUGH, which may be larger than asked for."""
    return first_guess(n_prev) < n_next


# Climbs: acts up the ladder on one handle in a FRESH process, every result object kept alive. The pool of idle buffers is empty at
# the start and only ever receives the first-guess buffers that overflowed, each smaller than the next step's guess: every step after
# the first gets a buffer of exactly first_guess(previous count) and, where takes_rerun() says so, is certain to overflow it.
CLIMBS = {"octree_first": (("octree", 0), ("octree", 1), ("flat", 2), ("octree", 3)),        # octree -> octree, octree -> flat, flat -> octree
          "flat_first": (("flat", 0), ("flat", 1), ("octree_share2", 2), ("flat", 3)),       # flat -> flat, flat -> octree, octree -> flat
          # records -> records (last_recs: cut leaves, between a fifth of the triangles and all of them -- two rungs apart the step is certain)
          "records": (("octree_records_march", 0), ("octree_records_march", 2)),
          "records_high": (("octree_records_march", 1), ("octree_records_march", 3))}


DC_FLOOR_CUBES = 1 << 20  # abi_mesh.hip, dc_mesh: the first capacity of the cube lists is never below this (unless the lattice has fewer cells)


# ---------------- CPU tests of the table ----------------
def _oracle_backed(dim):
    return [a for a in ACTS if a.dim == dim and a.oracle_backed]


@pytest.mark.parametrize("name", TREES3 + (TREE2,))
def test_every_oracle_backed_expectation_exists(name):
    t = tree(name)
    seen = 0
    for a in _oracle_backed(t.dim):
        for rung in range(4):
            w = a.want(t, rung)
            assert w and all(isinstance(v, bytes) for v in w.values()), (a.name, rung)
            assert a.error or all(len(v) > 0 for v in w.values()), (a.name, rung)
            seen += 1
    assert seen == 4 * len(_oracle_backed(t.dim)) and seen >= (4 if t.dim == 2 else 60)
    # the acts without an oracle say so: exactly these, whose CPU twins are held to the device in their own test files
    assert sorted(a.name for a in ACTS if not a.oracle_backed) == sorted(["render_view", "slices", "raycast", "ix_normals", "project", "deviation", "thickness",
                                                                         "render_image", "render_picture", "outline"])


def test_ladder_counts_are_the_stated_ones():
    for name in TREES3:
        t = tree(name)
        octree = [oracle_mesh(t, "octree", d, True) for d in LADDER]
        assert tuple(r.n_tris for r in octree) == COUNTS[name]
        assert tuple(oracle_mesh(t, "flat", d).n_tris for d in LADDER) == COUNTS[name]            # flat counts equal the octree's
        assert tuple(oracle_mesh(t, "octree", d, False).n_tris for d in LADDER) == COUNTS[name]   # pruning drops no surface
    assert oracle_mesh(tree("bolt"), "octree", 12, True).levels == 4
    assert tuple(oracle_mesh(tree("bolt"), "dc", d, False).n_tris for d in DC_LADDER) == DC_COUNTS_BOLT


def test_upward_steps_take_the_rerun_path():
    """Every upward step of the ladder overflows the buffer that the smaller mesh's hint asks for -- octree -> octree, octree -> flat,
    flat -> octree (the two share last_tris), records -> records (last_recs: cut leaves) -- and no downward step does. Dual
    contouring sizes its lists from last_dc_cubes with a floor of 2^20 cubes: no mesh of this table comes near it, so a dual
    contouring mesh after another never repeats its origin pass here (tests/test_gpu_mesh.py::test_dualcontour_lists_regrow drives
    that with a full-size part)."""
    for name in TREES3:
        n = COUNTS[name]
        for i in range(4):
            for j in range(4):
                assert takes_rerun(n[i], n[j]) == (j > i), (name, i, j)     # octree / flat in any combination: one hint, one rule
        # records: a cut leaf has one to five triangles, so tris / 5 <= cut leaves <= tris. From a small rung (0, 1) to a large one
        # (2, 3), the steps the pair matrix takes, even the fewest records of the larger mesh overflow the guess after the most of the smaller
        for i in (0, 1):
            for j in (2, 3):
                assert first_guess(n[i]) < -(-n[j] // 5), (name, i, j)
        assert not takes_rerun(0, n[3])                                       # a fresh handle's first buffer holds every mesh of the table
        for d in DC_LADDER:
            assert 8 ** (oracle_mesh(tree(name), "dc", d, False).levels - 1) < DC_FLOOR_CUBES   # (the whole lattice has fewer cells than the floor)
    # the pair matrix reaches an upward and a downward step for every ordered pair of mesher families
    fam = {}
    for k, a in enumerate(ACTS3):
        if a.family in MESHERS:
            fam.setdefault(a.family, k)
    for fa, ia in fam.items():
        for fb, ib in fam.items():
            (a0, b0), (a1, b1) = pair_rungs(ia, ib, 0), pair_rungs(ia, ib, 1)
            assert a0 < b0 and a1 > b1, (fa, fb)
    # every step of every climb, from the oracle's counts (records: the fewest cut leaves of the larger mesh against the most of the smaller)
    for kind, steps in CLIMBS.items():
        for name in TREES3:
            n = [BY_NAME[a].n_tris(tree(name), rung) for a, rung in steps]
            for prev, nxt in zip(n, n[1:]):
                assert first_guess(prev) < (-(-nxt // 5) if kind.startswith("records") else nxt), (kind, name, prev, nxt)
    i_oct, i_flat, i_rec = fam["octree"], fam["flat"], fam["records"]
    for ia, ib in ((i_oct, i_oct), (i_oct, i_flat), (i_flat, i_oct), (i_rec, i_rec)):
        ra, rb = pair_rungs(ia, ib, 0)
        assert ra in (0, 1) and rb in (2, 3)
        for name in TREES3:
            assert takes_rerun(COUNTS[name][ra], COUNTS[name][rb])


def test_no_mesh_exceeds_the_size_bound():
    biggest = 0
    for name in TREES3:
        for a in ACTS3:
            for rung in range(4):
                biggest = max(biggest, a.n_tris(tree(name), rung))
    assert 0 < biggest <= MAX_TRIS, biggest


def test_comparators_are_sensitive():
    """check() fails on the expectation of another rung (or, where an act has two rungs only, of the other one) and on the same bytes
    with one bit flipped, label by label; it passes on a copy."""
    for name in TREES3 + (TREE2,):
        t = tree(name)
        for a in _oracle_backed(t.dim):
            if isinstance(a, Refused):
                w = a.want(t, 0)
                with pytest.raises(AssertionError):
                    check({"code": ints(a.code + 1)}, w, a.name)
                continue
            w0, w3 = a.want(t, 0), a.want(t, 3)
            check(dict(w0), w0, a.name)
            with pytest.raises(AssertionError):
                check(w3, w0, a.name)
            for label, v in w0.items():
                for pos in {0, len(v) // 2, len(v) - 1}:
                    flipped = bytearray(v)
                    flipped[pos] ^= 1 << (pos % 8)
                    with pytest.raises(AssertionError):
                        check({**w0, label: bytes(flipped)}, w0, (a.name, label))
            with pytest.raises(AssertionError):
                check({k: v for k, v in list(w0.items())[1:]}, w0, a.name)       # a missing label
            with pytest.raises(AssertionError):
                check({**w0, "extra": b""}, w0, a.name)                          # one too many
    # sorted by bit pattern: the order of emission does not matter, a changed coordinate does
    tris = oracle_mesh(tree("bolt"), "octree", 12, True).tris
    assert tri_bytes(tris[::-1]) == tri_bytes(tris) and tri_bytes(-tris) != tri_bytes(tris)
