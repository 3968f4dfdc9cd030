"""The refusals of the contour unit (gsdf_amd/csrc/abi_contour.hip), straight at the C ABI: a table of bad calls of every entry point --
gsdf_hip_contour2, gsdf_hip_slice3, gsdf_hip_contour_create, _simplify, _measures, _sections, _hatch, _hatch_skin, gsdf_hip_hatch_read,
gsdf_hip_hatch_read_skin, gsdf_hip_contour_offset, _distance -- whose (return code, gsdf_hip_last_error text) must equal
tests/golden/contour_refusals.json row by row. One row per refusal with GSDF_ERR_BAD_ARGUMENT, GSDF_ERR_EMPTY_BUFFERS or
GSDF_ERR_DIMENSION that can be reached without exhausting memory or 2^31 elements (not reached: "out of memory" of a handle's `new`,
and "the program's bounds are not finite", which no program the builder makes has); rows with two faults at once pin the ORDER of the
checks. gsdf_hip_hatch_read_skin has two checks that cannot fail together, measures and sections have one each.

The fixture holds names, codes and texts only and is recorded from the build of the commit BEFORE a change to that unit, never from
the code under test:   python tests/test_gpu_contour_refusals.py --record /path/to/that/libgsdfhip.so   (once, on the GPU).
After the table one valid hatch on the same handles equals tests/hatchref.py byte for byte: a refused call leaves nothing behind."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURE = os.path.join(ROOT, "tests", "golden", "contour_refusals.json")
F = np.float32
NAN, INF = float("nan"), float("inf")


class Scene:
    """The smallest inputs that reach every row: the unit square (one layer), the same twice (two layers), a square of side 3e38, a
    handle without loops (the sphere sliced above itself), a plain hatch of the square; a 2-D circle and a 3-D sphere program."""

    def __init__(self, hip):
        import contoursimpref as S
        from scaffold.builder import Builder
        self.hip, self.L = hip, hip.lib()
        sq = np.array([(0, 0), (1, 0), (1, 1), (0, 1)], F)
        self.sq_xy, self.sq_start = sq.copy(), np.array([0, 4], np.uint32)
        self.ref = S.pack([sq])
        up = lambda r: hip.ContourHIP.from_arrays(r.xy, r.loop_start, r.loop_layer, r.n_layers, r.keys)  # noqa: E731
        self.square = up(self.ref)
        self.stack = up(S.pack([sq, sq], [0, 1], 2))
        self.huge = up(S.pack([sq * F(3e38)]))
        b = Builder()
        self.p2, ball = hip.SDF2HIP(b.NewCircle(1.0)), b.NewSphere(1.0)
        self.p3 = hip.SDF3HIP(ball)
        self.res = float(F(float(ball.Diagonal()) / 16))
        self.empty = hip.ContourHIP.slices(self.p3, self.res, [2.0])
        assert (self.empty.n_verts, self.empty.n_loops, self.empty.n_layers) == (0, 0, 1)
        self.plain = self.square.hatch_dirs(0.25, [(1.0, 0.0)])


def hatch_opts(hip, spacing=0.25, offset=0.0, dirs=((1.0, 0.0),), n_dirs=None, dry=0):
    o = hip.HatchOpts(spacing, offset, len(dirs) if n_dirs is None else n_dirs, dry)
    for k, (dx, dy) in enumerate(dirs):
        o.dir[k][0], o.dir[k][1] = dx, dy
    return C.byref(o)


def offset_opts(hip, res=0.25, insets=(0.1,), n_insets=None, dry=0, reserved=0):
    o = hip.OffsetOpts(res, len(insets) if n_insets is None else n_insets, dry, reserved, 0)
    for k, v in enumerate(insets):
        o.inset[k] = v
    return C.byref(o)


def table(sc):
    """[(name, call)]: call() makes the bad call and returns its code."""
    hip, L = sc.hip, sc.L
    p2, p3, sq, st2, empty, huge = sc.p2._h, sc.p3._h, sc.square._h, sc.stack._h, sc.empty._h, sc.huge._h
    out = lambda: C.byref(C.c_void_p())  # noqa: E731
    z = np.array([0.0], F)
    rows = []
    add = lambda name, call: rows.append((name, call))  # noqa: E731

    # ---- gsdf_hip_contour2, gsdf_hip_slice3
    add("contour2: null program", lambda: L.gsdf_hip_contour2(None, sc.res, None, out()))
    add("contour2: null out", lambda: L.gsdf_hip_contour2(p2, sc.res, None, None))
    add("contour2: 3-D program", lambda: L.gsdf_hip_contour2(p3, sc.res, None, out()))
    add("contour2: res 0", lambda: L.gsdf_hip_contour2(p2, 0.0, None, out()))
    add("contour2: res NaN", lambda: L.gsdf_hip_contour2(p2, NAN, None, out()))
    add("contour2: res too fine", lambda: L.gsdf_hip_contour2(p2, 1e-9, None, out()))
    add("contour2: 3-D program + res 0", lambda: L.gsdf_hip_contour2(p3, 0.0, None, out()))
    add("contour2: null out + res NaN", lambda: L.gsdf_hip_contour2(p2, NAN, None, None))
    add("contour2: res -1 + too fine", lambda: L.gsdf_hip_contour2(p2, -1e-9, None, out()))
    add("slice3: null program", lambda: L.gsdf_hip_slice3(None, sc.res, z.ctypes.data, 1, None, out()))
    add("slice3: 2-D program", lambda: L.gsdf_hip_slice3(p2, sc.res, z.ctypes.data, 1, None, out()))
    add("slice3: null z", lambda: L.gsdf_hip_slice3(p3, sc.res, None, 1, None, out()))
    add("slice3: no z", lambda: L.gsdf_hip_slice3(p3, sc.res, z.ctypes.data, 0, None, out()))
    add("slice3: res inf", lambda: L.gsdf_hip_slice3(p3, INF, z.ctypes.data, 1, None, out()))
    add("slice3: res too fine", lambda: L.gsdf_hip_slice3(p3, 1e-9, z.ctypes.data, 1, None, out()))
    add("slice3: 2-D program + null z", lambda: L.gsdf_hip_slice3(p2, sc.res, None, 1, None, out()))
    add("slice3: no z + res 0", lambda: L.gsdf_hip_slice3(p3, 0.0, z.ctypes.data, 0, None, out()))

    # ---- gsdf_hip_contour_create
    def create(xy=sc.sq_xy, n_verts=4, start=(0, 4), n_loops=1, layer=None, n_layers=1, null_out=False):
        xy = None if xy is None else np.ascontiguousarray(xy, F)
        start = None if start is None else np.array(start, np.uint32)
        layer = None if layer is None else np.array(layer, np.uint32)
        ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
        return L.gsdf_hip_contour_create(ptr(xy), n_verts, ptr(start), n_loops, ptr(layer), n_layers, None, None if null_out else out())
    nan_xy = sc.sq_xy.copy()
    nan_xy[2, 1] = NAN
    two = np.concatenate([sc.sq_xy, sc.sq_xy + F(2)])
    add("create: null out", lambda: create(null_out=True))
    add("create: no loops", lambda: create(n_loops=0))
    add("create: no vertices", lambda: create(n_verts=0))
    add("create: null xy", lambda: create(xy=None))
    add("create: null loop_start", lambda: create(start=None))
    add("create: no layers", lambda: create(n_layers=0))
    add("create: loop 0 starts at 1", lambda: create(start=(1, 4)))
    add("create: a loop of 2 vertices", lambda: create(xy=two, n_verts=8, start=(0, 6, 8), n_loops=2))
    add("create: the last loop ends early", lambda: create(start=(0, 3)))
    add("create: a layer the handle does not have", lambda: create(layer=(1,)))
    add("create: layers out of order", lambda: create(xy=two, n_verts=8, start=(0, 4, 8), n_loops=2, layer=(1, 0), n_layers=2))
    add("create: a NaN vertex", lambda: create(xy=nan_xy))
    add("create: loop 0 starts at 1 + a NaN vertex", lambda: create(xy=nan_xy, start=(1, 4)))
    add("create: no layers + a loop of 2 vertices", lambda: create(xy=two, n_verts=8, start=(0, 6, 8), n_loops=2, n_layers=0))
    add("create: no vertices + null xy", lambda: create(xy=None, n_verts=0))
    add("create: a layer the handle does not have + the last loop ends early", lambda: create(start=(0, 3), layer=(1,)))

    # ---- gsdf_hip_contour_simplify, _measures, _sections
    def simplify(c=sq, tol=0.1, levels=0, passes=0, dry=0, null_opts=False, null_out=False):
        o = hip.ContourSimplifyOpts(tol, levels, passes, dry)
        return L.gsdf_hip_contour_simplify(c, None if null_opts else C.byref(o), None if null_out else out(), None)
    add("simplify: null contour", lambda: simplify(c=None))
    add("simplify: null options", lambda: simplify(null_opts=True))
    add("simplify: tol -1", lambda: simplify(tol=-1.0))
    add("simplify: tol NaN", lambda: simplify(tol=NAN))
    add("simplify: levels 17", lambda: simplify(levels=17))
    add("simplify: passes 9", lambda: simplify(passes=9))
    add("simplify: null out, not dry", lambda: simplify(null_out=True))
    add("simplify: tol -1 + levels 17", lambda: simplify(tol=-1.0, levels=17))
    add("simplify: passes 9 + null out, not dry", lambda: simplify(passes=9, null_out=True))
    add("simplify: levels 17 + passes 9", lambda: simplify(levels=17, passes=9))
    add("measures: null contour", lambda: L.gsdf_hip_contour_measures(None, None, None))
    add("sections: null contour", lambda: L.gsdf_hip_contour_sections(None, None, None))

    # ---- gsdf_hip_contour_hatch, _hatch_skin: the options' checks are shared, every one is asked of both
    def hatch(c=sq, null_opts=False, null_out=False, **kw):
        return L.gsdf_hip_contour_hatch(c, None if null_opts else hatch_opts(hip, **kw), None if null_out else out(), None)

    def skin(c=st2, below=1, above=1, null_opts=False, null_skin=False, null_out=False, **kw):
        k = hip.SkinOpts(below, above)
        return L.gsdf_hip_contour_hatch_skin(c, None if null_opts else hatch_opts(hip, **kw), None if null_skin else C.byref(k), None if null_out else out(), None)
    for name, fn in (("hatch", hatch), ("skin", skin)):
        add(name + ": null contour", lambda fn=fn: fn(c=None))
        add(name + ": null options", lambda fn=fn: fn(null_opts=True))
        add(name + ": spacing 0", lambda fn=fn: fn(spacing=0.0))
        add(name + ": spacing NaN", lambda fn=fn: fn(spacing=NAN))
        add(name + ": offset inf", lambda fn=fn: fn(offset=INF))
        add(name + ": n_dirs 0", lambda fn=fn: fn(n_dirs=0))
        add(name + ": n_dirs 5", lambda fn=fn: fn(n_dirs=5))
        add(name + ": dir 0 is (0, 0)", lambda fn=fn: fn(dirs=((0.0, 0.0),)))
        add(name + ": dir 1 beyond 1", lambda fn=fn: fn(dirs=((1.0, 0.0), (0.5, 2.0))))
        add(name + ": dir 0 NaN", lambda fn=fn: fn(dirs=((NAN, 1.0),)))
        add(name + ": null out, not dry", lambda fn=fn: fn(null_out=True))
        add(name + ": spacing too small for the loops", lambda fn=fn: fn(spacing=1e-9))
        add(name + ": spacing too small for a handle without loops", lambda fn=fn: fn(c=empty, spacing=1e-9, offset=1.0))
        add(name + ": spacing NaN + n_dirs 0", lambda fn=fn: fn(spacing=NAN, n_dirs=0))
        add(name + ": offset inf + null out, not dry", lambda fn=fn: fn(offset=INF, null_out=True))
        add(name + ": dir 0 is (0, 0) + spacing too small for the loops", lambda fn=fn: fn(dirs=((0.0, 0.0),), spacing=1e-9))
    add("skin: null skin options", lambda: skin(null_skin=True))
    add("skin: below 9", lambda: skin(below=9))
    add("skin: above 9", lambda: skin(above=9))
    add("skin: spacing NaN + below 9", lambda: skin(spacing=NAN, below=9))
    add("skin: null out, not dry + above 9", lambda: skin(null_out=True, above=9))
    add("skin: below 9 + spacing too small for a handle without loops", lambda: skin(c=empty, below=9, spacing=1e-9, offset=1.0))
    add("skin: above 9 + spacing too small for the loops", lambda: skin(above=9, spacing=1e-9))

    # ---- gsdf_hip_hatch_read, gsdf_hip_hatch_read_skin
    add("hatch_read: null hatch", lambda: L.gsdf_hip_hatch_read(None, None, None, None, None))
    add("hatch_read_skin: null hatch", lambda: L.gsdf_hip_hatch_read_skin(None, None, None))
    add("hatch_read_skin: a plain hatch", lambda: L.gsdf_hip_hatch_read_skin(sc.plain._h, None, None))

    # ---- gsdf_hip_contour_offset, _distance: the options' checks and the lattice's are shared, every one is asked of both
    def offset(c=sq, null_opts=False, null_out=False, **kw):
        return L.gsdf_hip_contour_offset(c, None if null_opts else offset_opts(hip, **kw), None if null_out else out(), None)
    d_out = np.zeros(64 * 64, F)   # (room for the lattice of the square at res 0.25, which no row here gets as far as filling)

    def distance(c=sq, layer=0, null_opts=False, null_out=False, **kw):
        return L.gsdf_hip_contour_distance(c, None if null_opts else offset_opts(hip, **kw), layer, None if null_out else d_out.ctypes.data, None)
    for name, fn in (("offset", offset), ("distance", distance)):
        add(name + ": null contour", lambda fn=fn: fn(c=None))
        add(name + ": null options", lambda fn=fn: fn(null_opts=True))
        add(name + ": res 0", lambda fn=fn: fn(res=0.0))
        add(name + ": res NaN", lambda fn=fn: fn(res=NAN))
        add(name + ": n_insets 0", lambda fn=fn: fn(n_insets=0))
        add(name + ": n_insets 9", lambda fn=fn: fn(n_insets=9))
        add(name + ": inset 1 inf", lambda fn=fn: fn(insets=(0.1, INF)))
        add(name + ": reserved 1", lambda fn=fn: fn(reserved=1))
        add(name + ": the grown bounds overflow", lambda fn=fn: fn(c=huge, insets=(-3e38,)))
        add(name + ": res too fine", lambda fn=fn: fn(res=1e-9))
        add(name + ": res too fine for 8 insets", lambda fn=fn: fn(res=5e-5, insets=(0.01,) * 8))
        add(name + ": res 0 + inset 0 NaN", lambda fn=fn: fn(res=0.0, insets=(NAN,)))
        add(name + ": n_insets 9 + the grown bounds overflow", lambda fn=fn: fn(c=huge, n_insets=9, insets=(-3e38,)))
        add(name + ": inset 0 NaN + reserved 1", lambda fn=fn: fn(insets=(NAN,), reserved=1))
    add("offset: null out, not dry", lambda: offset(null_out=True))
    add("offset: reserved 1 + null out, not dry", lambda: offset(reserved=1, null_out=True))
    add("offset: null out, not dry + res too fine", lambda: offset(null_out=True, res=1e-9))
    add("distance: null out", lambda: distance(null_out=True))
    add("distance: layer 1 of 1", lambda: distance(layer=1))
    add("distance: layer 2 of 2", lambda: distance(c=st2, layer=2))
    add("distance: res 0 + layer 1 of 1", lambda: distance(res=0.0, layer=1))
    add("distance: layer 1 of 1 + res too fine", lambda: distance(layer=1, res=1e-9))
    add("distance: null out + res 0", lambda: distance(null_out=True, res=0.0))
    assert len({n for n, _ in rows}) == len(rows)
    return rows


def run_table(sc):
    """{name: [code, text]} of every row, in table order."""
    got = {}
    for name, call in table(sc):
        rc = call()
        got[name] = [int(rc), sc.L.gsdf_hip_last_error().decode()]
    return got


@pytest.fixture(scope="module")
def refused(gpu):
    sc = Scene(gpu)
    return sc, run_table(sc)


@pytest.mark.gpu
def test_every_refusal_has_the_recorded_code_and_text(refused):
    _, got = refused
    want = json.load(open(FIXTURE))
    assert list(got) == list(want), sorted(set(got) ^ set(want))
    assert all(code != 0 for code, _ in got.values()), [n for n, (code, _) in got.items() if code == 0]
    wrong = [(n, got[n], want[n]) for n in want if got[n] != want[n]]
    assert not wrong, wrong
    assert len(want) >= 120 and {code for code, _ in want.values()} == {-1, -3, -7}, len(want)   # EMPTY_BUFFERS, BAD_ARGUMENT, DIMENSION


@pytest.mark.gpu
def test_a_hatch_after_the_refusals_is_the_twins(refused):
    """The handles every row above was refused on: one valid hatch of the square, byte for byte."""
    import hatchref as H
    sc, _ = refused
    dirs = H.directions((45.0, 135.0))
    want, got = H.hatch(sc.ref, 0.125, dirs, 0.0437), sc.square.hatch_dirs(0.125, dirs, 0.0437)
    assert got.n_segments == want.stats["n_segments"] > 8
    for f in ("seg", "line", "layer_start", "layers"):
        a, b = getattr(got, f), getattr(want, f)
        assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), f
    assert (got.stats.n_crossings, got.stats.n_lines, got.stats.length) == (want.stats["n_crossings"], want.stats["n_lines"], want.stats["length"])


if __name__ == "__main__":
    # --record LIB: the table against the library at LIB (the build of the commit before the change) -> the fixture
    assert len(sys.argv) == 3 and sys.argv[1] == "--record", "usage: test_gpu_contour_refusals.py --record /path/to/libgsdfhip.so"
    sys.path.insert(0, ROOT)
    from gsdf_amd import hip
    hip.LIB_PATH = os.path.abspath(sys.argv[2])
    hip.init(0)
    rec = run_table(Scene(hip))
    assert all(code != 0 for code, _ in rec.values()), [n for n, (code, _) in rec.items() if code == 0]
    with open(FIXTURE, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("recorded %d rows from %s" % (len(rec), hip.LIB_PATH))
