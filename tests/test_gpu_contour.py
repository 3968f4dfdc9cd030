"""Contours on the device (gsdf_hip_contour2 / gsdf_hip_slice3; gsdf_amd/csrc/kernels_contour.h) against the CPU twin of the
contract (tests/contourref.py) over the oracle: coordinates, keys, loop starts, loop layers and the integer statistics identical, as
bytes -- the 2-D corpus, the two saddles, interpreter and per-tree kernels, a lattice large enough for many workgroups, scan blocks and
thirteen ranking rounds, fields with NaN and infinite distances, stacks of slices with every chunking, run twice, the argument errors."""
import importlib.util
import math
import os

import numpy as np
import pytest

import contourref
import corpus
from oracle.oracle import OracleSDF
from scaffold.builder import Builder
from contourref import check_structure, res_for, saddle_shape
from tree_edit import clone, first

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
INT_STATS = ("nx", "ny", "n_layers", "n_verts", "n_loops", "border_inside", "nonfinite_nodes", "saddle_cells", "rank_rounds", "evals")


def _example():
    spec = importlib.util.spec_from_file_location("render_png", os.path.join(ROOT, "examples", "render_png.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def same(dev, ref, what):
    """The device handle against the twin: the integer statistics, then the four arrays as bytes."""
    st = dev.stats
    got = {k: int(getattr(st, k)) for k in INT_STATS}
    assert got == {k: int(ref.stats[k]) for k in INT_STATS}, (what, got, ref.stats)
    assert (dev.n_layers, dev.n_loops, dev.n_verts) == (ref.stats["n_layers"], ref.stats["n_loops"], ref.stats["n_verts"]), what
    for f in ("keys", "loop_start", "loop_layer", "xy"):
        a, b = getattr(dev, f), getattr(ref, f)
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, a.shape, b.shape)
        if a.tobytes() != b.tobytes():
            bad = np.flatnonzero((a.reshape(len(a), -1).view(np.uint32) != b.reshape(len(b), -1).view(np.uint32)).any(axis=1))
            raise AssertionError((what, f, len(bad), bad[:5].tolist(), a[bad[:3]].tolist(), b[bad[:3]].tolist()))
    assert st.ms_eval > 0 and st.ms_trace > 0 and abs(st.ms_device - st.ms_eval - st.ms_trace) < 1e-9


def same_handles(a, b, what):
    assert a.stats.result_bytes() == b.stats.result_bytes(), what
    for f in ("xy", "keys", "loop_start", "loop_layer"):
        assert getattr(a, f).tobytes() == getattr(b, f).tobytes(), (what, f)


def test_corpus_outlines_match_the_twin(gpu):
    _, shapes = corpus.shapes2d()
    sides, loops = set(), 0
    for name, s in shapes:
        sdf = gpu.SDF2HIP(s)
        res = res_for(sdf.Bounds(), 40)
        ref = contourref.of_oracle(s.tree(), res)
        dev = gpu.ContourHIP.outline(sdf, res)
        same(dev, ref, name)
        sides |= {ref.stats["nx"], ref.stats["ny"]}
        loops += dev.n_loops
        if dev.n_loops:
            assert dev.areas().sum() > 0, name
    assert loops > 60 and not any(n % 64 == 0 for n in sides), (loops, sorted(sides))


@pytest.mark.parametrize("like", [True, False])
def test_saddles_match_the_twin(gpu, like):
    s = saddle_shape(Builder(), like)
    ref = contourref.of_oracle(s.tree(), F(0.3))
    dev = gpu.ContourHIP.outline(gpu.SDF2HIP(s), F(0.3))
    assert ref.stats["saddle_cells"] == 1 and ref.layers[0].case_counts[5 if like else 10] == 1
    same(dev, ref, ("saddle", like))
    assert dev.n_loops == 2 and (dev.areas() > 0).all()


@pytest.mark.parametrize("scene", ["text", "thread"])
def test_interpreter_and_per_tree_kernels(gpu, scene):
    s = _example().scene(scene)
    interp, spec = gpu.SDF2HIP(s), gpu.SDF2HIP(s).specialize()
    res = res_for(interp.Bounds(), 150)
    ref = contourref.of_oracle(s.tree(), res)
    a, b = gpu.ContourHIP.outline(interp, res), gpu.ContourHIP.outline(spec, res)
    same(a, ref, (scene, "interpreter"))
    same(b, ref, (scene, "per-tree"))
    assert spec.info()["specialized"] and not interp.info()["specialized"]
    assert ref.stats["n_loops"] >= (7 if scene == "text" else 1)
    check_structure(ref)


def test_large_circle_crosses_blocks_and_needs_13_rounds(gpu):
    s = Builder().NewCircle(1.0)
    res = F(2.0 / 2048)
    ref = contourref.of_oracle(s.tree(), res)
    dev = gpu.ContourHIP.outline(gpu.SDF2HIP(s), res)
    st = dev.stats
    assert st.rank_rounds >= 13 and dev.n_loops == 1 and st.nx * st.ny > 4_000_000 and dev.n_verts > 16 * 256  # (vertices over many workgroups; 8 million edge slots over many scan blocks)
    same(dev, ref, "circle 2/2048")
    assert abs(dev.areas()[0] / math.pi - 1) < float(res) ** 2


def _nonfinite_trees():
    b = Builder()
    out = []
    for name, v in (("offset-inf", float("inf")), ("offset-minus-inf", float("-inf")), ("offset-nan", float("nan"))):
        t = clone(b.Offset2D(b.NewRectangle(1, 1), 0.1).tree())
        t.nodes[first(t, "OFFSET2D")].p[0] = v
        out.append((name, t))
    # NaN parameters that reach the distance through arithmetic rather than a min / max: a scale and a translation by NaN
    t = clone(b.Scale2D(b.NewRectangle(1, 1), 2.0).tree())
    t.nodes[first(t, "SCALE2D")].p[0] = float("nan")
    out.append(("scale-nan", t))
    t = clone(b.Translate2D(b.NewCircle(0.5), 0.25, 0.0).tree())
    t.nodes[first(t, "TRANSLATE2D")].p[0] = float("nan")
    out.append(("translate-nan", t))
    # a line whose ends coincide (0 / 0 in its projection) next to a circle; a scale by zero (positions times Inf)
    t = clone(b.Union2D(b.NewLine2D(0.2, 0.1, 1.0, 0.5, 0.2), b.NewCircle(0.3)).tree())
    n = t.nodes[first(t, "LINE2D")]
    n.p[2], n.p[3] = n.p[0], n.p[1]
    out.append(("line-of-length-zero", t))
    t = clone(b.Union2D(b.Scale2D(b.NewRectangle(1, 1), 2.0), b.Translate2D(b.NewCircle(0.5), 2, 0)).tree())
    t.nodes[first(t, "SCALE2D")].p[0] = 0.0
    out.append(("scale-zero", t))
    return out


def test_nan_and_inf_fields(gpu):
    """The call returns, the loops close, the counts and the bytes are the twin's. The oracle differs from the device where it meets
    NaN (tests/test_gpu_nan.py), so the twin runs over the device's own distances everywhere -- and over the oracle's too where the
    oracle has no NaN on the lattice."""
    seen = {"nonfinite": 0, "loops": 0, "oracle": 0}
    for name, t in _nonfinite_trees():
        for spec in (False, True):
            sdf = gpu.SDF2HIP(t)
            if spec:
                sdf.specialize()
            res = res_for(sdf.Bounds(), 40)
            dev = gpu.ContourHIP.outline(sdf, res)
            ref = contourref.contour(sdf.Evaluate, sdf.Bounds(), res)
            same(dev, ref, (name, spec))
            check_structure(ref)
            assert dev.loop_start[-1] == dev.n_verts and int(dev.stats.nonfinite_nodes) == ref.stats["nonfinite_nodes"]
            seen["nonfinite"] += ref.stats["nonfinite_nodes"]
            seen["loops"] += dev.n_loops
            o = OracleSDF(t)
            nx, ny, xs, ys = contourref.lattice(o.Bounds(), res)
            if not np.isnan(o.Evaluate(contourref.positions(xs, ys))).any():
                same(dev, contourref.contour(o.Evaluate, o.Bounds(), res), (name, spec, "oracle"))
                seen["oracle"] += 1
    assert seen["nonfinite"] > 0 and seen["loops"] > 0 and seen["oracle"] > 0, seen


@pytest.fixture(scope="module")
def stacks():
    """bolt and npt-flange at diag / 60, seven layers: (shape, res, z, twin), computed once."""
    out = {}
    for name in ("bolt", "npt-flange"):
        s = Builder().Scene(name)
        bb = s.Bounds()
        res = F(float(s.Diagonal()) / 60)
        z = contourref.layer_heights(bb, F(F(bb[5] - bb[2]) / F(7)))
        assert len(z) == 7
        out[name] = (s, res, z, contourref.of_oracle(s.tree(), res, z))
    return out


@pytest.mark.parametrize("name", ["bolt", "npt-flange"])
def test_slices_match_the_twin_with_every_chunking(gpu, stacks, name):
    s, res, z, ref = stacks[name]
    sdf = gpu.SDF3HIP(s)
    assert (gpu.layer_heights(sdf.Bounds(), F(F(sdf.Bounds()[5] - sdf.Bounds()[2]) / F(7))) == z).all()
    e0 = sdf.Evaluations()
    dev = gpu.ContourHIP.slices(sdf, res, z)
    assert sdf.Evaluations() - e0 == ref.stats["nx"] * ref.stats["ny"] * 7 == int(dev.stats.evals)
    same(dev, ref, name)
    # layer by layer: each layer alone is the twin's layer
    for k in range(7):
        one = gpu.ContourHIP.slices(sdf, res, z[k:k + 1])
        lay = ref.layers[k]
        assert one.keys.tobytes() == lay.keys.tobytes() and one.xy.tobytes() == lay.xy.tobytes(), (name, k)
        assert one.loop_start.tolist() == lay.loop_start.tolist()
    # one layer per chunk, three layers per chunk (the last chunk shorter), the default: identical bytes
    per_layer = ref.stats["nx"] * ref.stats["ny"]
    for max_nodes in (1, 3 * per_layer, 7 * per_layer + 5):
        same_handles(gpu.ContourHIP.slices(sdf, res, z, max_nodes=max_nodes), dev, (name, max_nodes))
    if name == "npt-flange":
        a = dev.areas()
        for k in range(7):
            assert ((a[dev.loop_layer == k] > 0).sum(), (a[dev.loop_layer == k] < 0).sum()) == (1, 1), k  # the bore is a hole in every layer


def test_an_empty_layer_between_others(gpu, stacks):
    s, res, z, ref = stacks["bolt"]
    per = [int((ref.loop_layer == k).sum()) for k in range(7)]
    assert per[0] == 0 and per[1] > 0 and per[2] > 0, per  # the lowest mid-height of the bolt's box meets no material
    zz = np.array([z[1], z[0], z[2]], F)
    want = contourref.of_oracle(s.tree(), res, zz)
    sdf = gpu.SDF3HIP(s)
    for max_nodes in (0, 1):
        dev = gpu.ContourHIP.slices(sdf, res, zz, max_nodes=max_nodes)
        same(dev, want, ("bolt, empty layer in the middle", max_nodes))
        assert sorted(set(dev.loop_layer.tolist())) == [0, 2] and dev.loops(1) == []


def test_run_twice(gpu, stacks):
    s, res, z, _ = stacks["npt-flange"]
    sdf = gpu.SDF3HIP(s)
    same_handles(gpu.ContourHIP.slices(sdf, res, z), gpu.ContourHIP.slices(sdf, res, z), "slices twice")
    t = _example().scene("text")
    sdf2 = gpu.SDF2HIP(t)
    r2 = res_for(sdf2.Bounds(), 300)
    same_handles(gpu.ContourHIP.outline(sdf2, r2), gpu.ContourHIP.outline(sdf2, r2), "outline twice")


def test_empty_bounds(gpu):
    b = Builder()
    s = b.Intersection2D(b.Translate2D(b.NewCircle(0.4), 0.45, 1), b.NewRectangle(1, 0.61))
    dev = gpu.ContourHIP.outline(gpu.SDF2HIP(s), F(0.1))
    same(dev, contourref.of_oracle(s.tree(), F(0.1)), "empty bounds")
    assert (dev.stats.nx, dev.stats.ny, dev.n_loops, dev.loop_start.tolist()) == (4, 4, 0, [0])


def test_argument_errors(gpu):
    b = Builder()
    s2, s3 = gpu.SDF2HIP(b.NewCircle(1.0)), gpu.SDF3HIP(b.NewSphere(1.0))
    z = np.zeros(1, F)

    def code(fn):
        with pytest.raises(gpu.HipError) as e:
            fn()
        return e.value.code

    DIMENSION, BAD_ARGUMENT = -7, -3  # gsdf_hip.h: GSDF_ERR_DIMENSION, GSDF_ERR_BAD_ARGUMENT
    assert code(lambda: gpu.ContourHIP.outline(s3, 0.1)) == DIMENSION
    assert code(lambda: gpu.ContourHIP.slices(s2, 0.1, z)) == DIMENSION
    for res in (0.0, -0.1, float("nan"), float("inf"), float("-inf")):
        assert code(lambda: gpu.ContourHIP.outline(s2, res)) == BAD_ARGUMENT, res
        assert code(lambda: gpu.ContourHIP.slices(s3, res, z)) == BAD_ARGUMENT, res
    assert code(lambda: gpu.ContourHIP.slices(s3, 0.1, np.zeros(0, F))) == BAD_ARGUMENT
    # 2 / res + 4 nodes a side: 46341^2 >= 2^31 is refused (before any allocation: 2^31 nodes would need 48 GB), as is a quotient
    # beyond int32; nothing was evaluated by any refused call
    e2, e3 = s2.Evaluations(), s3.Evaluations()
    for res in (2.0 / 46338, 1e-7, 1e-30):
        assert code(lambda: gpu.ContourHIP.outline(s2, res)) == BAD_ARGUMENT, res
        assert code(lambda: gpu.ContourHIP.slices(s3, res, z)) == BAD_ARGUMENT, res
    assert (s2.Evaluations(), s3.Evaluations()) == (e2, e3)
    # the handles still work
    assert gpu.ContourHIP.outline(s2, 0.1).n_loops == 1 and gpu.ContourHIP.slices(s3, 0.1, z).n_loops == 1
