"""The UI's view on the device (gsdf_hip_render3; gsdf_amd/csrc/kernels_view.h) against its CPU twin (tests/viewref.py) over the
oracle: RGBA bytes, depth bits and per-pixel evaluation counts identical -- corpus shapes, the example parts (the fibonacci
showerhead is not 1-Lipschitz), supersampling, clamped pitch, a camera inside the part, an off-origin target, a degenerate tree;
interpreter and per-tree kernels, refilling and plain kernels, repeated frames; the argument errors; the example's PNG."""
import importlib.util
import os
import struct
import zlib

import numpy as np
import pytest

import corpus
import viewref
from oracle.oracle import OracleSDF
from scaffold.builder import Builder

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = ["npt-flange", "bolt", "knurled-cylinder", "glyph-plate", "fibonacci-showerhead"]


def _twin(tree, view, w, h):
    return viewref.render(OracleSDF(tree).Evaluate, view, w, h)


def _same(dev, twin, what, mask=None):
    rgba, depth, evals = dev
    m = np.ones(depth.shape, bool) if mask is None else mask
    bad = (rgba != twin["rgba"]).any(axis=2) | (depth.view(np.uint32) != twin["depth"].view(np.uint32)) | (evals != twin["evals"])
    bad &= m
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist())


def _frame(hip, sdf, view, w, h, monkeypatch=None, plain=False):
    if monkeypatch is not None:
        monkeypatch.setenv("GSDF_HIP_VIEW_REFILL", "0" if plain else "1")
    return sdf.render3(view, w, h)


def _inside_point(tree):
    """The most negative of a coarse lattice over the bounds (a point in the part's material)."""
    bb = np.array(tree.bb[:], np.float32)
    g = np.stack(np.meshgrid(*[np.linspace(bb[a], bb[a + 3], 17, dtype=np.float32) for a in range(3)], indexing="ij"), -1).reshape(-1, 3)
    d = OracleSDF(tree).Evaluate(g)
    return g[int(np.argmin(d))]


def test_corpus_shapes_match_the_twin(gpu):
    _, shapes = corpus.shapes3d()
    hits = 0
    for name, s in shapes:
        sdf = gpu.SDF3HIP(s)
        v = gpu.view_orbit(s.Bounds(), 0.6, 0.35)
        dev = sdf.render3(v, 32, 24)
        tw = _twin(s.tree(), v, 32, 24)
        _same(dev, tw, name)
        hits += int(np.isfinite(tw["depth"]).sum())
    assert hits > 1000


@pytest.mark.parametrize("scene", SCENES)
def test_scenes_match_the_twin(gpu, scene, monkeypatch):
    s = Builder().Scene(scene)
    t = s.tree()
    interp = gpu.SDF3HIP(s)
    spec = gpu.SDF3HIP(s).specialize()
    bb = s.Bounds()
    diag = float(s.Diagonal())
    cams = [dict(yaw=0.5, pitch=0.4), dict(yaw=-2.2, pitch=2.0),  # pitch clamped to pi/2 - 0.01
            dict(yaw=1.1, pitch=-0.3, cam_dist=0.6 * diag, target=tuple(0.25 * (bb[:3] + bb[3:]))),  # off-origin target
            dict(yaw=0.3, pitch=0.2, cam_dist=1e-3 * diag, target=tuple(_inside_point(t)))]  # camera inside the part
    for k, cam in enumerate(cams):
        for w, h, aa in ((160, 120, 1), (64, 48, 3)):
            if k >= 2 and aa == 3:
                continue
            v = gpu.view_orbit(bb, aa=aa, **cam)
            tw = _twin(t, v, w, h)
            e0 = spec.Evaluations()
            a = _frame(gpu, spec, v, w, h, monkeypatch, plain=False)
            assert spec.Evaluations() - e0 == int(tw["evals"].astype(np.int64).sum())
            _same(a, tw, (scene, cam, aa, "specialised"))
            _same(_frame(gpu, spec, v, w, h, monkeypatch, plain=True), tw, (scene, cam, aa, "specialised, plain"))
            _same(_frame(gpu, interp, v, w, h, monkeypatch, plain=False), tw, (scene, cam, aa, "interpreter"))
            if k == 0:
                _same(_frame(gpu, interp, v, w, h, monkeypatch, plain=True), tw, (scene, cam, aa, "interpreter, plain"))
                b = _frame(gpu, spec, v, w, h, monkeypatch, plain=False)
                assert all((x == y).all() for x, y in zip(a, b)), "two renders of one frame differ"
            if k == 3:
                assert np.isfinite(tw["depth"]).all() and (tw["depth"] == 0).all()  # every ray starts in the material
            elif k == 0:
                assert 0.05 < np.isfinite(tw["depth"]).mean() < 0.95, scene


def test_degenerate_tree_where_the_oracle_is_finite(gpu):
    from test_gpu_nan import degenerate_trees
    trees = dict(degenerate_trees())
    masked = 0
    for name in ("smooth-union-k0", "scale-zero"):
        t = trees[name]
        bb = np.array(t.bb[:], np.float32)
        v = gpu.view_orbit(bb, 0.5, 0.3)
        tw = _twin(t, v, 64, 48)
        for spec in (False, True):
            sdf = gpu.SDFHIP(t)
            if spec:
                sdf.specialize()
            a = sdf.render3(v, 64, 48)
            _same(a, tw, (name, spec), mask=~tw["nonfinite"])
            assert (a[0][..., 3] == 255).all()
            b = sdf.render3(v, 64, 48)
            assert all((x == y).all() for x, y in zip(a, b)), name
        masked += int(tw["nonfinite"].sum())
    assert masked < 2 * 64 * 48


def test_full_hd_specialised_equals_interpreter(gpu, monkeypatch):
    s = Builder().Scene("npt-flange")
    spec = gpu.SDF3HIP(s).specialize()
    interp = gpu.SDF3HIP(s)
    v = gpu.view_orbit(s.Bounds(), 0.7, 0.45)
    a = _frame(gpu, spec, v, 1920, 1080, monkeypatch)
    b = _frame(gpu, interp, v, 1920, 1080, monkeypatch)
    assert all((x == y).all() for x, y in zip(a, b))
    assert np.isfinite(a[1]).mean() > 0.05
    _same(spec.render3(v, 480, 270), _twin(s.tree(), v, 480, 270), "npt-flange 480x270")


def test_argument_errors(gpu):
    b = Builder()
    s = b.NewSphere(1.0)
    sdf = gpu.SDF3HIP(s)
    v = gpu.view_orbit(s.Bounds(), 0.1, 0.2)
    for w, h in ((0, 10), (10, 0), (-3, 5), (20000, 4)):
        with pytest.raises(gpu.HipError) as e:
            sdf.render3(v, w, h)
        assert e.value.code == -3
    for field, val in (("aa", 0), ("aa", 9), ("max_steps", -1), ("max_steps", 4097)):
        bad = gpu.view_orbit(s.Bounds(), 0.1, 0.2)
        setattr(bad, field, val)
        with pytest.raises(gpu.HipError) as e:
            sdf.render3(bad, 8, 8)
        assert e.value.code == -3, (field, val)
    for field in ("ro", "ww"):
        bad = gpu.view_orbit(s.Bounds(), 0.1, 0.2)
        getattr(bad, field)[1] = float("nan")
        with pytest.raises(gpu.HipError) as e:
            sdf.render3(bad, 8, 8)
        assert e.value.code == -3
    bad = gpu.view_orbit(s.Bounds(), 0.1, 0.2)
    bad.char_dist = float("inf")
    with pytest.raises(gpu.HipError):
        sdf.render3(bad, 8, 8)
    flat = gpu.SDF2HIP(b.NewCircle(1.0))
    with pytest.raises(gpu.HipError) as e:
        flat.render3(v, 8, 8)
    assert e.value.code == -7
    v.max_steps = 0
    e0 = sdf.Evaluations()
    rgba, depth, evals = sdf.render3(v, 8, 6)
    assert (rgba[..., :3] == 0).all() and (rgba[..., 3] == 255).all() and np.isinf(depth).all() and (evals == 0).all()
    assert sdf.Evaluations() == e0


def _read_png(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    off, idat, w, h = 8, b"", None, None
    while off < len(data):
        n, = struct.unpack(">I", data[off:off + 4])
        kind, body = data[off + 4:off + 8], data[off + 8:off + 8 + n]
        assert zlib.crc32(kind + body) == struct.unpack(">I", data[off + 8 + n:off + 12 + n])[0]
        if kind == b"IHDR":
            w, h, depth, ctype = struct.unpack(">IIBB", body[:10])
            assert depth == 8 and ctype == 6
        elif kind == b"IDAT":
            idat += body
        off += 12 + n
    raw = np.frombuffer(zlib.decompress(idat), np.uint8).reshape(h, 1 + 4 * w)
    assert (raw[:, 0] == 0).all()
    return raw[:, 1:].reshape(h, w, 4)


def test_example_writes_the_frame_as_png(gpu, tmp_path):
    spec = importlib.util.spec_from_file_location("view_part", os.path.join(ROOT, "examples", "view_part.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = str(tmp_path / "part.png")
    assert mod.main(["bolt", "--width", "96", "--height", "64", "--yaw", "0.8", "--pitch", "0.3", "--aa", "2", "-o", out]) == 0
    s = Builder().Scene("bolt")
    rgba, _, _ = gpu.SDF3HIP(s).render_view(96, 64, yaw=0.8, pitch=0.3, aa=2)
    png = _read_png(out)
    assert (png == rgba).all() and (rgba[..., :3] > 0).any()
