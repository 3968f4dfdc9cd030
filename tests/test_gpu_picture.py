"""A 2-D part's picture on the device (gsdf_hip_image2_color; gsdf_amd/csrc/kernels_image.h) against the CPU twin of the colour
conversions (tests/colorref.py) over the oracle's distances: RGBA bytes identical for every conversion kind -- the 2-D corpus, the
reference's example pictures at odd sizes, fields with NaN and infinite distances; the distances identical to gsdf_hip_image2's and
DEFAULT's bytes identical to its bytes; interpreter and per-tree kernels; the evaluation counter; the argument errors; the example's
PNG."""
import importlib.util
import os

import numpy as np
import pytest

import colorref
import corpus
from gsdf_amd import png
from oracle.oracle import OracleSDF
from scaffold.builder import Builder
from tree_edit import clone, first

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _example():
    spec = importlib.util.spec_from_file_location("render_png", os.path.join(ROOT, "examples", "render_png.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _conversions(hip, bb):
    """One conversion of every kind, plus the corners of their arguments: IQ at the default and a short length, a gradient whose
    hues wrap (interpHSV's h0 += 1, hsvToRGB's fall-through), a plain one, black and white with and without smoothing."""
    bb = np.asarray(bb, F)
    diag = float(colorref.iq_default_length(bb)) * 3
    if not diag > 0:  # empty bounds (a disjoint intersection): RenderPNGFile has no default; any length will do
        diag = 3.0
    return [("default", hip.color_default()),
            ("iq", hip.color_iq(bb, diag / 3)),
            ("iq-short", hip.color_iq(bb, diag / 200)),
            ("gradient", hip.color_gradient(diag / 10, (120, 10, 20, 255), (150, 200, 255, 255))),
            ("gradient-wrap", hip.color_gradient(diag / 4, (255, 0, 40, 255), (255, 40, 0, 200))),
            ("gradient-0", hip.color_gradient(0.0, (9, 99, 199, 255), (250, 3, 30, 255))),
            ("bw", hip.color_gradient(diag / 50)),
            ("bw-0", hip.color_gradient(0.0))]


def _same(got, want, what):
    bad = (got != want).any(axis=-1)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:3].tolist(), want[bad][:3].tolist())


def _check_picture(hip, sdf, tree, w, h, what, oracle=True):
    """Every conversion of _conversions: the device's bytes against the twin over the device's own distances everywhere, and over
    the oracle's distances (which must be the device's, bit for bit, where the oracle's are not NaN)."""
    bb = sdf.Bounds()
    d_ref = OracleSDF(tree).Evaluate(colorref.lattice(bb, w, h)).reshape(h, w) if oracle else None
    for name, conv in _conversions(hip, bb):
        rgba, dist = sdf.render_picture(w, h, conv)
        _same(rgba, colorref.convert(dist, conv), (what, name, "twin over the device's distances"))
        if oracle:
            ok = ~np.isnan(d_ref)
            assert (dist.view(np.uint32)[ok] == d_ref.view(np.uint32)[ok]).all(), (what, name)
            _same(rgba[ok], colorref.convert(d_ref[ok], conv), (what, name, "twin over the oracle"))
    return d_ref


def test_corpus_shapes_match_the_twin(gpu):
    _, shapes = corpus.shapes2d()
    for name, s in shapes:
        sdf = gpu.SDF2HIP(s)
        _check_picture(gpu, sdf, s.tree(), 67, 41, name)


@pytest.mark.parametrize("scene", ["image", "text", "thread"])
def test_example_scenes_match_the_twin(gpu, scene):
    s = _example().scene(scene)
    t = s.tree()
    interp = gpu.SDF2HIP(s)
    spec = gpu.SDF2HIP(s).specialize()
    for w, h in ((257, 131), (64, 200), (1, 1), (3, 97)):
        _check_picture(gpu, spec, t, w, h, (scene, w, h, "specialised"))
        for name, conv in _conversions(gpu, interp.Bounds()):
            a = spec.render_picture(w, h, conv)
            b = interp.render_picture(w, h, conv)
            assert (a[0] == b[0]).all() and (a[1].view(np.uint32) == b[1].view(np.uint32)).all(), (scene, w, h, name)
    # the comparison above was per-tree against interpreter: every kind's per-tree kernel was built and launched
    assert spec.info()["kernels"]["picture"].endswith(":specialised/0123"), spec.info()["kernels"]
    assert interp.info()["kernels"]["picture"].endswith(":interpreter"), interp.info()["kernels"]
    # the picture RenderPNGFile draws, at its own size
    w = gpu.picture_size(spec.Bounds(), 300)
    rgba, dist = spec.render_picture(w, 300)
    _same(rgba, colorref.iq(dist, colorref.iq_default_length(spec.Bounds())), (scene, "RenderPNGFile default"))
    assert len(np.unique(rgba.reshape(-1, 4), axis=0)) > 20, scene


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
    seen = {"nan": 0, "inf": 0}
    for name, t in _nonfinite_trees():
        for spec in (False, True):
            sdf = gpu.SDF2HIP(t)
            if spec:
                sdf.specialize()
            # the oracle differs from the device where it meets NaN (tests/test_gpu_nan.py): held to the twin over the device's own
            # distances everywhere, and to the oracle where the oracle is not NaN
            _check_picture(gpu, sdf, t, 53, 29, (name, spec))
            assert sdf.info()["kernels"]["picture"].endswith(":specialised/0123" if spec else ":interpreter"), (name, sdf.info()["kernels"])
            _, dist = sdf.render_picture(53, 29)
            seen["nan"] += int(np.isnan(dist).sum())
            seen["inf"] += int(np.isinf(dist).sum())
    assert seen["nan"] > 0 and seen["inf"] > 0, seen


def test_agrees_with_image2(gpu):
    for s in (_example().scene("image"), _example().scene("thread"), Builder().NewHexagon(1.0)):
        for spec in (False, True):
            sdf = gpu.SDF2HIP(s)
            if spec:
                sdf.specialize()
            for w, h in ((211, 97), (640, 360)):
                dist2, rgba2 = sdf.render_image(w, h)
                rgba, dist = sdf.render_picture(w, h, gpu.color_default())
                assert (dist.view(np.uint32) == dist2.view(np.uint32)).all()
                assert (rgba == rgba2).all()
                rgba_iq, dist_iq = sdf.render_picture(w, h)
                assert (dist_iq.view(np.uint32) == dist2.view(np.uint32)).all()


def test_counter_grows_by_the_pixels(gpu):
    s = _example().scene("image")
    for spec in (False, True):
        sdf = gpu.SDF2HIP(s)
        if spec:
            sdf.specialize()
        for conv in (gpu.color_default(), gpu.color_iq(sdf.Bounds()), gpu.color_gradient(0.5, (1, 2, 3, 255), (4, 5, 6, 255)),
                     gpu.color_gradient(0.5)):
            e0 = sdf.Evaluations()
            sdf.render_picture(123, 45, conv)
            assert sdf.Evaluations() - e0 == 123 * 45


def test_argument_errors(gpu):
    b = Builder()
    sdf = gpu.SDF2HIP(b.NewCircle(1.0))
    bb = sdf.Bounds()
    ok = gpu.color_iq(bb)
    for w, h in ((0, 10), (10, 0), (-3, 5), (16385, 4), (4, 16385)):
        with pytest.raises(gpu.HipError) as e:
            sdf.render_picture(w, h, ok)
        assert e.value.code == -3, (w, h)

    def bad(**kw):
        c = gpu.color_iq(bb)
        for k, v in kw.items():
            if k == "reserved":
                c.reserved[v] = 1
            else:
                setattr(c, k, v)
        return c
    for conv in (bad(kind=4), bad(kind=-1), bad(length=0.0), bad(length=-1.0), bad(length=float("inf")), bad(length=float("nan")),
                 bad(reserved=0), bad(reserved=3), bad(kind=gpu.COLOR_GRADIENT, length=-0.5), bad(kind=gpu.COLOR_BW_SMOOTH, length=-1e-9),
                 bad(kind=gpu.COLOR_BW_SMOOTH, length=float("inf"))):
        with pytest.raises(gpu.HipError) as e:
            sdf.render_picture(8, 8, conv)
        assert e.value.code == -3, (conv.kind, conv.length, list(conv.reserved))
    # a NULL conversion
    with pytest.raises(gpu.HipError) as e:
        gpu._check(gpu.lib().gsdf_hip_image2_color(sdf._h, None, 8, 8, None, None))
    assert e.value.code == -3
    solid = gpu.SDF3HIP(b.NewSphere(1.0))
    with pytest.raises(gpu.HipError) as e:
        solid.render_picture(8, 8, ok)
    assert e.value.code == -7
    # both outputs optional; the largest size per side is accepted
    gpu._check(gpu.lib().gsdf_hip_image2_color(sdf._h, ok, 16384, 1, None, None))
    e0 = sdf.Evaluations()
    gpu._check(gpu.lib().gsdf_hip_image2_color(sdf._h, ok, 3, 5, None, None))
    assert sdf.Evaluations() - e0 == 15


def test_example_writes_the_picture_as_png(gpu, tmp_path):
    mod = _example()
    for scene, color, height in (("image", None, 64), ("text", "bw", 48), ("thread", "gradient", 80)):
        out = str(tmp_path / f"{scene}.png")
        args = [scene, "--height", str(height), "-o", out] + (["--color", color] if color else [])
        assert mod.main(args) == 0
        s = mod.scene(scene)
        sdf = gpu.SDF2HIP(s)
        w = gpu.picture_size(sdf.Bounds(), height)
        want, _ = sdf.render_picture(w, height, mod.conversion(gpu, color or mod.SCENES[scene][1], sdf.Bounds()))
        got = png.read_png(out)
        assert got.shape == (height, w, 4) and (got == want).all(), scene
    # render_png: RenderPNGFile's flow with its defaults
    s = mod.scene("image")
    sdf = gpu.SDF2HIP(s)
    out = str(tmp_path / "rpf.png")
    rgba = sdf.render_png(out, 54)
    assert rgba.shape == (54, 108, 4) and (png.read_png(out) == rgba).all()
    assert (rgba == sdf.render_picture(108, 54, gpu.color_iq(sdf.Bounds()))[0]).all()
