"""gsdfaux's colour conversions and RenderPNGFile's geometry, host side (no GPU): the host-only helpers gsdf_hip_picture_size,
gsdf_hip_color_iq and gsdf_hip_color_gradient against the reference's formulas (gsdfaux/gsdfaux.go:264-296, color.go:50-56), and
the CPU twin of the conversions (tests/colorref.py) at its anchors: the colours color.go names, the special cases, the float64
Exp / Cos statements against correctly rounded values, and the untyped constants."""
import ctypes as C
import os
import re
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import colorref
from gsdf_amd import hip, png

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMAGE_BB = np.array([-20, -20, 0, 60, 20, 0], F)  # examples/image: circle of radius 20 and the triangle (20,0) (60,20) (60,-20)


def test_struct_layout():
    assert C.sizeof(hip.GsdfColor2) == 32
    assert hip.GsdfColor2.length.offset == 4 and hip.GsdfColor2.c0.offset == 8 and hip.GsdfColor2.c1.offset == 12
    assert hip.GsdfColor2.reserved.offset == 16


def test_picture_size_of_the_image_example():
    assert hip.picture_size(IMAGE_BB, 1080) == 2160
    assert colorref.picture_size(IMAGE_BB, 1080) == 2160


@pytest.mark.parametrize("bb,hgt", [((0, 0, 0, 3, 7, 0), 300), ((-1.5, -0.1, 0, 2.25, 0.3, 0), 512), ((0, 0, 0, 1, 3, 0), 1000),
                                    ((-0.7, 2.1, 0, 0.6, 2.9, 0), 97), ((0, 0, 0, 10, 10 / 3, 0), 1080), ((0, 0, 0, 0.1, 7.7, 0), 4321)])
def test_picture_size_odd_aspect_ratios(bb, hgt):
    bb = np.array(bb, F)
    assert hip.picture_size(bb, hgt) == colorref.picture_size(bb, hgt)
    # float64 of the float32 size, truncated: not the float32 quotient's
    szx, szy = float(F(bb[3] - bb[0])), float(F(bb[4] - bb[1]))
    assert hip.picture_size(bb, hgt) == int(hgt / szy * szx)


def test_picture_size_errors():
    for bb, hgt in (((0, 0, 0, 1, 0, 0), 10),             # sz.Y == 0
                    ((0, 1, 0, 1, 0, 0), 10),             # sz.Y < 0
                    ((0, 0, 0, float("nan"), 1, 0), 10),  # non-finite
                    ((0, 0, 0, 1, float("inf"), 0), 10),
                    ((0, 0, 0, 1, 1, 0), 0),              # height out of range
                    ((0, 0, 0, 1, 1, 0), 16385),
                    ((0, 0, 0, 1e-3, 1, 0), 100),         # width 0
                    ((0, 0, 0, 100, 1, 0), 200)):         # width 20000
        with pytest.raises(hip.HipError) as e:
            hip.picture_size(np.array(bb, F), hgt)
        assert e.value.code == -3, (bb, hgt)
    assert hip.picture_size(np.array((0, 0, 0, 1, 1, 0), F), 16384) == 16384


def test_iq_default_is_the_diagonal_over_three():
    c = hip.color_iq(IMAGE_BB)
    assert c.kind == hip.COLOR_IQ and list(c.reserved) == [0, 0, 0, 0]
    want = colorref.iq_default_length(IMAGE_BB)
    assert F(c.length).view(np.uint32) == want.view(np.uint32)
    assert abs(float(want) - np.hypot(80, 40) / 3) < 1e-4
    for bb in ((-1.5, -0.1, 0, 2.25, 0.3, 0), (0, 0, 0, 1e-3, 7, 0), (3, 4, 0, 3, 9, 0)):
        bb = np.array(bb, F)
        assert F(hip.color_iq(bb, 0).length) == colorref.iq_default_length(bb)
        assert F(hip.color_iq(bb, -1).length) == colorref.iq_default_length(bb)
    assert F(hip.color_iq(IMAGE_BB, 2.5).length) == F(2.5)
    with pytest.raises(hip.HipError):
        hip.color_iq(np.zeros(6, F))  # empty bounds, no distance
    with pytest.raises(hip.HipError):
        hip.color_iq(IMAGE_BB, float("inf"))
    with pytest.raises(hip.HipError):
        hip.color_iq(np.array([0, 0, 0, float("nan"), 1, 0], F))


def test_gradient_constructor_maps_black_to_white_on_bw():
    assert hip.color_gradient(0.5).kind == hip.COLOR_BW_SMOOTH
    assert hip.color_gradient(0.5, (0, 0, 0, 255), (255, 255, 255, 255)).kind == hip.COLOR_BW_SMOOTH
    for c0, c1 in (((255, 255, 255, 255), (0, 0, 0, 255)), ((0, 0, 0, 254), (255, 255, 255, 255)), ((10, 200, 30, 255), (0, 0, 255, 255))):
        c = hip.color_gradient(0.5, c0, c1)
        assert c.kind == hip.COLOR_GRADIENT and tuple(c.c0) == c0 and tuple(c.c1) == c1 and F(c.length) == F(0.5)
    assert hip.color_gradient(0.0).length == 0.0
    for bad in (-1.0, float("nan"), float("inf")):
        with pytest.raises(hip.HipError) as e:
            hip.color_gradient(bad)
        assert e.value.code == -3


def test_iq_anchors():
    out = colorref.iq(np.array([0.0, -0.0, np.nan, np.inf, -np.inf], F), F(2.0))
    assert (out[0] == (255, 255, 255, 255)).all() and (out[1] == (255, 255, 255, 255)).all()  # SmoothStep's white edge
    assert (out[2] == (255, 0, 0, 255)).all()                                                   # red for NaN
    assert (out[3] == (0, 0, 0, 255)).all() and (out[4] == (0, 0, 0, 255)).all()               # Cos(Inf) = NaN -> u8(NaN) = 0
    # far from the edge the base colours show through, with the distance bands: outside orange, inside blue
    d = np.linspace(0.3, 3, 200, dtype=F)
    o, i = colorref.iq(d, F(1)), colorref.iq(-d, F(1))
    assert (o[:, 0] > o[:, 1]).all() and (o[:, 1] > o[:, 2]).all()
    assert (i[:, 2] > i[:, 1]).all() and (i[:, 1] > i[:, 0]).all()
    assert len(np.unique(o[:, 0])) > 20  # the cosine bands


def test_gradient_anchors():
    c0, c1 = (200, 30, 40, 255), (20, 60, 230, 255)
    d = np.array([-10, -0.5, -0.25, 0, 0.25, 0.5, 10, -np.inf, np.inf], F)
    out = colorref.gradient(d, F(1.0), c0, c1)
    for k in (0, 1, 7):
        assert tuple(out[k]) == c0
    for k in (5, 6, 8):
        assert tuple(out[k]) == c1
    assert (out[2:5, 3] == 255).all()
    # an end colour stored with its own alpha comes back as stored (image.RGBA keeps a color.RGBA's bytes)
    assert tuple(colorref.gradient(np.array([-5], F), F(1), (10, 20, 30, 128), c1)[0]) == (10, 20, 30, 128)
    # NaN takes the HSV path with blend NaN: h outside [0, 1] -> (0,0,0) + m = NaN -> u32(NaN) = 0
    assert tuple(colorref.gradient(np.array([np.nan], F), F(1), c0, c1)[0]) == (0, 0, 0, 255)
    # hsvToRGB at the primary colours, exactly
    for c in ((255, 0, 0, 255), (0, 255, 0, 255), (0, 0, 255, 255), (255, 255, 0, 255), (0, 255, 255, 255), (255, 0, 255, 255)):
        h, s, v = colorref.color_to_hsv(c)
        r, g, b = colorref.hsv_to_rgb(np.array([h], F), np.array([s], F), np.array([v], F))
        assert (F(r[0]) * 255, F(g[0]) * 255, F(b[0]) * 255) == tuple(F(x) for x in c[:3])


def test_hsv_wraps_to_an_h_above_one():
    """interpHSV's wrap (h0 += 1) gives hues above 1 mid-way; the switch has no case for them and gives (m, m, m)."""
    c0, c1 = (255, 0, 40, 255), (255, 40, 0, 255)  # hues just below 1 and just above 0
    h0, _, _ = colorref.color_to_hsv(c0)
    h1, _, _ = colorref.color_to_hsv(c1)
    assert h1 - h0 < -0.5
    out = colorref.gradient(np.linspace(-0.49, 0.49, 99, dtype=F), F(1), c0, c1)
    assert ((out[:, 0] == out[:, 1]) & (out[:, 1] == out[:, 2])).any()


def test_bw_anchors():
    nos = colorref.bw(np.array([-1, -0.0, 0, 1, np.nan, -np.inf, np.inf], F), F(0))
    assert [tuple(p) for p in nos] == [(0, 0, 0, 255)] + [(255, 255, 255, 255)] * 4 + [(0, 0, 0, 255), (255, 255, 255, 255)]
    d = np.linspace(-1, 1, 2001, dtype=F)
    ramp = colorref.bw(d, F(0.5))
    y = ramp[:, 0].astype(int)
    assert (ramp[:, 0] == ramp[:, 1]).all() and (ramp[:, 1] == ramp[:, 2]).all() and (ramp[:, 3] == 255).all()
    assert (np.diff(y) >= 0).all() and y[0] == 0 and y[-1] == 255 and len(np.unique(y)) == 256
    assert tuple(colorref.bw(np.array([np.nan], F), F(0.5))[0]) == (0, 0, 0, 255)  # Clamp(NaN) -> u8(NaN) = 0


def test_default_anchors():
    out = colorref.default(np.array([-1, 0, 1, np.nan, np.inf, -np.inf], F))
    assert [tuple(p) for p in out] == [(0, 0, 0, 255), (0, 0, 0, 255), (255, 255, 255, 255)] + [(255, 0, 0, 255)] * 3


def test_float_to_integer_conversions():
    v = np.array([0, 0.99, 1, 254.9, 255, 255.5, 256, 300, -0.5, -1, -3, np.nan, np.inf, -np.inf, 2.0 ** 63, 2.0 ** 62], F)
    got = colorref.to_int_bits(v) & np.uint64(0xff)
    assert got.tolist() == [0, 0, 1, 254, 255, 255, 0, 44, 0, 255, 253, 0, 0, 0, 0, 0]


def _round32(x):
    """float32 nearest to the mpmath value x."""
    if mpmath.isnan(x):
        return F(np.nan)
    if mpmath.isinf(x):
        return F(np.inf) if x > 0 else F(-np.inf)
    if abs(x) >= mpmath.mpf(2) ** 129:
        return F(np.inf) if x > 0 else F(-np.inf)
    if abs(x) < mpmath.mpf(2) ** -151:
        return F(0.0) if x >= 0 else F(-0.0)
    m, e = mpmath.mpf(x).man_exp  # (|mantissa|: the sign is kept apart)
    q = Fraction(int(m)) * Fraction(2) ** int(e)
    return colorref.const32(-q if x < 0 else q)


def _sweep(lo, hi, n, rng):
    return np.concatenate([np.linspace(lo, hi, n // 2, dtype=F), (lo + (hi - lo) * rng.random(n // 2)).astype(F)])


def test_exp_statement_against_correct_rounding():
    rng = np.random.default_rng(1)
    x = np.concatenate([_sweep(-110, 95, 3000, rng), _sweep(-1, 1, 1000, rng), _sweep(-1e-6, 1e-6, 400, rng),
                        np.array([0, -0.0, 2.0 ** -28, -2.0 ** -28, 2.0 ** -29, 88.72283, 88.72284, 88.7229, 89, -87.33655, -103.27893,
                                  -103.9721, -103.98, -104, 709.78, 709.79, 710, -745.13, -745.14, -746, 3e38, -3e38,
                                  np.inf, -np.inf, np.nan], F)]).astype(F)
    got = colorref.expf(x)
    mpmath.mp.prec = 200
    want = np.array([_round32(mpmath.exp(mpmath.mpf(float(v)))) if np.isfinite(v) else F(np.exp(v)) for v in x], F)
    same = (got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))
    nbad = int((~same).sum())
    print(f"Exp: {nbad} of {len(x)} float32 arguments differ from the correctly rounded value")
    assert nbad <= 5, x[~same][:10]
    # the special cases of exp.go
    assert colorref.exp64(np.array([np.inf]))[0] == np.inf and colorref.exp64(np.array([-np.inf]))[0] == 0
    assert colorref.exp64(np.array([710.0]))[0] == np.inf and colorref.exp64(np.array([-746.0]))[0] == 0
    assert colorref.exp64(np.array([2.0 ** -30]))[0] == 1 + 2.0 ** -30
    assert np.isnan(colorref.exp64(np.array([np.nan]))[0])


def test_cos_statement_against_correct_rounding():
    rng = np.random.default_rng(2)
    x = np.concatenate([_sweep(-20, 20, 2000, rng), _sweep(-2e4, 2e4, 2000, rng), _sweep(-2.0 ** 29, 2.0 ** 29, 600, rng),
                        (np.pi / 4 * np.arange(-40, 41)).astype(F), np.array([0, -0.0, 1e-20, 2.0 ** 28], F)]).astype(F)
    got = colorref.cosf(x)
    mpmath.mp.prec = 200
    want = np.array([_round32(mpmath.cos(mpmath.mpf(float(v)))) for v in x], F)
    same = got.view(np.uint32) == want.view(np.uint32)
    nbad = int((~same).sum())
    print(f"Cos: {nbad} of {len(x)} float32 arguments below 2^29 differ from the correctly rounded value")
    assert nbad <= 5, x[~same][:10]
    assert np.isnan(colorref.cos64(np.array([np.inf, -np.inf, np.nan]))).all()
    # beyond x (4/pi) >= 2^64 the integer part is 0 (the contract's pin): the cosine polynomial of the unreduced argument
    zz = np.float64(1e20) * np.float64(1e20)
    c = colorref._COS
    want = 1.0 - 0.5 * zz + zz * zz * ((((((c[0] * zz) + c[1]) * zz + c[2]) * zz + c[3]) * zz + c[4]) * zz + c[5])
    assert np.isfinite(want) and colorref.cos64(np.array([-1e20]))[0] == want
    # (far beyond 2^29 Cody-Waite's three-part pi/4 leaves a residue of the size of the argument: where Go reduces exactly, these
    # statements give values outside [-1, 1]; IQ meets them only at distances of millions of characteristic lengths)
    assert abs(colorref.cos64(np.array([1e19]))[0]) > 1
    assert colorref._FOUR_OVER_PI == float(mpmath.mpf(4) / mpmath.pi)


def test_constants_are_the_nearest_float32_of_the_rationals():
    for k in range(1, 7):
        q = Fraction(k, 6)
        c = colorref.const32(q)
        # the nearest float32: no other float32 is closer
        for nb in (np.nextafter(c, F(0)), np.nextafter(c, F(2))):
            assert abs(Fraction(float(c)) - q) <= abs(Fraction(float(nb)) - q), k
    assert colorref.K1_6 == colorref.const32(Fraction(1, 6)) and colorref.K5_6 == colorref.const32(Fraction(5, 6))
    assert colorref.K1_3 == colorref.const32(Fraction(1, 3)) and colorref.K2_3 == colorref.const32(Fraction(2, 3))
    # the device kernel's literals are the same float32 values
    src = open(os.path.join(ROOT, "gsdf_amd", "csrc", "kernels_image.h")).read()
    lits = dict(re.findall(r"constexpr float (k\d_\d) = ([0-9.]+)f;", src))
    assert len(lits) == 4
    for name, q in (("k1_6", Fraction(1, 6)), ("k1_3", Fraction(1, 3)), ("k2_3", Fraction(2, 3)), ("k5_6", Fraction(5, 6))):
        assert F(float(lits[name])) == colorref.const32(q), name
        assert Fraction(lits[name]) == Fraction(float(colorref.const32(q))), name  # written out exactly


def test_mod_is_the_exact_remainder():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.random(5000).astype(F) * F(12), np.array([0, 2, 4, 11.999999, 1e-40, 6, 1.9999999], F)]).astype(F)
    assert (colorref.fmod2(x).view(np.uint32) == np.fmod(x, F(2)).view(np.uint32)).all()


def test_png_round_trip(tmp_path):
    rng = np.random.default_rng(4)
    rgba = rng.integers(0, 256, (37, 53, 4), dtype=np.uint8)
    path = str(tmp_path / "x.png")
    png.write_png(path, rgba)
    assert (png.read_png(path) == rgba).all()
