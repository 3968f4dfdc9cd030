"""CPU twin of gsdfaux's colour conversions as include/gsdf_hip.h states them (gsdf_color2; gsdfaux/color.go), in numpy: every
float32 step one float32 operation, every float64 step of Exp / Cos one float64 operation, in the contract's order. The device
kernel (gsdf_amd/csrc/kernels_image.h) must give the same bytes for the same distances. Also RenderPNGFile's picture size
(gsdfaux.go:271-274) in float64, as Go computes it.

The float32 constants Go writes as untyped expressions (1.0/6, 2.0/3, ...) are the float32 values nearest to the exact rationals
(`const32`), computed from fractions.Fraction -- rounding 1/6 to float64 first and then to float32 can differ in general.
"""
import math
from fractions import Fraction

import numpy as np

F = np.float32
D = np.float64
DEFAULT, IQ, GRADIENT, BW_SMOOTH = 0, 1, 2, 3


def const32(q):
    """The float32 nearest to the rational q (ties to even), without a detour through float64."""
    q = Fraction(q)
    if q == 0:
        return F(0)
    sign, q = (-1, -q) if q < 0 else (1, q)
    e = math.floor(math.log2(q.numerator) - math.log2(q.denominator))
    while Fraction(2) ** e > q:
        e -= 1
    while Fraction(2) ** (e + 1) <= q:
        e += 1
    e = max(e, -126)
    ulp = Fraction(2) ** (e - 23)
    m = q / ulp
    n = math.floor(m)
    r = m - n
    if r > Fraction(1, 2) or (r == Fraction(1, 2) and n % 2 == 1):
        n += 1
    if n * ulp >= Fraction(2) ** 128:  # beyond the largest float32 (or rounded up to 2^128)
        return F(sign * np.inf)
    return F(sign * float(n * ulp))


K1_6, K1_3, K2_3, K5_6 = const32(Fraction(1, 6)), const32(Fraction(2, 6)), const32(Fraction(4, 6)), const32(Fraction(5, 6))
K3_6 = const32(Fraction(3, 6))

# ---- float64 Exp and Cos (the contract's statements of Go's math.Exp and math.Cos) ----------------------------------------------
_LN2HI, _LN2LO, _LOG2E = 6.93147180369123816490e-01, 1.90821492927058770002e-10, 1.44269504088896338700e+00
_OVERFLOW, _UNDERFLOW, _NEARZERO = 7.09782712893383973096e+02, -7.45133219101941108420e+02, 1.0 / (1 << 28)
_P = (1.66666666666666657415e-01, -2.77777777770155933842e-03, 6.61375632143793436117e-05, -1.65339022054652515390e-06,
      4.13813679705723846039e-08)
_SIN = (1.58962301576546568060e-10, -2.50507477628578072866e-8, 2.75573136213857245213e-6, -1.98412698295895385996e-4,
        8.33333333332211858878e-3, -1.66666666666666307295e-1)
_COS = (-1.13585365213876817300e-11, 2.08757008419747316778e-9, -2.75573141792967388112e-7, 2.48015872888517045348e-5,
        -1.38888888888730564116e-3, 4.16666666666665929218e-2)
_PI4A, _PI4B, _PI4C = 7.85398125648498535156e-1, 3.77489470793079817668e-8, 2.69515142907905952645e-15
_FOUR_OVER_PI = 4 / math.pi  # the float64 nearest to 4/pi (checked in tests/test_color_host.py)


def exp64(x):
    """math.Exp (go/src/math/exp.go) over a float64 array."""
    x = np.asarray(x, D)
    with np.errstate(all="ignore"):
        nan, pinf, ninf = np.isnan(x), x == np.inf, x == -np.inf
        over, under = ~nan & (x > _OVERFLOW) & ~pinf, ~nan & (x < _UNDERFLOW) & ~ninf
        near = (-_NEARZERO < x) & (x < _NEARZERO)
        reg = ~(nan | pinf | ninf | over | under | near)
        xr = np.where(reg, x, 1.0)
        k = np.where(xr < 0, np.trunc(_LOG2E * xr - 0.5), np.where(xr > 0, np.trunc(_LOG2E * xr + 0.5), 0.0))
        hi = xr - k * _LN2HI
        lo = k * _LN2LO
        r = hi - lo
        t = r * r
        c = r - t * (_P[0] + t * (_P[1] + t * (_P[2] + t * (_P[3] + t * _P[4]))))
        y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi)
        ki = k.astype(np.int64)
        k1 = np.sign(ki) * (np.abs(ki) // 2)  # C's k / 2 (towards zero)
        k2 = ki - k1
        res = (y * np.ldexp(1.0, k1)) * np.ldexp(1.0, k2)
        out = np.where(reg, res, 0.0)
        out = np.where(near, 1.0 + x, out)
        out = np.where(over | pinf, np.inf, out)
        out = np.where(nan, x, out)
        return out


def cos64(x):
    """math.Cos (go/src/math/sin.go) with Cody-Waite reduction at every finite argument; an integer part >= 2^64 is taken as 0."""
    x = np.asarray(x, D)
    with np.errstate(all="ignore"):
        bad = ~np.isfinite(x)
        ax = np.abs(np.where(bad, 0.0, x))
        v = ax * _FOUR_OVER_PI
        y = np.where(v < 18446744073709551616.0, np.floor(v), 0.0)  # (double)(uint64)v: exact
        j = (y - 8.0 * np.floor(y * 0.125)).astype(np.int64)  # j & 7, exactly
        odd = (j & 1) == 1
        j = np.where(odd, (j + 1) & 7, j)
        y = np.where(odd, y + 1.0, y)
        z = ((ax - y * _PI4A) - y * _PI4B) - y * _PI4C
        sign = j > 3
        j = np.where(j > 3, j - 4, j)
        sign = np.where(j > 1, ~sign, sign)
        zz = z * z
        ps = z + z * zz * ((((((_SIN[0] * zz) + _SIN[1]) * zz + _SIN[2]) * zz + _SIN[3]) * zz + _SIN[4]) * zz + _SIN[5])
        pc = 1.0 - 0.5 * zz + zz * zz * ((((((_COS[0] * zz) + _COS[1]) * zz + _COS[2]) * zz + _COS[3]) * zz + _COS[4]) * zz + _COS[5])
        r = np.where((j == 1) | (j == 2), ps, pc)
        r = np.where(sign, -r, r)
        return np.where(bad, np.nan, r)


def expf(x):
    with np.errstate(over="ignore"):
        return exp64(np.asarray(x, F).astype(D)).astype(F)


def cosf(x):
    return cos64(np.asarray(x, F).astype(D)).astype(F)


# ---- helpers ------------------------------------------------------------------------------------------------------------------
def to_int_bits(v):
    """Go's float32 -> uint8 / uint32 conversion as amd64 does it: int64 truncation, low bits kept; NaN and |v| >= 2^63 -> 0."""
    v = np.asarray(v, F)
    with np.errstate(all="ignore"):
        ok = np.abs(v) < F(2.0 ** 63)  # (False for NaN)
        return np.where(ok, np.where(ok, v, F(0)).astype(np.int64), 0).astype(np.uint64) & np.uint64(0xffffffff)


def clamp(v, lo, hi):
    v = np.asarray(v, F)
    return np.where(v < lo, F(lo), np.where(v > hi, F(hi), v)).astype(F)  # a NaN stays NaN


def interp(x, y, a):
    return (x + a * (y - x)).astype(F)


def fmod2(x):
    """math32.Mod(x, 2): exact, sign of x."""
    ax = np.abs(x)
    return np.copysign(ax - F(2) * np.floor(ax * F(0.5)), x).astype(F)


def _pack(r, g, b):
    r, g, b = (np.asarray(c, np.uint64) & np.uint64(0xff) for c in (r, g, b))
    return np.stack([r, g, b, np.full(r.shape, 255, np.uint64)], -1).astype(np.uint8)


# ---- the conversions ------------------------------------------------------------------------------------------------------------
def iq(d, length):
    d0 = np.asarray(d, F)
    with np.errstate(all="ignore"):
        inv = F(1) / F(length)
        d = (d0 * inv).astype(F)
        pos = d > 0
        cx, cy, cz = (np.where(pos, F(a), F(b)).astype(F) for a, b in ((0.9, 0.65), (0.6, 0.85), (0.3, 1.0)))
        a = np.abs(d)
        s1 = (F(1) - expf((F(-6) * a).astype(F))).astype(F)
        cx, cy, cz = s1 * cx, s1 * cy, s1 * cz
        s2 = (F(0.8) + F(0.2) * cosf((F(150) * d).astype(F))).astype(F)
        cx, cy, cz = s2 * cx, s2 * cy, s2 * cz
        t = clamp((a / F(0.01)).astype(F), 0, 1)
        mx = (F(1) - (t * t) * (F(3) - F(2) * t)).astype(F)
        cx, cy, cz = interp(cx, F(1), mx), interp(cy, F(1), mx), interp(cz, F(1), mx)
        out = _pack(to_int_bits(cx * F(255)), to_int_bits(cy * F(255)), to_int_bits(cz * F(255)))
    out[np.isnan(d0)] = (255, 0, 0, 255)
    return out


def rgb_to_hsv(r, g, b):
    """rgbToHSV (color.go:178-200), float32 scalars."""
    r, g, b = F(r), F(g), F(b)
    xmax, xmin = max(r, g, b), min(r, g, b)
    c = F(xmax - xmin)
    v = xmax
    h = F(0)
    if c == 0:
        h = F(0)
    elif v == r:
        h = F((g - b) / F(c * F(6)))
    elif v == g:
        h = F(K1_3 + F((b - r) / F(c * F(6))))
    elif v == b:
        h = F(K2_3 + F((r - g) / F(c * F(6))))
    if h < 0:
        h = F(h + F(1))
    s = F(c / xmax) if xmax > 0 else F(0)
    return h, s, v


def color_to_hsv(c):
    """colorToHSV of an image.RGBA colour's bytes (color.go:124-127)."""
    return rgb_to_hsv(F(F(c[0]) / F(255)), F(F(c[1]) / F(255)), F(F(c[2]) / F(255)))


def hsv_to_rgb(h, s, v):
    """hsvToRGB (color.go:150-174), float32 arrays; an h outside [0, 1] (NaN included) gives (0, 0, 0) + m."""
    with np.errstate(all="ignore"):
        c = (s * v).astype(F)
        x = (c * (F(1) - np.abs(fmod2((h * F(6)).astype(F)) - F(1)))).astype(F)
        m = (v - c).astype(F)
        z = np.zeros_like(c)
        conds = [(h >= 0) & (h <= K1_6), (h > K1_6) & (h <= K1_3), (h > K1_3) & (h <= K3_6), (h > K3_6) & (h <= K2_3),
                 (h > K2_3) & (h <= K5_6), (h > K5_6) & (h <= F(1))]
        r = np.select(conds, [c, x, z, z, x, c], z)
        g = np.select(conds, [x, c, c, x, z, z], z)
        b = np.select(conds, [z, z, x, c, c, x], z)
        return (r + m).astype(F), (g + m).astype(F), (b + m).astype(F)


def gradient(d, length, c0, c1):
    """ColorConversionLinearGradient for a pair other than black -> white."""
    d = np.asarray(d, F)
    h0, s0, v0 = color_to_hsv(c0)
    h1, s1, v1 = color_to_hsv(c1)
    if F(h1 - h0) > F(0.5):
        h0 = F(h0 + F(1))
    elif F(h1 - h0) < F(-0.5):
        h1 = F(h1 + F(1))
    with np.errstate(all="ignore"):
        blend = (d / F(length) + F(0.5)).astype(F)
        h, s, v = interp(h0, h1, blend), interp(s0, s1, blend), interp(v0, v1, blend)
        r, g, b = hsv_to_rgb(h, s, v)
        out = _pack(to_int_bits(clamp(r, 0, 1) * F(255)), to_int_bits(clamp(g, 0, 1) * F(255)), to_int_bits(clamp(b, 0, 1) * F(255)))
        out[blend <= 0] = np.asarray(c0, np.uint8)
        out[blend >= 1] = np.asarray(c1, np.uint8)
    return out


def bw(d, length):
    """blackAndWhiteLinearSmooth / blackAndWhiteNoSmoothing."""
    d = np.asarray(d, F)
    out = np.empty(d.shape + (4,), np.uint8)
    out[...] = 255
    with np.errstate(all="ignore"):
        if F(length) == 0:
            out[d < 0, :3] = 0
            return out
        blend = (d / F(length) + F(0.5)).astype(F)
        y = (to_int_bits(clamp(blend, 0, 1) * F(255)) & np.uint64(0xff)).astype(np.uint8)
        out[..., 0], out[..., 1], out[..., 2] = y, y, y
        out[blend <= 0, :3] = 0
        out[blend >= 1, :3] = 255
    return out


def default(d):
    """ImageRendererSDF2's own default (gsdf_hip_image2's bytes)."""
    d = np.asarray(d, F)
    out = np.zeros(d.shape + (4,), np.uint8)
    out[..., 3] = 255
    with np.errstate(all="ignore"):
        out[d > 0, :3] = 255
    out[~np.isfinite(d)] = (255, 0, 0, 255)
    return out


def convert(d, conv):
    """The bytes of a GsdfColor2 (gsdf_amd.hip) for the distances d: (..., 4) uint8."""
    kind, length = int(conv.kind), F(conv.length)
    if kind == IQ:
        return iq(d, length)
    if kind == GRADIENT:
        return gradient(d, length, tuple(conv.c0), tuple(conv.c1))
    if kind == BW_SMOOTH:
        return bw(d, length)
    return default(d)


# ---- RenderPNGFile's geometry ---------------------------------------------------------------------------------------------------
def hypot32(p, q):
    """math32.Hypot (scaffold/ms.hpp: hypotf32)."""
    p, q = abs(F(p)), abs(F(q))
    if math.isinf(p) or math.isinf(q):
        return F(np.inf)
    if p < q:
        p, q = q, p
    if p == 0:
        return F(0)
    q = F(q / p)
    return F(p * F(np.sqrt(F(F(1) + F(q * q)))))


def picture_size(bb, pic_height):
    """gsdfaux.go:271-274: width from the float32 size of the bounds, in float64, truncated."""
    bb = np.asarray(bb, F)
    szx, szy = F(bb[3] - bb[0]), F(bb[4] - bb[1])
    return int(float(pic_height) / float(szy) * float(szx))


def iq_default_length(bb):
    """RenderPNGFile's nil conversion: ColorConversionInigoQuilez(bb.Diagonal() / 3)."""
    bb = np.asarray(bb, F)
    return F(hypot32(F(bb[3] - bb[0]), F(bb[4] - bb[1])) / F(3))


def lattice(bb, w, h):
    """gsdf_hip_image2's pixel positions (image.go:82-88): (h*w, 2) float32, row 0 at the top."""
    bb = np.asarray(bb, F)
    dx, dy = F(F(bb[3] - bb[0]) / F(w)), F(F(bb[4] - bb[1]) / F(h))
    xmin, ymax = F(bb[0] + F(dx / F(2))), bb[4]
    pos = np.empty((h, w, 2), F)
    pos[..., 0] = (np.arange(w, dtype=F) * dx + xmin).astype(F)[None, :]
    pos[..., 1] = (ymax - np.arange(h, dtype=F) * dy).astype(F)[:, None]
    return pos.reshape(-1, 2)
