"""Arguments for holding a math routine to a reference over EVERY float32 magnitude (tests/test_oracle_math.py: the oracle's
restatement against float64; tests/test_gpu_math.py: the device's routes against the oracle's).

structured(): every binade (biased exponents 1..254) x 7 mantissas x both signs, the zeros, subnormals. The mantissas are the ends of
the binade, its middle, a third, two thirds and the neighbours of the ends: what a table, a range test or a rounding goes wrong on.
breakpoints(): the values at which the routes themselves change course, each with its float32 neighbours."""
import math

import numpy as np

F = np.float32
MANTISSAS = (0x000000, 0x000001, 0x2AAAAB, 0x400000, 0x555555, 0x7FFFFE, 0x7FFFFF)
SUBNORMALS = (0x000001, 0x000002, 0x400000, 0x7FFFFF)


def _bits(u):
    return np.asarray(u, np.uint32).view(np.float32)


def structured():
    e = np.arange(1, 255, dtype=np.uint32)[:, None] << 23
    pos = (e | np.asarray(MANTISSAS, np.uint32)[None, :]).ravel()
    pos = np.concatenate([pos, np.asarray((0,) + SUBNORMALS, np.uint32)])
    return _bits(np.concatenate([pos, pos | np.uint32(0x80000000)]))


def around(v, n=2):
    """float32(v) and its n neighbours on either side, both signs."""
    c = np.asarray([v], np.float32).view(np.uint32)[0].astype(np.int64)
    u = (c + np.arange(-n, n + 1)).astype(np.uint32)
    return _bits(np.concatenate([u, u | np.uint32(0x80000000)]))


def breakpoints():
    """The routes' own breakpoints: atan's range ends 0.66 and tan(3 pi / 8), acos' 0.7 and 1, the octant boundaries k pi / 4 to the
    last bit, cossin_fast's 2^20, the reduction's 2^29, sqrt_k's 2^-96, div_uniform_k's 2^+-90, atan2_fast's 2^+-100, recip_for's
    2^+-30."""
    v = [0.66, math.tan(3 * math.pi / 8), 0.7, 1.0, 2.0 ** 20, 2.0 ** 29, 2.0 ** -96, 2.0 ** 90, 2.0 ** -90, 2.0 ** 100, 2.0 ** -100,
         2.0 ** 30, 2.0 ** -30, 0.5, 2.0 ** -126]
    v += [k * math.pi / 4 for k in range(1, 65)] + [k * math.pi / 4 for k in (1 << 10, 1 << 16, (1 << 20) + 1, (1 << 24) + 3, (1 << 27) + 5)]
    return np.concatenate([around(x) for x in v])


def random_bits(n, seed):
    """n finite float32 values, uniform over the bit patterns (so over the exponents)."""
    u = np.random.default_rng(seed).integers(0, 1 << 32, int(n * 1.02) + 16, dtype=np.uint64).astype(np.uint32)
    x = _bits(u)
    return np.ascontiguousarray(x[np.isfinite(x)][:n])


def one_operand(n_random=90000, seed=11):
    return np.ascontiguousarray(np.concatenate([structured(), breakpoints(), random_bits(n_random, seed)]))


def two_operands(n_random=30000, seed=12):
    """(x, y): the structured set against 16 rotations of itself (every pairing of magnitudes a fixed stride apart, up to the whole
    exponent range), |y| == |x| with every sign, ratios at atan's breakpoints to the last bit, one operand zero, random pairs, and
    random pairs whose exponents lie within 2 of each other (where hypot and the octant selection decide)."""
    s = structured()
    xs, ys = [], []
    for r in (0, 1, 2, 3, 5, 7, 14, 70, 140, 350, 700, 901, 1400, 1787, 2500, 3300):
        xs.append(s)
        ys.append(np.roll(s, r))
    xs += [s, s]
    ys += [-s, np.zeros_like(s)]
    for ratio in (0.66, math.tan(3 * math.pi / 8), 1.0, math.tan(math.pi / 8)):
        for d in range(-2, 3):
            with np.errstate(over="ignore"):
                y = (s.astype(np.float64) * ratio).astype(np.float32)
            y = (y.view(np.uint32).astype(np.int64) + d).astype(np.uint32).view(np.float32)
            ok = np.isfinite(y)
            xs.append(s[ok])
            ys.append(y[ok])
    a, b = random_bits(n_random, seed), random_bits(n_random, seed + 1)
    xs.append(a)
    ys.append(b)
    rng = np.random.default_rng(seed + 2)
    eb = ((a.view(np.uint32) >> 23) & 0xFF).astype(np.int64)
    ec = np.clip(eb + rng.integers(-2, 3, len(a)), 1, 254).astype(np.uint32)
    c = ((b.view(np.uint32) & np.uint32(0x807FFFFF)) | (ec << 23)).view(np.float32)
    xs.append(a)
    ys.append(c)
    x, y = np.concatenate(xs), np.concatenate(ys)
    return np.ascontiguousarray(np.concatenate([x, y])), np.ascontiguousarray(np.concatenate([y, x]))   # both orders
