"""The two identities behind the face form of the box-like primitives (interp.h: face2_k / face3_k), on the host.

    u <= 0 or v <= 0:                      min(0, max(u, v)) + hypot(max(u, 0), max(v, 0))             ==  max(u, v) + 0
    at least two of qx, qy, qz <= 0:       min(max(qx, max(qy, qz)), 0) + norm3(max(qx, 0), max(qy, 0), max(qz, 0))
                                                                                                       ==  max(qx, max(qy, qz)) + 0

bit for bit (NaN for NaN), in both operand orders the ops use -- min(0, m) / min(m, 0), max(0, x) / max(x, 0), in + h / h + in -- over
every combination of +-0, +-subnormal, +-FLT_MIN, +-1, +-FLT_MAX, +-Inf, +-NaN and over random bit patterns. hypot is the oracle's
math32.Hypot; min / max are taken
  * from the oracle's math export (Go: math.Min(+0, -0) = -0, math.Max(+0, -0) = +0, NaN propagates),
  * by the other zero-sign conventions a min / max may follow -- of two zeros the first operand, or the second -- each with NaN
    propagated and with NaN dropped (v_min_f32 / v_max_f32 return the other operand).
The requirement is 0 mismatches.
"""
import numpy as np
import pytest

from oracle import oracle

from face_points import F, grid, random_bits, same

ZERO = F(0.0)


def _go():
    return (lambda a, b: oracle.math_apply("min", a, b)), (lambda a, b: oracle.math_apply("max", a, b))


def _emulated(first_of_zeros, drop_nan):
    def pick(a, b, less):
        a, b = np.broadcast_arrays(np.asarray(a, F), np.asarray(b, F))
        with np.errstate(invalid="ignore"):
            r = np.where(less(a, b), a, b)
            zeros = (a == 0) & (b == 0)
        r = np.where(zeros, a if first_of_zeros else b, r)
        na, nb = np.isnan(a), np.isnan(b)
        if drop_nan:
            r = np.where(na, b, np.where(nb, a, r))
        else:
            r = np.where(na | nb, F(np.nan), r)
        return np.ascontiguousarray(r, F)
    return (lambda a, b: pick(a, b, np.less)), (lambda a, b: pick(a, b, np.greater))


CONVENTIONS = {"go": _go, "first-zero": lambda: _emulated(True, False), "second-zero": lambda: _emulated(False, False),
               "first-zero-drop-nan": lambda: _emulated(True, True), "second-zero-drop-nan": lambda: _emulated(False, True)}


def _hyp(a, b):
    return oracle.math_apply("hypot", a, b)


def _add(a, b):
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.asarray(a, F) + np.asarray(b, F)).astype(F)


def _operands(terms):
    rng = np.random.default_rng(20 + terms)
    parts = [grid(terms), random_bits(rng, 1 << 20, terms)]
    # random signs and magnitudes of order 1 as well: random bit patterns seldom sit close to each other
    parts.append([(rng.random(1 << 18, F) * 4 - 2).astype(F) for _ in range(terms)])
    return [np.concatenate([p[t] for p in parts]) for t in range(terms)]


@pytest.mark.parametrize("conv", list(CONVENTIONS))
def test_two_terms(conv):
    mn, mx = CONVENTIONS[conv]()
    u, v = _operands(2)
    with np.errstate(invalid="ignore"):
        ok = (u <= 0) | (v <= 0)
    assert ok.sum() > len(u) // 2
    u, v = u[ok], v[ok]
    zero = np.zeros_like(u)
    m = mx(u, v)
    new = _add(m, zero)
    # D_CYL0 / D_RECT2D / D_EXTRUDE_POST: min(0, m), max(0, x) or max(x, 0); D_CYLR / D_HEX: min(m, 0), max(x, 0); sums in either order
    for inn, ax, ay in ((mn(zero, m), mx(zero, u), mx(zero, v)), (mn(m, zero), mx(u, zero), mx(v, zero)), (mn(zero, m), mx(u, zero), mx(v, zero))):
        h = _hyp(ax, ay)
        for old in (_add(inn, h), _add(h, inn)):
            bad = np.flatnonzero(~same(old, new))
            assert bad.size == 0, (conv, bad.size, u[bad[:4]].tolist(), v[bad[:4]].tolist())
    # what the + 0 is for: without it the zero cases differ under at least one convention (stated once, not required per convention)
    if conv == "go":
        assert (~same(_add(mn(zero, m), _hyp(mx(zero, u), mx(zero, v))), m)).any()


@pytest.mark.parametrize("conv", list(CONVENTIONS))
def test_three_terms(conv):
    mn, mx = CONVENTIONS[conv]()
    qx, qy, qz = _operands(3)
    with np.errstate(invalid="ignore"):
        ok = ((qx <= 0).astype(int) + (qy <= 0) + (qz <= 0)) >= 2
    assert ok.sum() > len(qx) // 4
    qx, qy, qz = qx[ok], qy[ok], qz[ok]
    zero = np.zeros_like(qx)
    m = mx(qx, mx(qy, qz))
    new = _add(m, zero)
    for inn, ax, ay, az in ((mn(m, zero), mx(qx, zero), mx(qy, zero), mx(qz, zero)), (mn(zero, m), mx(zero, qx), mx(zero, qy), mx(zero, qz))):
        n3 = _hyp(ax, _hyp(ay, az))  # ms3.Norm = hypot(x, hypot(y, z))
        for old in (_add(n3, inn), _add(inn, n3)):
            bad = np.flatnonzero(~same(old, new))
            assert bad.size == 0, (conv, bad.size, qx[bad[:4]].tolist(), qy[bad[:4]].tolist(), qz[bad[:4]].tolist())
