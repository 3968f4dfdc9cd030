"""The device's math routes against the oracle's restatement of the reference's math package, function by function.

The other device selftests (tests/test_gpu_eval.py) hold each SHORT route to the device's own long route; inside trees both meet the
oracle at arguments of order 1 only. Here every route is run on its own (gsdf_hip_selftest_math: one value per lane) over every
float32 magnitude -- tests/math_points.py: all binades, both signs, subnormals, zeros, the routes' own breakpoints to the last bit,
random bit patterns -- and compared with oracle.math_apply bit for bit. The stated domain, each line with its reason:

  finite inputs            the evaluators take finite positions; Inf / NaN special cases are not reproduced (dev_math.h's header)
  sin, cos: |x| < 2^29     beyond, Go's math.Sin / Cos reduce by Payne-Hanek (sin.go: reduceThreshold); device and oracle keep Cody-Waite
  Sincos:   |x| < 2^29     math32.Sincos has no second reduction at all; past 2^32 pi / 4 its octant does not fit the integer it is
                           converted to, which C (the oracle) and the device define differently
  acos: |x| <= 1           NaN beyond, on both sides
  pow13: x >= 0, 1 ulp     exp(log(x) / 3) through two different libraries (ocml on the device, libm in the oracle)
  min, max: no NaN         v_min_f32 / v_max_f32 drop a NaN, math32.Min / Max hand it on (tests/test_gpu_nan.py)
  sqrt, division           IEEE: against numpy's float32 sqrt and division

The arrays keep the structured set in magnitude order (whole waves in one regime: both sides of every vote) and the random patterns
mixed (lanes of one wave in different regimes: the vote fails, the fall-back runs).

Time, one run on one MI355X machine: this file 2.8 s (27 cases, 0.01-0.16 s each: one launch over 5e4 to 4e5 values and the oracle's
loop over the same), of which 1.5 s load the libraries; beside it the rest of the GPU suite 765 s (444 cases; tests/test_gpu_scale.py
has the split from the parent commit's suite).
"""
import numpy as np
import pytest

import math_points as MP
from oracle.oracle import math_apply as ref_apply
from test_oracle_math import TRIG_LIMIT, ulps

pytestmark = pytest.mark.gpu


def _diff(got, want):
    return (got.view(np.uint32) != want.view(np.uint32)) & ~(np.isnan(got) & np.isnan(want))


def _report(what, x, y, got, want, bad):
    k = np.flatnonzero(bad)
    print(what, "values", len(x), "mismatches", len(k))
    for i in k[:6]:
        print("   x=%r (0x%08x) y=%r got=%r want=%r" % (float(x[i]), int(x[i:i + 1].view(np.uint32)[0]), None if y is None else float(y[i]), float(got[i]), float(want[i])))
    return len(k)


ONE = [  # device route, oracle function, domain
    ("sin", "sin", lambda x: np.abs(x) < TRIG_LIMIT),
    ("cos", "cos", lambda x: np.abs(x) < TRIG_LIMIT),
    ("cossin_s", "sin", lambda x: np.abs(x) < TRIG_LIMIT),
    ("cossin_c", "cos", lambda x: np.abs(x) < TRIG_LIMIT),
    ("sincos_s", "sincos_s", lambda x: np.abs(x) < TRIG_LIMIT),
    ("sincos_c", "sincos_c", lambda x: np.abs(x) < TRIG_LIMIT),
    ("acos", "acos", lambda x: np.abs(x) <= 1),
    ("cbrt", "cbrt", lambda x: np.isfinite(x)),
    ("round", "round", lambda x: np.isfinite(x)),
    ("floor", "floor", lambda x: np.isfinite(x)),
]


@pytest.mark.parametrize("route,fn,domain", ONE, ids=[r[0] for r in ONE])
def test_one_operand_routes_equal_the_oracle(gpu, route, fn, domain):
    x = MP.one_operand()
    x = x[domain(x)]
    assert len(x) > 40000
    got, want = gpu.math_apply(route, x), ref_apply(fn, x)
    assert _report(route, x, None, got, want, _diff(got, want)) == 0


TWO = [("hypot", "hypot"), ("atan2_ref", "atan2"), ("atan2", "atan2"), ("min", "min"), ("max", "max")]


@pytest.mark.parametrize("route,fn", TWO, ids=[r[0] for r in TWO])
def test_two_operand_routes_equal_the_oracle(gpu, route, fn):
    x, y = MP.two_operands()
    assert np.isfinite(x).all() and np.isfinite(y).all() and len(x) > 100000
    got, want = gpu.math_apply(route, x, y), ref_apply(fn, x, y)
    assert _report(route, x, y, got, want, _diff(got, want)) == 0


def test_pow13_within_one_ulp(gpu):
    x = MP.one_operand()
    x = x[(x >= 0) & ~np.signbit(x)]
    got, want = gpu.math_apply("pow13", x), ref_apply("pow13", x)
    assert np.isfinite(got).all() and np.isfinite(want).all()
    u = ulps(got, want)
    print("pow13 values", len(x), "largest difference", int(u.max()), "ulp; differing", int((u > 0).sum()))
    assert u.max() <= 1


def test_sqrt_is_ieee(gpu):
    x = MP.one_operand()
    got = gpu.math_apply("sqrt", x)
    with np.errstate(invalid="ignore"):
        want = np.sqrt(x)                                    # float32 in, float32 out: correctly rounded; NaN below zero on both sides
    assert _report("sqrt", x, None, got, want, _diff(got, want)) == 0


# divisors: inside [2^-30, 2^30] the host hands the node RN(1 / d) and the wave takes the exact-reciprocal form where every numerator
# is in [2^-90, 2^90]; outside (and for a wave with one numerator out of range, or a zero) the IEEE division runs. The same bits.
DIVISORS = [3.0, 0.1, -7.25, 2.0 ** 30, 2.0 ** -30, float(np.nextafter(np.float32(2.0 ** 30), np.float32(np.inf))),
            float(np.nextafter(np.float32(2.0 ** -30), np.float32(0))), 3.0e20, -1.7e-23, 2.0 ** -126]


@pytest.mark.parametrize("d", DIVISORS, ids=["%g" % d for d in DIVISORS])
def test_division_by_a_uniform_divisor_is_ieee(gpu, d):
    x = MP.one_operand()
    got = gpu.math_apply("div", x, divisor=d)
    with np.errstate(over="ignore", under="ignore"):
        want = (x / np.float32(d)).astype(np.float32)
    assert _report("div by %g" % d, x, None, got, want, _diff(got, want)) == 0
