"""Mass and section properties without a device: the new symbols and struct layouts, the argument errors that are decided before a
device is touched, gsdf_hip_inertia_principal against the twin (tests/massref.py) and numpy.linalg.eigh, the twin against closed
forms, and the host-side arithmetic (gsdf_amd/csrc/mass_host.h, abi_mass.cpp) as a stand-alone program under AddressSanitizer and
UBSan.

Bounds used below (derived from the contract in include/gsdf_hip.h, not measured). A second-moment term of a mesh is
(det * bracket) / 120: fewer than 32 float64 operations, each rounding at most 2^-53 of an intermediate value, and every
intermediate value of the chain is below the bound of the term's own chain, 72 2^(5e) before the division; so a term is off by less
than 32 * 72 / 120 * 2^(5e-53) < 2^(5e-48). Its quantisation adds 2^(5e-63), the one conversion of the sum 2^-53 of a sum below
n_tris 2^(5e). Together below n_tris 2^(5e-47): the tests use n_tris 2^(5e-44), the lower degrees n_tris 2^(3e-44) and n_tris 2^(4e-44)
by the same count. Loops likewise: n 2^(3e-44) for the first moments, n 2^(4e-44) for the second."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import massref as M
import toporef as T
from gsdf_amd import hip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gsdf_amd", "csrc")
NEW = ["gsdf_hip_indexed_mass", "gsdf_hip_indexed_mass_ms", "gsdf_hip_inertia_principal", "gsdf_hip_contour_sections", "gsdf_hip_contour_sections_ms"]


def test_symbols_and_layouts():
    L = hip.lib()
    for name in NEW:
        assert name in hip.SYMBOLS and hasattr(L, name), name
    assert C.sizeof(hip.Mass) == 160 == hip.MASS_DTYPE.itemsize == M.MASS_DTYPE.itemsize
    assert [(f, getattr(hip.Mass, f).offset) for f, _ in hip.Mass._fields_] == [("volume", 0), ("first", 8), ("second", 32), ("centroid", 80), ("inertia", 104),
                                                                                 ("exponent", 152), ("label", 156)]
    assert [hip.MASS_DTYPE.fields[f][1] for f in hip.MASS_DTYPE.names] == [0, 8, 32, 80, 104, 152, 156] and hip.MASS_DTYPE == M.MASS_DTYPE
    assert C.sizeof(hip.Section) == 96 == hip.SECTION_DTYPE.itemsize == M.SECTION_DTYPE.itemsize
    assert [(f, getattr(hip.Section, f).offset) for f, _ in hip.Section._fields_] == [("area", 0), ("first", 8), ("second", 24), ("centroid", 48), ("central", 64),
                                                                                       ("n_verts", 88), ("layer_or_n_loops", 92)]
    assert [hip.SECTION_DTYPE.fields[f][1] for f in hip.SECTION_DTYPE.names] == [0, 8, 24, 48, 64, 88, 92] and hip.SECTION_DTYPE == M.SECTION_DTYPE
    hdr = open(os.path.join(ROOT, "include", "gsdf_hip.h")).read()
    assert 'GSDF_ABI_ASSERT(sizeof(gsdf_mass) == 160' in hdr and 'GSDF_ABI_ASSERT(sizeof(gsdf_section) == 96' in hdr
    assert L.gsdf_hip_indexed_mass(None, None, None, 0, None) == -3 and L.gsdf_hip_contour_sections(None, None, None) == -3
    assert L.gsdf_hip_indexed_mass_ms() == 0.0 and L.gsdf_hip_contour_sections_ms() == 0.0     # after a call that failed


def test_argument_errors_need_no_device():
    """Decided from the arguments alone, before the handle is looked at: `handle` below is an address that is never read."""
    L = hip.lib()
    handle, n, rec = C.c_void_p(64), C.c_uint64(7), np.zeros(1, hip.MASS_DTYPE)
    assert L.gsdf_hip_indexed_mass(None, rec.ctypes.data, None, 0, None) == -3                                   # GSDF_ERR_BAD_ARGUMENT
    assert L.gsdf_hip_indexed_mass(handle, None, None, 0, None) == -3 and b"nothing asked for" in L.gsdf_hip_last_error()
    assert L.gsdf_hip_indexed_mass(handle, None, rec.ctypes.data, 1, None) == -3 and b"shells needs n" in L.gsdf_hip_last_error()
    assert L.gsdf_hip_indexed_mass(handle, rec.ctypes.data, rec.ctypes.data, 1, None) == -3 and n.value == 7
    assert L.gsdf_hip_contour_sections(None, None, None) == -3
    i6, m, ax = np.array([1, 2, 3, 0, 0, 0], np.float64), np.zeros(3), np.zeros(9)
    assert L.gsdf_hip_inertia_principal(None, m.ctypes.data, ax.ctypes.data) == -3
    assert L.gsdf_hip_inertia_principal(i6.ctypes.data, None, ax.ctypes.data) == -3 and L.gsdf_hip_inertia_principal(i6.ctypes.data, m.ctypes.data, None) == -3
    for k in range(6):
        for bad in (np.nan, np.inf, -np.inf):
            x = i6.copy()
            x[k] = bad
            assert L.gsdf_hip_inertia_principal(x.ctypes.data, m.ctypes.data, ax.ctypes.data) == -3 and b"NaN or infinite" in L.gsdf_hip_last_error()
            with pytest.raises(hip.HipError):
                hip.inertia_principal(x)


def test_the_examples_density_argument():
    """examples/render_ply.py --density: checked with the command line, before a device is needed."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("render_ply_mass", os.path.join(ROOT, "examples", "render_ply.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    assert mod.parse_args(["bolt"]).density == 1.0 and mod.parse_args(["bolt", "--report", "--density", "7.85"]).density == 7.85
    for bad in ("0", "-1", "nan", "inf"):
        with pytest.raises(SystemExit):
            mod.parse_args(["bolt", "--density", bad])


# ---- principal axes -------------------------------------------------------------------------------------------------------------------
def _tensors():
    """(name, the six entries, separated: the eigenvalues are distinct, so that eigh's eigenvectors are well defined)."""
    out = [("diagonal", [3.0, 1.0, 2.0, 0, 0, 0], True), ("sphere", [0.4, 0.4, 0.4, 0, 0, 0], False), ("two equal", [2.0, 5.0, 2.0, 0, 0, 0], False),
           ("two equal, rotated", [3.5, 3.5, 2.0, 1.5, 0, 0], False)]
    rng = np.random.default_rng(20)
    for k in range(20):
        q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
        lam = np.array([1.0, 4.0, 7.0]) + rng.random(3) * 2.0             # gaps of at least 1
        a = (q * lam) @ q.T
        out.append(("random %d" % k, [a[0, 0], a[1, 1], a[2, 2], a[0, 1], a[0, 2], a[1, 2]], True))
    return [(n, np.array(i6, np.float64), sep) for n, i6, sep in out]


def _full(i6):
    return np.array([[i6[0], i6[3], i6[4]], [i6[3], i6[1], i6[5]], [i6[4], i6[5], i6[2]]])


def test_principal_axes_have_the_twins_bytes():
    for name, i6, _ in _tensors():
        m, ax = hip.inertia_principal(i6)
        tm, tax = M.principal(i6)
        assert m.tobytes() == tm.tobytes() and ax.tobytes() == tax.tobytes(), (name, m, tm, ax, tax)
        m2, ax2 = hip.inertia_principal(_full(i6))
        assert m2.tobytes() == m.tobytes() and ax2.tobytes() == ax.tobytes()
    m, ax = hip.inertia_principal([3.0, 1.0, 2.0, 0, 0, 0])                # ascending, the stated signs, right-handed
    assert m.tolist() == [1, 2, 3] and ax.tolist() == [[0, 1, 0], [0, 0, 1], [1, 0, 0]]
    m, ax = hip.inertia_principal([0.4, 0.4, 0.4, 0, 0, 0])                # equal moments keep their order
    assert m.tolist() == [0.4] * 3 and ax.tolist() == np.eye(3).tolist()


def test_principal_axes_against_eigh():
    """Measured on these 24 tensors (the test prints the four figures): moments within 6.61e-16 of the largest moment of
    numpy.linalg.eigh's; axes of the 21 separated tensors (up to eigh's sign) within 7.77e-16 per component; residual |A x - m x|
    within 2.20e-16 of the largest moment and |X X^T - 1| within 1.33e-15 for all. The bound below is 4 x the largest of these,
    5.4e-15: far below the 1e-12 above which the stop rule would be wrong."""
    tol = 5.4e-15
    assert tol < 1e-12
    worst = [0.0, 0.0, 0.0, 0.0]
    for name, i6, separated in _tensors():
        a = _full(i6)
        m, ax = hip.inertia_principal(i6)
        w, v = np.linalg.eigh(a)
        big = np.abs(w).max()
        worst[0] = max(worst[0], np.abs(m - w).max() / big)
        worst[2] = max(worst[2], np.abs(a @ ax.T - ax.T * m).max() / big)
        worst[3] = max(worst[3], np.abs(ax @ ax.T - np.eye(3)).max())
        assert (np.diff(m) >= 0).all() and np.linalg.det(ax) > 0, name
        for k in range(2):
            assert ax[k][np.argmax(np.abs(ax[k]))] > 0, (name, ax)           # the stated sign
        if separated:
            for k in range(3):
                worst[1] = max(worst[1], np.abs(v[:, k] * np.sign(v[:, k] @ ax[k]) - ax[k]).max())
    print("moments %.2e axes %.2e residual %.2e orthonormal %.2e" % tuple(worst))
    assert max(worst) <= tol, worst


# ---- the twin against closed forms -----------------------------------------------------------------------------------------------------
def _tensor_of(rec):
    return np.array(rec["inertia"], np.float64)


def test_box_away_from_the_origin_and_translated():
    lo, hi = (1.5, 2.25, -0.5), (3.0, 4.0, 1.25)                             # dyadic corners
    v, i = M.box(lo, hi)
    tot, shells, _ = M.mesh_mass(v, i)
    e = int(tot["exponent"])
    assert e == 3 and len(i) == 12 and len(shells) == 1 and shells[0].tobytes()[:152] == tot.tobytes()[:152]
    vol, first, second = M.box_moments(lo, hi)
    bound = 12 * 2.0 ** (5 * e - 44)                                         # (module docstring)
    assert abs(tot["volume"] - vol) <= 12 * 2.0 ** (3 * e - 44) and np.abs(tot["first"] - first).max() <= 12 * 2.0 ** (4 * e - 44)
    assert np.abs(tot["second"] - second).max() <= bound, (tot["second"], second)
    d = np.subtract(hi, lo)
    want = vol / 12 * np.array([d[1] ** 2 + d[2] ** 2, d[0] ** 2 + d[2] ** 2, d[0] ** 2 + d[1] ** 2, 0, 0, 0])
    assert np.abs(_tensor_of(tot) - want).max() <= 2 * bound
    # parallel axes: the same box somewhere else has the same central tensor, within the bound at ITS exponent
    shift = np.array([16.5, -9.25, 4.0])
    v2 = (v.astype(np.float64) + shift).astype(np.float32)
    assert (v2.astype(np.float64) == v.astype(np.float64) + shift).all()
    tot2, _, _ = M.mesh_mass(v2, i)
    e2 = int(tot2["exponent"])
    assert e2 == 5 and np.abs(_tensor_of(tot2) - want).max() <= 2 * 12 * 2.0 ** (5 * e2 - 44)
    assert np.abs(tot2["centroid"] - (np.add(lo, hi) / 2 + shift)).max() <= 12 * 2.0 ** (4 * e2 - 44)


def test_tetrahedron():
    tot, _, _ = M.mesh_mass(T.TET_V, T.TET_I)                                # a corner at the origin, legs 6
    bound = 4 * 2.0 ** (5 * 3 - 44)
    assert tot["exponent"] == 3 and tot["volume"] == 36 and np.abs(tot["centroid"] - 1.5).max() <= bound
    assert np.abs(tot["second"] - np.array([129.6] * 3 + [64.8] * 3)).max() <= bound
    assert np.abs(_tensor_of(tot) - np.array([97.2] * 3 + [16.2] * 3)).max() <= 4 * bound
    m, ax = hip.inertia_principal(tot["inertia"])                            # the (1, 1, 1) axis carries the largest moment, 97.2 + 2 * 16.2
    assert np.allclose(m, [81, 81, 129.6], rtol=0, atol=1e-12) and np.allclose(ax[2] * np.sign(ax[2][0]), np.ones(3) / np.sqrt(3), rtol=0, atol=1e-12)


def test_face_order_and_orientation():
    v, i = M.sphere(10, 16)
    assert len(i) == 288
    a, sa, ia = M.mesh_mass(v, i)
    perm = np.random.default_rng(4).permutation(len(i))
    b, sb, ib = M.mesh_mass(v, i[perm])
    assert ia == ib and a.tobytes() == b.tobytes() and sa.tobytes() == sb.tobytes()      # integer sums: no order
    assert abs(a["volume"] / (4 / 3 * np.pi) - 1) < 0.05 and np.allclose(a["inertia"][:3], 0.4 * a["volume"], rtol=0.05)
    # On a dyadic grid (multiples of 2^-6 below 1) every product and sum of a term is exact, so that swapping b and c negates the
    # term, and its quotient by 6, 24 or 120 rounds the same way for either sign: the inverted shell has the negated integers.
    vq = (np.rint(v.astype(np.float64) * 64) / 64).astype(np.float32)
    _, _, up = M.mesh_mass(vq, i)
    neg, _, down = M.mesh_mass(vq, i[:, [0, 2, 1]])
    assert down == [[-q for q in up[0]]] and neg["volume"] < 0 and (neg["second"][:3] < 0).all()
    # a cavity: the outer sphere and an inverted inner one are two shells; the mesh's integers are the sums of the shells'
    vi, ii = M.sphere(6, 8, 0.5)
    vq2 = (np.rint(vi.astype(np.float64) * 64) / 64).astype(np.float32)
    vv, jj = T.join((vq, i), (vq2, ii[:, [0, 2, 1]]))
    tot, shells, ints = M.mesh_mass(vv, jj)
    assert len(shells) == 2 and shells[1]["volume"] < 0 < tot["volume"] < shells[0]["volume"]
    assert tot.tobytes() == M.mass_record([ints[0][k] + ints[1][k] for k in range(10)], int(tot["exponent"]), M.TOTAL).tobytes()


def test_zero_volume_is_nan_not_a_division():
    v, i = M.box((0, 0, 0), (1, 1, 1))
    vv, jj = T.join((v, i), (v, i[:, [0, 2, 1]]))                            # a box and its inverse, apart as shells, cancelling as a mesh
    tot, shells, _ = M.mesh_mass(vv, jj)
    assert tot["volume"] == 0 and (tot["second"] == 0).all() and len(shells) == 2
    assert tot["centroid"].view(np.uint64).tolist() == [0x7ff8000000000000] * 3 and tot["inertia"].view(np.uint64).tolist() == [0x7ff8000000000000] * 6


def _rect(x0, y0, x1, y1, hole=False):
    p = [[x0, y0], [x1, y0], [x1, y1], [x0, y1]]
    return p[::-1] if hole else p


def _rect_moments(x0, y0, x1, y1):
    """area, first (x, y), second (xx, yy, xy) of an axis-aligned rectangle about the origin."""
    w, h = x1 - x0, y1 - y0
    return np.array([w * h, (x1 ** 2 - x0 ** 2) / 2 * h, (y1 ** 2 - y0 ** 2) / 2 * w, (x1 ** 3 - x0 ** 3) / 3 * h, (y1 ** 3 - y0 ** 3) / 3 * w,
                     (x1 ** 2 - x0 ** 2) * (y1 ** 2 - y0 ** 2) / 4])


def _check_section(rec, want, n, e):
    got = np.concatenate([[rec["area"]], rec["first"], rec["second"]])
    bounds = np.array([n * 2.0 ** (2 * e - 44)] + [n * 2.0 ** (3 * e - 44)] * 2 + [n * 2.0 ** (4 * e - 44)] * 3)      # (module docstring)
    assert (np.abs(got - want) <= bounds).all(), (got, want)
    a, fx, fy, xx, yy, xy = want
    assert np.abs(rec["centroid"] - [fx / a, fy / a]).max() <= 4 * bounds[1] / abs(a)
    assert np.abs(rec["central"] - [xx - fx * fx / a, yy - fy * fy / a, xy - fx * fy / a]).max() <= 4 * bounds[3]


def test_sections_of_a_rectangle_a_frame_and_an_l():
    outer, inner = (1.5, -2.25, 6.0, 3.5), (2.0, -1.0, 4.5, 0.75)            # dyadic
    xy = np.array(_rect(*outer) + _rect(*inner, hole=True), np.float32)
    loops, layers, ints = M.sections(xy, [0, 4, 8], [0, 0], 1)
    e = M.loop_exponent(xy)
    assert e == 3
    _check_section(loops[0], _rect_moments(*outer), 4, e)
    _check_section(loops[1], -_rect_moments(*inner), 4, e)
    _check_section(layers[0], _rect_moments(*outer) - _rect_moments(*inner), 8, e)          # the material: holes are negative
    assert layers[0]["n_verts"] == 8 and layers[0]["layer_or_n_loops"] == 2 and loops[1]["layer_or_n_loops"] == 0
    assert layers[0].tobytes() == M.section_record([ints[0][k] + ints[1][k] for k in range(6)], e, 8, 2).tobytes()
    # the same two loops in two layers; a third layer without a loop: NaN centroid, sums 0
    l2, y2, _ = M.sections(xy, [0, 4, 8], [0, 1], 3)
    assert y2[0].tobytes()[:88] == loops[0].tobytes()[:88] and y2[1].tobytes()[:88] == loops[1].tobytes()[:88]
    assert y2[2]["area"] == 0 and y2[2]["centroid"].view(np.uint64).tolist() == [0x7ff8000000000000] * 2 and y2[2]["layer_or_n_loops"] == 0
    # an L: the rectangle (0, 0) .. (4, 1) and on it (0, 1) .. (1.5, 3.25), counter-clockwise, somewhere in the plane
    off = np.array([-7.5, 2.25])
    l_xy = (np.array([[0, 0], [4, 0], [4, 1], [1.5, 1], [1.5, 3.25], [0, 3.25]]) + off).astype(np.float32)
    ll, _, _ = M.sections(l_xy, [0, 6], None, 1)
    want = _rect_moments(-7.5, 2.25, -3.5, 3.25) + _rect_moments(-7.5, 3.25, -6.0, 5.5)
    _check_section(ll[0], want, 6, M.loop_exponent(l_xy))
    # a vertex order that starts elsewhere on the loop: the same integers
    assert M.loop_ints(np.roll(l_xy, 2, axis=0), [0, 6])[1] == M.loop_ints(l_xy, [0, 6])[1]


# ---- the host arithmetic as a stand-alone program under the sanitisers -------------------------------------------------------------------
PROGRAM = r'''
#include <cstdio>
#include <cstring>
#include <limits>
#include <string>
#include "mass_host.h"

static std::string g_text;
int fail(int code, const std::string& msg) { g_text = msg; return code; }   // what abi_mass.cpp imports (the library's: abi_host.cpp)

static void hex(const char* what, const double* d, int n) {
  std::printf("%s", what);
  for (int i = 0; i < n; i++) { unsigned long long u; std::memcpy(&u, d + i, 8); std::printf(" %016llx", u); }
  std::printf("\n");
}
static __int128 big(long long hi, unsigned long long lo) { return (__int128)hi * ((__int128)1 << 64) + (__int128)lo; }

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  double m[3], ax[9];
  const double t[4][6] = {{3, 1, 2, 0, 0, 0}, {0.4, 0.4, 0.4, 0, 0, 0}, {3.5, 3.5, 2.0, 1.5, 0, 0}, {97.2, 97.2, 97.2, 16.2, 16.2, 16.2}};
  for (int k = 0; k < 4; k++) {
    if (gsdf_hip_inertia_principal(t[k], m, ax) != GSDF_OK) return 1;
    hex("moments", m, 3);
    hex("axes", ax, 9);
  }
  // tiny and huge entries, an off-diagonal entry that is negligible beside one neighbour only, zeros
  const double odd[4][6] = {{1e-300, 2e-300, 3e-300, 1e-301, -1e-301, 5e-302}, {1e300, 2e300, 3e300, 1e299, -1e299, 5e298}, {0, 1, 1, 1e-200, 0, 0.5}, {0, 0, 0, 0, 0, 0}};
  for (int k = 0; k < 4; k++)
    if (gsdf_hip_inertia_principal(odd[k], m, ax) != GSDF_OK) return 2;
  double bad[6] = {1, 2, 3, 0, 0, 0};
  if (gsdf_hip_inertia_principal(nullptr, m, ax) != GSDF_ERR_BAD_ARGUMENT || gsdf_hip_inertia_principal(bad, nullptr, ax) != GSDF_ERR_BAD_ARGUMENT ||
      gsdf_hip_inertia_principal(bad, m, nullptr) != GSDF_ERR_BAD_ARGUMENT) return 3;
  for (int k = 0; k < 6; k++) {
    bad[k] = k % 2 ? nan : -inf;
    if (gsdf_hip_inertia_principal(bad, m, ax) != GSDF_ERR_BAD_ARGUMENT || g_text.find("NaN") == std::string::npos) return 4;
    bad[k] = 1;
  }
  // the conversions: integers that stand for simple values, a zero volume, the largest sums a handle can reach at e = -125, large ones at e = 128
  gsdf_mass rec;
  const __int128 cube[10] = {big(0, 1ull << 59), big(0, 1ull << 57), big(0, 1ull << 57), big(0, 1ull << 57), big(0, 3ull << 55), big(0, 3ull << 55), big(0, 3ull << 55),
                             big(0, 1ull << 55), big(0, 1ull << 55), big(0, 1ull << 55)};
  mass::fill_mass(&rec, cube, 1, 7u);
  hex("mass", &rec.volume, 19);
  if (rec.exponent != 1 || rec.label != 7u) return 5;
  __int128 zero[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  mass::fill_mass(&rec, zero, -125, 0xffffffffu);
  hex("mass", &rec.volume, 19);
  __int128 top[10], mid[10];
  for (int k = 0; k < 10; k++) {
    top[k] = (k % 2 ? -1 : 1) * big(1ll << 29, 12345ull + (unsigned long long)k);   // about 2^93: 2^31 terms of 2^62
    mid[k] = (k % 2 ? -1 : 1) * big(0, (1ull << 53) + (unsigned long long)k);        // (first * first stays finite at e = 128)
  }
  mass::fill_mass(&rec, top, -125, 0u);
  hex("mass", &rec.volume, 19);
  mass::fill_mass(&rec, mid, 128, 0u);
  hex("mass", &rec.volume, 19);
  gsdf_section sec;
  const __int128 sq[6] = {big(0, 3ull << 58), big(0, 15ull << 54), big(0, 3ull << 57), big(0, 21ull << 52), big(0, 13ull << 54), big(0, 15ull << 53)};
  mass::fill_section(&sec, sq, 3, 4u, 1u);
  hex("section", &sec.area, 11);
  if (sec.n_verts != 4u || sec.layer_or_n_loops != 1u) return 6;
  const __int128 none[6] = {0, 0, 0, 0, 0, 0};
  mass::fill_section(&sec, none, -125, 0u, 0u);
  hex("section", &sec.area, 11);
  if (mass::whole(0xffffffffull, (unsigned long long)-1ll) != (__int128)-1) return 7;      // low sum 2^32 - 1, rest sum -1: the integer -1
  std::printf("done\n");
  return 0;
}
'''


def test_host_arithmetic_as_a_program_under_the_sanitisers(tmp_path):
    src, exe = tmp_path / "mass_check.cpp", tmp_path / "mass_check"
    src.write_text(PROGRAM)
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                         "-static-libubsan", "-I" + CSRC, os.path.join(CSRC, "abi_mass.cpp"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    pr = subprocess.run([str(exe)], capture_output=True, text=True)
    assert pr.returncode == 0 and pr.stderr == "" and pr.stdout.strip().endswith("done"), pr.stdout[-2000:] + pr.stderr[-4000:]     # (the sanitisers report on stderr)
    lines = pr.stdout.splitlines()
    words = lambda a: " ".join("%016x" % int(x) for x in np.ascontiguousarray(a, np.float64).reshape(-1).view(np.uint64))
    got = [l.split(" ", 1)[1] for l in lines if l.startswith(("moments", "axes"))]
    want = []
    for i6 in ([3, 1, 2, 0, 0, 0], [0.4, 0.4, 0.4, 0, 0, 0], [3.5, 3.5, 2.0, 1.5, 0, 0], [97.2, 97.2, 97.2, 16.2, 16.2, 16.2]):
        m, ax = M.principal(i6)
        want += [words(m), words(ax)]
    assert got == want
    # the conversions against the twin's, on the same integers
    got = [l.split(" ", 1)[1] for l in lines if l.startswith("mass")]
    top = lambda k: (-1 if k % 2 else 1) * ((1 << 29 << 64) + 12345 + k)
    mid = lambda k: (-1 if k % 2 else 1) * ((1 << 53) + k)
    cases = [([1 << 59] + [1 << 57] * 3 + [3 << 55] * 3 + [1 << 55] * 3, 1), ([0] * 10, -125), ([top(k) for k in range(10)], -125), ([mid(k) for k in range(10)], 128)]
    assert got == [words(np.frombuffer(M.mass_record(ints, e, 0).tobytes()[:152], np.float64)) for ints, e in cases]
    unit = M.mass_record(cases[0][0], 1, 7)                                  # the first case's integers stand for 1, 1/2, 3/4 and 1/4 at e = 1
    assert unit["volume"] == 1 and unit["first"].tolist() == [0.5] * 3 and unit["second"].tolist() == [0.75] * 3 + [0.25] * 3
    assert np.isfinite(M.mass_record(*cases[3], 0)["inertia"]).all() and np.isfinite(M.mass_record(*cases[2], 0)["inertia"]).all()
    got = [l.split(" ", 1)[1] for l in lines if l.startswith("section")]
    cases = [([3 << 58, 15 << 54, 3 << 57, 21 << 52, 13 << 54, 15 << 53], 3, 4, 1), ([0] * 6, -125, 0, 0)]
    assert got == [words(np.frombuffer(M.section_record(*c).tobytes()[:88], np.float64)) for c in cases]
    square = M.section_record(*cases[0])                                     # the square (1, 2) .. (4, 6) of tests/test_gpu_mass.py
    assert square["area"] == 12 and square["first"].tolist() == [30, 48] and square["second"].tolist() == [84, 208, 120] and square["central"].tolist() == [9, 16, 0]
