"""The evaluator side's host-only unit (gsdf_amd/csrc/abi_evalhost.cpp) as a stand-alone C++ program under AddressSanitizer and
UBSan: g++ only, no GPU, nothing loaded into Python.

The unit imports four symbols (fail, gsdf_hip_program_bounds, gsdf_hip_program_is2d, gsdf_hip_eval3); the program below defines them
over a `gsdf_program` of its own -- fixed bounds and the closed-form float32 field x + 2 y - 3 z, written unfused -- and drives
  * the block cache over batches of positions pytest writes to a file, against oracle.OracleBlockCachedSDF3 around the same field:
    distances as bits, hits and evaluations after every batch, Reset, and the error returns;
  * the camera, picture-size and colour helpers with null, non-finite and degenerate arguments, against what the shipped library
    returns through ctypes for the same calls (one table of cases, rendered once as C++ and once as ctypes calls)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

from gsdf_amd import hip
from oracle.oracle import OracleBlockCachedSDF3

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "gsdf_amd", "csrc")
BB = np.array([-1.25, -2.5, 0.5, 3.0, 2.0, 4.0], F)
RES = (0.5, 0.75, 0.25)

# ---- the helper calls: (function, arguments); None is a null pointer, floats go over as float32 ------------------------------------
OK_BB = (-1.0, -2.0, -3.0, 1.0, 2.0, 3.0)
BB2 = (-20.0, -20.0, 0.0, 60.0, 20.0, 0.0)
NAN, INF = float("nan"), float("inf")
CASES = [
    # view_orbit(bb, yaw, pitch, cam_dist, target, view?)
    ("orbit", (OK_BB, 0.3, 0.2, 0.0, None, True)),
    ("orbit", (OK_BB, -2.0, 0.4, 7.5, (0.5, -0.25, 1.0), True)),
    ("orbit", (OK_BB, 1.0, math.pi / 2, 0.0, None, True)),            # pitch clamped short of the pole
    ("orbit", (OK_BB, 1.0, -40.0, 0.0, None, True)),
    ("orbit", (None, 0.0, 0.0, 0.0, None, True)),
    ("orbit", (OK_BB, 0.0, 0.0, 0.0, None, False)),
    ("orbit", ((NAN, -2.0, -3.0, 1.0, 2.0, 3.0), 0.0, 0.0, 0.0, None, True)),
    ("orbit", (OK_BB, INF, 0.0, 0.0, None, True)),
    ("orbit", (OK_BB, 0.0, NAN, 0.0, None, True)),
    ("orbit", (OK_BB, 0.0, 0.0, -INF, None, True)),
    ("orbit", (OK_BB, 0.0, 0.0, 0.0, (0.0, INF, 0.0), True)),
    ("orbit", ((1.0, 1.0, 1.0, 1.0, 1.0, 1.0), 0.0, 0.0, 0.0, None, True)),  # empty bounds, no distance
    ("orbit", ((1.0, 1.0, 1.0, 1.0, 1.0, 1.0), 0.0, 0.0, 2.0, None, True)),  # empty bounds, a distance
    ("orbit", ((-3e38, -3e38, -3e38, 3e38, 3e38, 3e38), 0.0, 0.0, 1.0, None, True)),  # the diagonal overflows
    ("orbit", (OK_BB, 0.5, 0.5, 1e-3, (1e10, 0.0, 0.0), True)),       # the camera distance vanishes next to the target
    # picture_size(bb, height, w?)
    ("size", (BB2, 1080, True)),
    ("size", ((0.0, 0.0, 0.0, 0.1, 7.7, 0.0), 4321, True)),
    ("size", (None, 100, True)),
    ("size", (BB2, 100, False)),
    ("size", ((0.0, 0.0, 0.0, NAN, 1.0, 0.0), 10, True)),
    ("size", ((0.0, 0.0, 0.0, 1.0, 1.0, 0.0), 0, True)),
    ("size", ((0.0, 0.0, 0.0, 1.0, 1.0, 0.0), 16385, True)),
    ("size", ((0.0, 0.0, 0.0, 1.0, 0.0, 0.0), 10, True)),             # no height
    ("size", ((0.0, 1.0, 0.0, 1.0, 0.0, 0.0), 10, True)),
    ("size", ((-3e38, 0.0, 0.0, 3e38, 1.0, 0.0), 10, True)),          # the width overflows float32
    ("size", ((0.0, 0.0, 0.0, 1e-3, 1.0, 0.0), 100, True)),           # width 0
    ("size", ((0.0, 0.0, 0.0, 100.0, 1.0, 0.0), 200, True)),          # width 20000
    # color_iq(bb, char_dist, out?)
    ("iq", (BB2, 0.0, True)),
    ("iq", (BB2, -1.0, True)),
    ("iq", (BB2, 2.5, True)),
    ("iq", (None, 2.5, True)),
    ("iq", (None, 0.0, True)),
    ("iq", (None, NAN, True)),
    ("iq", (BB2, 2.5, False)),
    ("iq", (BB2, INF, True)),
    ("iq", (BB2, NAN, True)),
    ("iq", ((0.0, 0.0, 0.0, NAN, 1.0, 0.0), 0.0, True)),
    ("iq", ((0.0, 0.0, 0.0, 0.0, 0.0, 0.0), 0.0, True)),              # empty bounds, no distance
    ("iq", ((-3e38, -3e38, 0.0, 3e38, 3e38, 0.0), 0.0, True)),
    # color_gradient(length, c0, c1, out?)
    ("grad", (0.5, (0, 0, 0, 255), (255, 255, 255, 255), True)),
    ("grad", (0.0, (0, 0, 0, 254), (255, 255, 255, 255), True)),
    ("grad", (3.0, (10, 200, 30, 255), (0, 0, 255, 128), True)),
    ("grad", (0.5, None, (255, 255, 255, 255), True)),
    ("grad", (0.5, (0, 0, 0, 255), None, True)),
    ("grad", (0.5, (0, 0, 0, 255), (255, 255, 255, 255), False)),
    ("grad", (-1.0, (0, 0, 0, 255), (255, 255, 255, 255), True)),
    ("grad", (NAN, (0, 0, 0, 255), (255, 255, 255, 255), True)),
    ("grad", (INF, (0, 0, 0, 255), (255, 255, 255, 255), True)),
]


def _cf(v):
    """A C++ float literal with the bits of float32(v)."""
    v = float(F(v))
    if math.isnan(v):
        return "NAN"
    if math.isinf(v):
        return "INFINITY" if v > 0 else "-INFINITY"
    return v.hex() + "f"


def _carr(typ, vals, name):
    """(declaration, expression) of an array argument; None is a null pointer."""
    if vals is None:
        return "", "nullptr"
    body = ", ".join(_cf(v) if typ == "float" else str(int(v)) for v in vals)
    return f"const {typ} {name}[{len(vals)}] = {{{body}}}; ", name


def _case_cpp(i, fn, a):
    if fn == "orbit":
        d0, bb = _carr("float", a[0], "bb")
        d1, ta = _carr("float", a[4], "ta")
        call = f"gsdf_view o; std::memset(&o, 0xAB, sizeof o); int rc = gsdf_hip_view_orbit({bb}, {_cf(a[1])}, {_cf(a[2])}, {_cf(a[3])}, {ta}, {'&o' if a[5] else 'nullptr'});"
        return f"  {{ {d0}{d1}{call} report({i}, rc, &o, sizeof o); }}\n"
    if fn == "size":
        d0, bb = _carr("float", a[0], "bb")
        return f"  {{ {d0}int o = -77; int rc = gsdf_hip_picture_size({bb}, {a[1]}, {'&o' if a[2] else 'nullptr'}); report({i}, rc, &o, sizeof o); }}\n"
    if fn == "iq":
        d0, bb = _carr("float", a[0], "bb")
        return f"  {{ {d0}gsdf_color2 o; std::memset(&o, 0xAB, sizeof o); int rc = gsdf_hip_color_iq({bb}, {_cf(a[1])}, {'&o' if a[2] else 'nullptr'}); report({i}, rc, &o, sizeof o); }}\n"
    d0, c0 = _carr("uint8_t", a[1], "c0")
    d1, c1 = _carr("uint8_t", a[2], "c1")
    return (f"  {{ {d0}{d1}gsdf_color2 o; std::memset(&o, 0xAB, sizeof o); int rc = gsdf_hip_color_gradient({_cf(a[0])}, {c0}, {c1}, {'&o' if a[3] else 'nullptr'}); "
            f"report({i}, rc, &o, sizeof o); }}\n")


def _case_ctypes(fn, a):
    """The same call on the shipped library: (return code, the output's bytes; an output left alone keeps its fill)."""
    L = hip.lib()
    fl = lambda vals: None if vals is None else (C.c_float * len(vals))(*[float(F(v)) for v in vals])
    u8 = lambda vals: None if vals is None else (C.c_uint8 * 4)(*vals)
    if fn == "orbit":
        o = hip.GsdfView()
        C.memset(C.byref(o), 0xAB, C.sizeof(o))
        rc = L.gsdf_hip_view_orbit(fl(a[0]), F(a[1]), F(a[2]), F(a[3]), fl(a[4]), C.byref(o) if a[5] else None)
    elif fn == "size":
        o = C.c_int(-77)
        rc = L.gsdf_hip_picture_size(fl(a[0]), a[1], C.byref(o) if a[2] else None)
    elif fn == "iq":
        o = hip.GsdfColor2()
        C.memset(C.byref(o), 0xAB, C.sizeof(o))
        rc = L.gsdf_hip_color_iq(fl(a[0]), F(a[1]), C.byref(o) if a[2] else None)
    else:
        o = hip.GsdfColor2()
        C.memset(C.byref(o), 0xAB, C.sizeof(o))
        rc = L.gsdf_hip_color_gradient(F(a[0]), u8(a[1]), u8(a[2]), C.byref(o) if a[3] else None)
    return rc, bytes(o).hex()


PROGRAM_HEAD = r"""
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#include "abi_host.h"

// ---- what abi_evalhost.cpp imports ----------------------------------------------------------------------------------------------
struct gsdf_program { float bb[6]; int is2d; uint64_t calls; };
static std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
extern "C" int gsdf_hip_program_bounds(const gsdf_program* p, float bb[6]) {
  if (!p || !bb) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  std::memcpy(bb, p->bb, sizeof(float) * 6);
  return GSDF_OK;
}
extern "C" int gsdf_hip_program_is2d(const gsdf_program* p) { return p && p->is2d ? 1 : 0; }
extern "C" int gsdf_hip_eval3(gsdf_program* p, const void* pos, size_t stride, size_t n_pos, float* dist, size_t n_dist) {
  if (!p || !pos || !dist || n_pos != n_dist || n_pos == 0 || stride < 12) return fail(GSDF_ERR_BAD_ARGUMENT, "the cache passed on a bad call");
  p->calls++;
  for (size_t i = 0; i < n_pos; i++) {
    const float* q = (const float*)((const char*)pos + i * stride);
    const float ty = 2.0f * q[1];
    const float tz = 3.0f * q[2];
    const float s = q[0] + ty;
    dist[i] = s - tz;
  }
  return GSDF_OK;
}

static void report(int i, int rc, const void* out, size_t n) {
  std::printf("case %d %d ", i, rc);
  for (size_t k = 0; k < n; k++) std::printf("%02x", ((const unsigned char*)out)[k]);
  std::printf("\n");
}
static void helper_cases() {
"""

PROGRAM_TAIL = r"""
}

static int refused(const char* what, int rc) {
  std::printf("err %s %d %s\n", what, rc, rc ? g_err.c_str() : "");
  return rc;
}

// argv: positions file, distances file, resx resy resz. Positions file: per batch uint64 n, uint64 stride, n * stride bytes.
int main(int argc, char** argv) {
  if (argc != 6) return 2;
  const float rx = std::stof(argv[3]), ry = std::stof(argv[4]), rz = std::stof(argv[5]);
  gsdf_program prog = {{%BB%}, 0, 0};
  gsdf_program flat = prog;
  flat.is2d = 1;
  gsdf_blockcache* c = nullptr;
  refused("res_zero", gsdf_hip_blockcache_create(&prog, 0.0f, ry, rz, &c));
  refused("res_negative", gsdf_hip_blockcache_create(&prog, rx, -ry, rz, &c));
  refused("res_nan", gsdf_hip_blockcache_create(&prog, rx, ry, NAN, &c));
  refused("program_2d", gsdf_hip_blockcache_create(&flat, rx, ry, rz, &c));
  refused("program_null", gsdf_hip_blockcache_create(nullptr, rx, ry, rz, &c));
  if (c) return 3;
  if (refused("create", gsdf_hip_blockcache_create(&prog, rx, ry, rz, &c)) || !c) return 3;
  {
    float p4[8] = {0, 0, 0, 0, 0, 0, 0, 0}, d2[2];
    refused("length_mismatch", gsdf_hip_blockcache_eval3(c, p4, 12, 2, d2, 1));
    refused("empty", gsdf_hip_blockcache_eval3(c, p4, 12, 0, d2, 0));
    refused("stride_8", gsdf_hip_blockcache_eval3(c, p4, 8, 2, d2, 2));
    refused("stride_13", gsdf_hip_blockcache_eval3(c, p4, 13, 1, d2, 1));
    refused("null_buffer", gsdf_hip_blockcache_eval3(c, nullptr, 12, 2, d2, 2));
    refused("null_cache", gsdf_hip_blockcache_eval3(nullptr, p4, 12, 2, d2, 2));
    std::printf("after_errors %llu %llu %llu\n", (unsigned long long)gsdf_hip_blockcache_hits(c), (unsigned long long)gsdf_hip_blockcache_evaluations(c),
                (unsigned long long)prog.calls);
  }
  FILE* in = std::fopen(argv[1], "rb");
  FILE* out = std::fopen(argv[2], "wb");
  if (!in || !out) return 4;
  std::vector<char> first;
  uint64_t first_n = 0, first_stride = 0, hdr[2];
  for (int b = 0; std::fread(hdr, 8, 2, in) == 2; b++) {
    std::vector<char> pos(hdr[0] * hdr[1]);
    if (std::fread(pos.data(), 1, pos.size(), in) != pos.size()) return 5;
    std::vector<float> dist(hdr[0]);
    if (refused("batch", gsdf_hip_blockcache_eval3(c, pos.data(), hdr[1], hdr[0], dist.data(), hdr[0]))) return 6;
    std::fwrite(dist.data(), 4, dist.size(), out);
    std::printf("batch %d %llu %llu\n", b, (unsigned long long)gsdf_hip_blockcache_hits(c), (unsigned long long)gsdf_hip_blockcache_evaluations(c));
    if (b == 0) { first = pos; first_n = hdr[0]; first_stride = hdr[1]; }
  }
  std::fclose(in);
  // Reset clears the counters and the cells: the first batch again misses where it missed before
  if (refused("reset", gsdf_hip_blockcache_reset(c, &prog, rx, ry, rz))) return 7;
  std::printf("reset %llu %llu\n", (unsigned long long)gsdf_hip_blockcache_hits(c), (unsigned long long)gsdf_hip_blockcache_evaluations(c));
  {
    std::vector<float> dist(first_n);
    if (refused("batch", gsdf_hip_blockcache_eval3(c, first.data(), first_stride, first_n, dist.data(), first_n))) return 8;
    std::fwrite(dist.data(), 4, dist.size(), out);
    std::printf("again %llu %llu\n", (unsigned long long)gsdf_hip_blockcache_hits(c), (unsigned long long)gsdf_hip_blockcache_evaluations(c));
  }
  std::fclose(out);
  gsdf_hip_blockcache_destroy(c);
  gsdf_hip_blockcache_destroy(nullptr);
  std::printf("null_handles %llu %llu\n", (unsigned long long)gsdf_hip_blockcache_hits(nullptr), (unsigned long long)gsdf_hip_blockcache_evaluations(nullptr));
  helper_cases();
  std::printf("done\n");
  return 0;
}
"""


class Field:
    """The program's field and bounds, for the oracle's cache."""

    def Bounds(self):
        return BB

    def Evaluate(self, pos):
        pos = np.asarray(pos, F).reshape(-1, 3)
        return ((pos[:, 0] + F(2) * pos[:, 1]) - F(3) * pos[:, 2]).astype(F)


def _batches():
    """Four batches of about 300 points: inside and around the bounds (below bb.Min the cell numbers are negative and truncate toward
    zero: (-res, res) is ONE cell), exact repeats inside a batch, earlier points again and nudged inside their cell, strides 12 / 16."""
    rng = np.random.default_rng(7)
    lo, hi = BB[:3] - F(2), BB[3:] + F(1)
    out, seen = [], np.zeros((0, 3), F)
    for b in range(4):
        fresh = (lo + rng.random((180, 3)).astype(F) * (hi - lo)).astype(F)
        near_min = (BB[:3] + (rng.random((40, 3)).astype(F) * F(2) - F(1)) * np.array(RES, F)).astype(F)  # both sides of bb.Min, one cell
        parts = [fresh, near_min, fresh[rng.integers(0, 180, 30)]]  # exact repeats
        if len(seen):
            old = seen[rng.integers(0, len(seen), 60)]
            parts += [old[:30], (old[30:] + F(1e-3) * rng.standard_normal((30, 3)).astype(F)).astype(F)]
        pts = np.concatenate(parts).astype(F)
        pts = pts[rng.permutation(len(pts))]
        seen = np.concatenate([seen, pts])
        out.append((pts, 12 if b % 2 == 0 else 16))
    return out


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("evalhost")
    src = tmp / "evalhost_check.cpp"
    body = "".join(_case_cpp(i, fn, a) for i, (fn, a) in enumerate(CASES))
    src.write_text(PROGRAM_HEAD + body + PROGRAM_TAIL.replace("%BB%", ", ".join(_cf(v) for v in BB)))
    exe = tmp / "evalhost_check"
    cc = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan",
                         "-D__HIP_PLATFORM_AMD__",
                         "-I/opt/rocm/include", "-I" + CSRC, "-I" + os.path.join(ROOT, "include"),
                         os.path.join(CSRC, "abi_evalhost.cpp"), os.path.join(CSRC, "compile.cpp"), str(src), "-o", str(exe)], capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    batches = _batches()
    with open(tmp / "pos.bin", "wb") as f:
        for pts, stride in batches:
            rows = np.full((len(pts), stride // 4), np.nan, F)  # (the fourth word of a 16-byte position is never read)
            rows[:, :3] = pts
            f.write(np.array([len(pts), stride], np.uint64).tobytes() + rows.tobytes())
    pr = subprocess.run([str(exe), str(tmp / "pos.bin"), str(tmp / "dist.bin")] + [repr(r) for r in RES], capture_output=True, text=True)
    assert pr.returncode == 0 and pr.stderr == "" and pr.stdout.strip().endswith("done"), pr.stdout[-2000:] + pr.stderr[-4000:]  # (the sanitisers report on stderr)
    return batches, pr.stdout.splitlines(), np.fromfile(tmp / "dist.bin", F)


def test_block_cache_matches_the_oracle(run):
    batches, lines, dist = run
    ref = OracleBlockCachedSDF3(Field(), *RES)
    got = [tuple(int(x) for x in l.split()[2:]) for l in lines if l.startswith("batch ")]
    assert len(got) == 4
    at = 0
    for b, (pts, _) in enumerate(batches):
        want = ref.Evaluate(pts)
        have = dist[at:at + len(pts)]
        at += len(pts)
        assert (have.view(np.uint32) == want.view(np.uint32)).all(), b
        assert got[b] == (ref.hits, ref.evals), b
    assert ref.hits > 100 and ref.evals == sum(len(p) for p, _ in batches)  # the batches do hit: repeats, cells met again
    # a hit returns the cell's distance, not the point's: the batches hold such points
    allp = np.concatenate([p for p, _ in batches])
    assert (dist[:at].view(np.uint32) != Field().Evaluate(allp).view(np.uint32)).any()
    # Reset clears both counters and the cells
    ref.Reset(Field(), *RES)
    assert [l for l in lines if l.startswith("reset ")] == ["reset 0 0"]
    want = ref.Evaluate(batches[0][0])
    assert (dist[at:].view(np.uint32) == want.view(np.uint32)).all() and len(dist) == at + len(want)
    assert [l for l in lines if l.startswith("again ")] == [f"again {ref.hits} {ref.evals}"]
    assert "null_handles 0 0" in lines


def test_block_cache_error_returns(run):
    _, lines, _ = run
    err = {l.split()[1]: (int(l.split()[2]), " ".join(l.split()[3:])) for l in lines if l.startswith("err ")}
    for what in ("res_zero", "res_negative", "res_nan"):
        assert err[what] == (-8, "invalid resolution for BlockCachedSDF3"), what
    assert err["program_2d"] == (-7, "program is 2D")
    assert err["program_null"] == (-3, "null argument")
    assert err["length_mismatch"] == (-2, "position and distance buffer length mismatch")
    assert err["empty"] == (-1, "empty buffers")
    assert err["stride_8"] == (-3, "bad position stride") and err["stride_13"] == (-3, "bad position stride")
    assert err["null_buffer"] == (-3, "null buffer") and err["null_cache"] == (-3, "null argument")
    assert err["create"] == (0, "") and err["reset"] == (0, "") and err["batch"] == (0, "")
    assert "after_errors 0 0 0" in lines  # a refused call counts nothing and evaluates nothing
    with pytest.raises(ValueError):
        OracleBlockCachedSDF3(Field(), 0.0, RES[1], RES[2])


def test_helpers_return_what_the_shipped_library_returns(run):
    _, lines, _ = run
    got = {int(l.split()[1]): (int(l.split()[2]), l.split()[3]) for l in lines if l.startswith("case ")}
    assert len(got) == len(CASES)
    codes = []
    for i, (fn, a) in enumerate(CASES):
        assert got[i] == _case_ctypes(fn, a), (i, fn, a)
        codes.append(got[i][0])
    assert codes.count(0) >= 14 and codes.count(-3) >= 30 and set(codes) == {0, -3}
