"""The marshalling step of a kernel launch (gsdf_amd/csrc/launch_args.h), on the host: a stand-alone C++ program, g++ only.

Every kernel that exists both ahead of time and per tree is launched through one function (abi_program.h: launch_kernel) that takes
the parameter types from the kernel's signature and converts each argument to them, whatever the type of the expression at the call.
The program below feeds the header a made-up signature and arguments of other types, and checks that slot i of the pointer array
points at storage of parameter i's size holding the converted value; that a wrong count or a non-convertible argument is refused at
compile time is asserted inside the program (launch_args::accepts), not by a failing compiler run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <cstring>
#include "launch_args.h"

using launch_args::accepts;
using launch_args::Marshalled;
typedef void Sig(const uint32_t*, unsigned long long, int, float, uint64_t, unsigned);
struct Cam { float ro[3]; int aa; };
struct Other { int x; };

// what the compiler refuses: a wrong count, a non-convertible argument
static_assert(accepts<Sig, uint32_t*, int, size_t, double, int, long>::value, "arguments of other arithmetic types are converted");
static_assert(accepts<Sig, void*, int, int, int, int, int>::value, "void* goes to a typed pointer parameter (static_cast)");
static_assert(accepts<Sig, decltype(nullptr), int, int, int, int, int>::value, "nullptr is a pointer");
static_assert(!accepts<Sig, uint32_t*, int, size_t, double, int>::value, "one argument short");
static_assert(!accepts<Sig, uint32_t*, int, size_t, double, int, long, int>::value, "one argument too many");
static_assert(!accepts<Sig>::value, "no arguments");
static_assert(!accepts<Sig, float*, int, int, float, int, int>::value, "float* is no const uint32_t*");
static_assert(!accepts<Sig, int, int, int, float, int, int>::value, "an integer is no pointer");
static_assert(!accepts<Sig, uint32_t*, int*, int, float, int, int>::value, "a pointer is no integer");
static_assert(!accepts<Sig, uint32_t*, int, int, Other, int, int>::value, "a struct is no float");
static_assert(accepts<void(Cam, float*), Cam, float*>::value && accepts<void(Cam, float*), const Cam&, void*>::value, "a struct by value");
static_assert(!accepts<void(Cam, float*), Other, float*>::value, "another struct");
static_assert(accepts<void()>::value && !accepts<void(), int>::value, "no parameters");

static int fails = 0;
template <typename T>
static void expect(void* slot, T want, const char* what) {
  T got;
  std::memcpy(&got, slot, sizeof(T));
  if (std::memcmp(&got, &want, sizeof(T)) != 0) { std::printf("FAIL %s\n", what); fails++; }
}

int main() {
  uint32_t code[4] = {1, 2, 3, 4};
  const size_t n = 70000;        // for the int
  const double step = 0.1;       // for the float: 0.1 is not representable, the slot must hold float(0.1)
  {
    // int literals for the 64-bit parameters: 4 bytes at the call, 8 in the slot
    Marshalled<Sig> m(code, -1, n, step, 5, 7L);
    static_assert(Marshalled<Sig>::N == 6, "six parameters");
    void** a = m.args();
    expect<const uint32_t*>(a[0], code, "pointer");
    expect<unsigned long long>(a[1], 0xffffffffffffffffull, "int -1 -> unsigned long long (all 8 bytes)");
    expect<int>(a[2], 70000, "size_t -> int");
    expect<float>(a[3], 0.1f, "double -> float");
    expect<uint64_t>(a[4], (uint64_t)5, "int -> uint64_t (all 8 bytes)");
    expect<unsigned>(a[5], 7u, "long -> unsigned");
    // each slot is storage of its own: distinct, inside the object, none aliasing an argument
    for (int i = 0; i < 6; i++) {
      if ((char*)a[i] < (char*)&m || (char*)a[i] >= (char*)&m + sizeof m) { std::printf("FAIL slot %d outside the marshalled storage\n", i); fails++; }
      for (int j = 0; j < i; j++) if (a[i] == a[j]) { std::printf("FAIL slots %d and %d alias\n", i, j); fails++; }
    }
    // storage of the parameter's size: writing the full width of every slot stays inside the object (the sanitizer run sees it if not)
    unsigned long long big = 0x0123456789abcdefull;
    std::memcpy(a[1], &big, 8);
    std::memcpy(a[4], &big, 8);
    expect<unsigned long long>(a[1], big, "8-byte slot");
    expect<int>(a[2], 70000, "neighbour untouched");
    expect<float>(a[3], 0.1f, "neighbour untouched");
    expect<unsigned>(a[5], 7u, "neighbour untouched");
  }
  {
    // the later arguments of a call are evaluated once and copied, not referenced
    int level = 3;
    Marshalled<void(int, unsigned long long)> m(level, level);
    level = 9;
    expect<int>(m.args()[0], 3, "copied at the call");
    expect<unsigned long long>(m.args()[1], 3ull, "copied at the call");
  }
  {
    Cam cam = {{1.f, 2.f, 3.f}, 4};
    float out[2];
    void* vp = out;
    Marshalled<void(Cam, float*)> m(cam, vp);
    Cam got;
    std::memcpy(&got, m.args()[0], sizeof got);
    if (std::memcmp(&got, &cam, sizeof cam) != 0) { std::printf("FAIL struct by value\n"); fails++; }
    expect<float*>(m.args()[1], out, "void* -> float*");
  }
  {
    Marshalled<void(const float*, int)> m(nullptr, 1);
    expect<const float*>(m.args()[0], nullptr, "nullptr");
  }
  if (fails) return 1;
  std::printf("ok\n");
  return 0;
}
"""


def test_arguments_are_converted_to_the_kernels_parameter_types(tmp_path):
    src = tmp_path / "launch_args_check.cpp"
    src.write_text(PROGRAM)
    exe = tmp_path / "launch_args_check"
    cc = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-O1", "-I", os.path.join(ROOT, "gsdf_amd", "csrc"), str(src), "-o", str(exe)],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr


def test_header_needs_no_hip():
    """The marshalling header is host-only: it includes nothing of HIP (the program above is compiled without ROCm's include path)."""
    text = open(os.path.join(ROOT, "gsdf_amd", "csrc", "launch_args.h")).read()
    assert "#include <hip" not in text and "#include \"abi_" not in text
