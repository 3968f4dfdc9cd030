// abi_eval.hip -- C ABI (include/gsdf_hip.h), evaluator side, what launches kernels: program handles (their per-tree kernels:
// abi_spec.hip), the self-test hooks, the gleval.SDF3 / SDF2 Evaluate drop-ins (host buffers, pipelined tickets, registered memory,
// device-resident), central-difference normals, projection, rays, the 2-D image and picture renderers, the UI's view of a 3-D part.
// Kernels: kernels_eval.h, kernels_image.h, kernels_view.h, kernels_project.h and kernels_ray.h over the interpreter of interp.h.
// The entry points of this side that need no GPU (camera, colour conversions, block cache): abi_evalhost.cpp.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <thread>

#include "kernels_common.h"
#include "kernels_eval.h"
#include "kernels_view.h"
#include "kernels_project.h"
#include "kernels_ray.h"
#include "kernels_image.h"
#include "abi_program.h"

extern "C" int gsdf_hip_init(int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n == 0) return fail(GSDF_ERR_NO_DEVICE, std::string("no HIP device: ") + hipGetErrorString(e));
  if (device >= 0) {
    if (device >= n) return fail(GSDF_ERR_NO_DEVICE, "device index out of range");
    HIP_TRY(hipSetDevice(device));
  }
  return GSDF_OK;
}

extern "C" int gsdf_hip_grid_cus(int device, int* real_cus) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n == 0) { (void)hipGetLastError(); return 0; }
  if (device < 0 && hipGetDevice(&device) != hipSuccess) return 0;
  if (device >= n) return 0;
  return grid_cus(device, real_cus);
}

extern "C" int gsdf_hip_program_create(const gsdf_tree* tree, gsdf_program** out) {
  if (!tree || !out) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *out = nullptr;
  gsdf_program* p = new (std::nothrow) gsdf_program();
  if (!p) return fail(GSDF_ERR_BAD_ARGUMENT, "out of memory");
  try {
    p->prog = gsdf_dev::compile(*tree);
  } catch (const std::exception& e) {
    delete p;
    return fail(GSDF_ERR_BAD_TREE, e.what());
  }
  int ndev = 0;
  hipError_t e = hipGetDeviceCount(&ndev);
  if (e != hipSuccess || ndev == 0) {
    delete p;
    return fail(GSDF_ERR_NO_DEVICE, std::string("no HIP device: ") + hipGetErrorString(e));
  }
  auto cleanup = [&](int code) { gsdf_hip_program_destroy(p); return code; };
  if (hipGetDevice(&p->device) != hipSuccess) return cleanup(fail(GSDF_ERR_HIP, "hipGetDevice failed"));
  p->num_cu = grid_cus(p->device);
  if (p->lds_bytes(p->batch_k()) + gsdf_program::kCreateExtra > gsdf_program::kLdsPerCu) return cleanup(fail(GSDF_ERR_BAD_TREE, "tree needs more LDS scratch than one CU has"));
  if (p->stream.ensure() != hipSuccess) return cleanup(fail(GSDF_ERR_HIP, "hipStreamCreate failed"));
  size_t bytes = p->prog.code.size() * sizeof(uint32_t);
  if (hipMalloc((void**)&p->d_code.p, bytes) != hipSuccess) return cleanup(fail(GSDF_ERR_HIP, "hipMalloc(program) failed"));
  if (hipMemcpy(p->d_code.p, p->prog.code.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return cleanup(fail(GSDF_ERR_HIP, "hipMemcpy(program) failed"));
  *out = p;
  return GSDF_OK;
}

// What the exhaustive self-test hooks below share: a zeroed block of two counters on the device, `launch(counters)` on the null
// stream, the two words back in *out0 and *out1 (either may be null; written on success only).
template <typename Launch>
static int selftest_run(uint64_t* out0, uint64_t* out1, Launch&& launch) {
  DevBuf d_c;
  HIP_TRY(d_c.alloc(16));
  if (hipMemset(d_c.p, 0, 16) != hipSuccess) return fail(GSDF_ERR_HIP, "memset failed");
  launch((unsigned long long*)d_c.p);
  unsigned long long h[2] = {0, 0};
  if (hipMemcpy(h, d_c.p, 16, hipMemcpyDeviceToHost) != hipSuccess) return fail(GSDF_ERR_HIP, "selftest kernel failed");
  if (out0) *out0 = h[0];
  if (out1) *out1 = h[1];
  return GSDF_OK;
}

// Test hook: runs dm::div_by_uniform(n, d, RN(1/d)) for all 2^32 numerators n on the GPU and counts results that
// differ from n / d among the numerators the interpreter would send down the fast path.
extern "C" int gsdf_hip_selftest_div(float d, uint64_t* mismatches, uint64_t* fast_path_numerators, float* recip) {
  const float r = gsdf_dev::recip_for(d);
  if (recip) *recip = r;
  if (mismatches) *mismatches = 0;
  if (fast_path_numerators) *fast_path_numerators = 0;
  if (r == 0.f) return GSDF_OK;  // divisor not eligible: the device always uses the IEEE expansion
  return selftest_run(mismatches, fast_path_numerators, [&](unsigned long long* c) { hipLaunchKernelGGL(div_selftest_kernel, dim3(4096), dim3(BLOCK), 0, nullptr, d, r, c, c + 1); });
}

// Test hook: dm::circ_sector_fast (the circular array's sector index without the angle) against the reference's
// floor(float32(atan2(y, x)) / angle) over 2^32 points -- all magnitudes, signed zeros, and points hugging the sector
// boundaries -- for angle = float32(2 pi) / ncirc as circarray forms it (cpu_evaluators.go:1047).
extern "C" int gsdf_hip_selftest_circ(float ncirc, uint64_t* mismatches, uint64_t* fast_path_points) {
  if (mismatches) *mismatches = 0;
  if (fast_path_points) *fast_path_points = 0;
  if (!(ncirc >= 1.f)) return fail(GSDF_ERR_BAD_ARGUMENT, "ncirc must be >= 1");
  const float angle = 6.2831853071795862f / ncirc;
  return selftest_run(mismatches, fast_path_points, [&](unsigned long long* c) { hipLaunchKernelGGL(circ_selftest_kernel, dim3(4096), dim3(BLOCK), 0, nullptr, angle, c, c + 1); });
}

// Test hook: dm::atan2_fast (float32 of math.Atan2 without the reference's float64 operation sequence, accepted only where the
// rounding is decided) against dm::atan2_ref, over 2^log2n pairs of `mode` (kernels_eval.h: atan2_selftest_kernel).
extern "C" int gsdf_hip_selftest_atan2(int mode, int log2n, uint64_t* mismatches, uint64_t* fast_path_points) {
  if (mismatches) *mismatches = 0;
  if (fast_path_points) *fast_path_points = 0;
  if (mode < 0 || mode > 2 || log2n < 0 || log2n > 40) return fail(GSDF_ERR_BAD_ARGUMENT, "mode in 0..2, log2n in 0..40");
  return selftest_run(mismatches, fast_path_points, [&](unsigned long long* c) { hipLaunchKernelGGL(atan2_selftest_kernel, dim3(4096), dim3(BLOCK), 0, nullptr, mode, log2n, c, c + 1); });
}

// Test hook: dm::cossin_fast (float32 of math.Cos / math.Sin by FMAs, accepted only where the rounding is decided) against dm::cossinf_,
// over every float32 argument.
extern "C" int gsdf_hip_selftest_cossin(uint64_t* mismatches, uint64_t* fast_path_arguments) {
  if (mismatches) *mismatches = 0;
  if (fast_path_arguments) *fast_path_arguments = 0;
  return selftest_run(mismatches, fast_path_arguments, [&](unsigned long long* c) { hipLaunchKernelGGL(cossin_selftest_kernel, dim3(4096), dim3(BLOCK), 0, nullptr, c, c + 1); });
}

// Test hook: dm::sqrt_1to2 against sqrtf for all 8,388,609 floats in [1, 2]; dm::sqrt_core against sqrtf for every float >= 2^-96.
extern "C" int gsdf_hip_selftest_sqrt(uint64_t* mismatches) {
  if (mismatches) *mismatches = 0;
  return selftest_run(mismatches, nullptr, [&](unsigned long long* c) { hipLaunchKernelGGL(sqrt_selftest_kernel, dim3(1024), dim3(BLOCK), 0, nullptr, c); });
}

// Test hook: one of the device's math routes over n host values (kernels_eval.h: math_selftest_kernel), for a comparison with the
// oracle's restatement of the same function on the host. y may be null for the functions of one argument; for fn 17 the divisor is
// divisor (wave-uniform, with the host's RN(1/divisor) where recip_for grants one) and y is not read; for fn 20 / 21 it is the third
// slab distance.
extern "C" int gsdf_hip_selftest_math(int fn, const float* x, const float* y, float* out, uint64_t n, float divisor) {
  if (fn < 0 || fn > 21 || !x || !out) return fail(GSDF_ERR_BAD_ARGUMENT, "fn in 0..21, x and out not null");
  if (n == 0) return GSDF_OK;
  if (n > (1ull << 28)) return fail(GSDF_ERR_BAD_ARGUMENT, "n <= 2^28");
  const bool two = fn == 0 || fn == 1 || fn == 8 || fn == 9 || fn == 15 || fn >= 18;
  if (two && !y) return fail(GSDF_ERR_BAD_ARGUMENT, "this function takes two operands");
  const size_t bytes = (size_t)n * sizeof(float);
  DevBuf buf;
  HIP_TRY(buf.alloc(3 * bytes));
  float* d_b = (float*)buf.p;
  if (hipMemcpy(d_b, x, bytes, hipMemcpyHostToDevice) != hipSuccess) return fail(GSDF_ERR_HIP, "copy failed");
  if (two && hipMemcpy(d_b + n, y, bytes, hipMemcpyHostToDevice) != hipSuccess) return fail(GSDF_ERR_HIP, "copy failed");
  const float r = fn == 17 ? gsdf_dev::recip_for(divisor) : 0.f;
  hipLaunchKernelGGL(math_selftest_kernel, dim3((unsigned)((n + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, nullptr, fn, d_b, two ? d_b + n : nullptr,
                     d_b + 2 * n, n, divisor, r);
  if (hipMemcpy(out, d_b + 2 * n, bytes, hipMemcpyDeviceToHost) != hipSuccess) return fail(GSDF_ERR_HIP, "selftest kernel failed");
  return GSDF_OK;
}

extern "C" void gsdf_hip_program_destroy(gsdf_program* p) { delete p; }  // (~gsdf_program, abi_program.h)

extern "C" int gsdf_hip_program_bounds(const gsdf_program* p, float bb[6]) {
  if (!p || !bb) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  std::memcpy(bb, p->prog.bb, sizeof(float) * 6);
  return GSDF_OK;
}
extern "C" int gsdf_hip_program_is2d(const gsdf_program* p) { return p && p->prog.is2d ? 1 : 0; }
extern "C" int gsdf_hip_program_info(const gsdf_program* p, uint32_t* code_words, uint32_t* lds_slots) {
  if (!p) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (code_words) *code_words = (uint32_t)p->prog.code.size();
  if (lds_slots) *lds_slots = (uint32_t)p->prog.nslots;
  return GSDF_OK;
}
extern "C" uint64_t gsdf_hip_evaluations(const gsdf_program* p) { return p ? p->evals + p->evals_host.load() : 0; }

// The ahead-of-time eval_kernel<DIM, K, W> of a variant: exactly the instantiations this library launches (null: none).
using eval_kernel_t = decltype(&eval_kernel<3, 4, 4>);
static eval_kernel_t eval_aot(int dim, SweepVariant v) {
  const int w = v.k == 1 ? 4 : (v.w == 4 ? 4 : 3);
  if (dim == 3) {
    if (v.k == 4) return w == 4 ? eval_kernel<3, 4, 4> : eval_kernel<3, 4, 3>;
    if (v.k == 2) return w == 4 ? eval_kernel<3, 2, 4> : eval_kernel<3, 2, 3>;
    return eval_kernel<3, 1, 4>;
  }
  if (v.k == 4) return w == 4 ? eval_kernel<2, 4, 4> : eval_kernel<2, 4, 3>;
  if (v.k == 2) return w == 4 ? eval_kernel<2, 2, 4> : eval_kernel<2, 2, 3>;
  return eval_kernel<2, 1, 4>;
}

// host_mapped: the buffers are pinned host memory the kernel reaches across PCIe (the host-buffer API's small and registered calls).
// Such a call is bound by the reads' latency and bandwidth, not by the evaluation: ONE point per lane puts four times as many
// workgroups on the bus at once (32 768 points: 128 workgroups instead of 32) -- 24.6 -> 19.6 us per blocking call from registered
// buffers, 31.4 -> 26.1 us from pageable ones (tools/gpu_dropin_k.sh).
static int eval_dev(gsdf_program* p, int dim, const void* d_pos, size_t stride_bytes, float* d_dist, size_t n, hipStream_t s, bool count = true, bool host_mapped = false) {
  if (stride_bytes % 4 != 0 || stride_bytes < (size_t)dim * 4) return fail(GSDF_ERR_BAD_ARGUMENT, "bad position stride");
  spec_adopt(p);  // (a background build that has finished: its kernels from here on)
  static const bool k1_off = env_flag("GSDF_HIP_NO_EVAL_K1");  // developer knob (A/B timing)
  // This entry runs on several host threads at once (the host-buffer calls): the kernel it launches and what that kernel was built
  // for are read as ONE snapshot under the mutex every writer of them holds: adoption and the K = 1 group's build (abi_spec.hip).
  hipFunction_t f_eval = nullptr, f_eval_k1 = nullptr;
  int spec_eval_k = 0;
  {
    std::lock_guard<std::mutex> lk(p->spec_async_mu);
    f_eval = p->spec.f_eval; f_eval_k1 = p->spec.f_eval_k1; spec_eval_k = p->spec.eval_k;
  }
  const bool latency = host_mapped && !k1_off && (f_eval_k1 != nullptr || f_eval == nullptr);  // (a specialised handle without a K = 1 build keeps its specialised kernel)
  const int k = latency ? 1 : p->batch_k();
  static const int eval_bpc = env_int("GSDF_HIP_EVAL_BPC", 64);  // tuning knob: finer grids drain evenly (8 -> 64 per CU: +10 % on npt-flange)
  const unsigned grid = grid_for((n + k - 1) / k, p->num_cu, eval_bpc);
  // the per-tree kernel with one point per lane for a latency-bound call, else the one built for this K (whichever W it was
  // built for: same launch), else the interpreter's
  const hipFunction_t f = latency && f_eval_k1 ? f_eval_k1 : (f_eval && spec_eval_k == k ? f_eval : nullptr);
  HIP_TRY(launch_kernel(eval_aot(dim, p->sweep_variant(k)), f, grid, BLOCK, p->lds_bytes(k), s, p->d_code.p, d_pos, stride_bytes / 4, d_dist, n));
  if (count) p->evals += n;  // (concurrent host-buffer callers count through evals_host instead)
  return GSDF_OK;
}

// ---- caller buffers the GPU can reach directly (pinned + device-mapped): no staging copy at all ----------------------
// Process-wide table of host ranges registered through gsdf_hip_host_alloc / gsdf_hip_host_register. A call whose
// positions AND distances lie inside such ranges runs the kernel straight on the caller's memory across PCIe.
namespace {
struct HostRange { char* p; size_t n; bool owned; };
std::mutex g_reg_mu;
std::vector<HostRange> g_reg;
void* reg_device_ptr(const void* h, size_t n) {
  std::lock_guard<std::mutex> lk(g_reg_mu);
  for (const HostRange& r : g_reg)
    if ((const char*)h >= r.p && (const char*)h + n <= r.p + r.n) {
      void* d = nullptr;
      if (hipHostGetDevicePointer(&d, r.p, 0) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
      return (char*)d + ((const char*)h - r.p);
    }
  return nullptr;
}
}  // namespace
extern "C" void* gsdf_hip_host_alloc(size_t bytes) {
  void* h = nullptr;
  if (bytes == 0 || hipHostMalloc(&h, bytes, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  std::lock_guard<std::mutex> lk(g_reg_mu);
  g_reg.push_back(HostRange{(char*)h, bytes, true});
  return h;
}
extern "C" int gsdf_hip_host_register(void* ptr, size_t bytes) {
  if (!ptr || bytes == 0) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  HIP_TRY(hipHostRegister(ptr, bytes, hipHostRegisterMapped | hipHostRegisterPortable));
  std::lock_guard<std::mutex> lk(g_reg_mu);
  g_reg.push_back(HostRange{(char*)ptr, bytes, false});
  return GSDF_OK;
}
extern "C" int gsdf_hip_host_release(void* ptr) {  // gsdf_hip_host_alloc'ed: freed; gsdf_hip_host_register'ed: unregistered
  if (!ptr) return GSDF_OK;
  HostRange r{nullptr, 0, false};
  {
    std::lock_guard<std::mutex> lk(g_reg_mu);
    for (size_t i = 0; i < g_reg.size(); i++)
      if (g_reg[i].p == (char*)ptr) { r = g_reg[i]; g_reg.erase(g_reg.begin() + (long)i); break; }
  }
  if (!r.p) return fail(GSDF_ERR_BAD_ARGUMENT, "not a registered host buffer");
  if (r.owned) HIP_TRY(hipHostFree(r.p));
  else HIP_TRY(hipHostUnregister(r.p));
  return GSDF_OK;
}

static constexpr size_t kSmallPos = (size_t)1 << 20, kSmallDist = (size_t)1 << 18;

// What every Evaluate drop-in refuses: a program of the other dimension; for the host-buffer forms, gleval's argument errors first.
static int eval_dim_refused(const gsdf_program* p, int dim) {
  if (p->prog.is2d != (dim == 2)) return fail(GSDF_ERR_DIMENSION, dim == 2 ? "program is 3D, eval2 called" : "program is 2D, eval3 called");
  return GSDF_OK;
}
static int eval_args_refused(const gsdf_program* p, int dim, const void* pos, const float* dist, size_t n_pos, size_t n_dist) {
  if (!p) return fail(GSDF_ERR_BAD_ARGUMENT, "null program");
  if (n_pos != n_dist) return fail(GSDF_ERR_LENGTH_MISMATCH, "position and distance buffer length mismatch");
  if (n_pos == 0) return fail(GSDF_ERR_EMPTY_BUFFERS, "empty buffers");
  if (!pos || !dist) return fail(GSDF_ERR_BAD_ARGUMENT, "null buffer");
  return eval_dim_refused(p, dim);
}

static int slot_acquire(gsdf_program* p, int* idx) {
  std::unique_lock<std::mutex> lk(p->slot_mu);
  for (;;) {
    for (int i = 0; i < gsdf_program::kSlots; i++)
      if (!p->slot[i].busy) { p->slot[i].busy = true; p->slot[i].waiting = false; p->slot[i].gen = (p->slot[i].gen + 1u) & 0x7fffffu; *idx = i; return GSDF_OK; }
    p->slot_cv.wait(lk);
  }
}
static void slot_release(gsdf_program* p, int idx) {
  { std::lock_guard<std::mutex> lk(p->slot_mu); p->slot[idx].busy = false; }
  p->slot_cv.notify_one();
}

// Enqueue one host-buffer evaluation on a staging slot (no wait). Small calls (what the reference's renderers issue:
// <= 32768 points, gsdfaux.go:89,113) make no DMA round trips: the kernel reads the positions from -- and writes the
// distances to -- pinned, device-mapped host memory across PCIe itself: the caller's own buffers when they are registered
// (zero copy), else the slot's staging buffers (one memcpy in, one out).
static int eval_submit(gsdf_program* p, int dim, const void* pos, size_t stride, size_t n_pos, float* dist, size_t n_dist, int* ticket) {
  if (int rc = eval_args_refused(p, dim, pos, dist, n_pos, n_dist)) return rc;
  HIP_TRY(hipSetDevice(p->device));
  const size_t pbytes = n_pos * stride;
  int si = -1;
  int rc = slot_acquire(p, &si);
  if (rc) return rc;
  gsdf_program::Slot& sl = p->slot[si];
  auto bail = [&](int code) { slot_release(p, si); return code; };
  if (sl.s.ensure() != hipSuccess) return bail(fail(GSDF_ERR_HIP, "hipStreamCreate failed"));
  void* dp = reg_device_ptr(pos, pbytes);
  void* dd = dp ? reg_device_ptr(dist, n_pos * sizeof(float)) : nullptr;
  sl.zero_copy = dp && dd;
  sl.user_dist = dist;
  sl.n = n_pos;
  if (!sl.zero_copy) {
    if (pbytes > kSmallPos || n_pos > kSmallDist) return bail(fail(GSDF_ERR_BAD_ARGUMENT, "internal: large call on the small path"));
    if (!sl.h_pos.p && hipHostMalloc(&sl.h_pos.p, kSmallPos, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) return bail(fail(GSDF_ERR_HIP, "hipHostMalloc failed"));
    if (!sl.h_dist.p && hipHostMalloc((void**)&sl.h_dist.p, kSmallDist * sizeof(float), hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) return bail(fail(GSDF_ERR_HIP, "hipHostMalloc failed"));
    std::memcpy(sl.h_pos.p, pos, pbytes);
    if (hipHostGetDevicePointer(&dp, sl.h_pos.p, 0) != hipSuccess || hipHostGetDevicePointer(&dd, sl.h_dist.p, 0) != hipSuccess) return bail(fail(GSDF_ERR_HIP, "hipHostGetDevicePointer failed"));
  }
  spec_ensure(p, SPEC_EVAL_K1);  // (eval_kernel<D, 1, 4> of a specialised handle, at its first host-mapped call)
  rc = eval_dev(p, dim, dp, stride, (float*)dd, n_pos, sl.s.s, /*count=*/false, /*host_mapped=*/true);
  if (rc) return bail(rc);
  // completion flag behind the kernel (eval_wait polls it; hipStreamSynchronize remains the fallback)
  // (hipStreamWriteValue32 instead of the one-thread kernel was tried: slower, 38.7 vs 29.9 us per blocking pageable call)
  static const bool use_flag = env_flag_on("GSDF_HIP_EVAL_FLAG");  // developer knob (A/B timing)
  sl.flagged = false;
  if (use_flag) {
    if (!sl.h_flag.p) {
      void* hf = nullptr; void* df = nullptr;
      if (hipHostMalloc(&hf, 64, hipHostMallocMapped | hipHostMallocPortable) == hipSuccess && hipHostGetDevicePointer(&df, hf, 0) == hipSuccess) {
        sl.h_flag.p = (unsigned*)hf; sl.d_flag = (unsigned*)df; *sl.h_flag.p = 0u;
      } else { (void)hipGetLastError(); if (hf) (void)hipHostFree(hf); }
    }
    if (sl.h_flag.p) {
      sl.flag_val = sl.flag_val + 1u ? sl.flag_val + 1u : 1u;
      hipLaunchKernelGGL(signal_kernel, dim3(1), dim3(1), 0, sl.s.s, sl.d_flag, sl.flag_val);
      if (hipGetLastError() == hipSuccess) sl.flagged = true;
    }
  }
  p->evals_host.fetch_add(n_pos);
  *ticket = si | (int)(sl.gen << 8);
  return GSDF_OK;
}
static int eval_wait(gsdf_program* p, int tk) {
  const int ticket = tk & 0xff;
  if (!p || tk < 0 || ticket >= gsdf_program::kSlots) return fail(GSDF_ERR_BAD_ARGUMENT, "bad evaluation ticket");
  {  // the slot must be in flight for THIS ticket, and nobody else may be waiting on it
    std::lock_guard<std::mutex> lk(p->slot_mu);
    gsdf_program::Slot& s0 = p->slot[ticket];
    if (!s0.busy || s0.waiting || s0.gen != ((unsigned)tk >> 8)) return fail(GSDF_ERR_BAD_ARGUMENT, "bad evaluation ticket (stale, or waited for twice)");
    s0.waiting = true;
  }
  gsdf_program::Slot& sl = p->slot[ticket];
  hipError_t e = hipSuccess;
  bool done = false;
  if (sl.flagged) {  // poll the flag the stream writes behind the kernel: ~100 us of spinning at most, then the blocking wait
    const volatile unsigned* f = sl.h_flag.p;
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spin = 0;; spin++) {
      if (*f == sl.flag_val) { done = true; break; }
      __builtin_ia32_pause();
      if ((spin & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(200)) break;
    }
    std::atomic_thread_fence(std::memory_order_acquire);
  }
  if (!done) e = hipStreamSynchronize(sl.s.s);
  if (e == hipSuccess && !sl.zero_copy) std::memcpy(sl.user_dist, sl.h_dist.p, sl.n * sizeof(float));
  slot_release(p, ticket);
  if (e != hipSuccess) return fail(GSDF_ERR_HIP, std::string("hipStreamSynchronize: ") + hipGetErrorString(e));
  return GSDF_OK;
}

static int eval_host(gsdf_program* p, int dim, const void* pos, size_t stride, size_t n_pos, float* dist, size_t n_dist) {
  const size_t pbytes = n_pos * stride;
  const bool small = pbytes <= kSmallPos && n_pos <= kSmallDist;
  if (small || (pos && dist && n_pos == n_dist && n_pos && reg_device_ptr(pos, pbytes) && reg_device_ptr(dist, n_pos * sizeof(float)))) {
    int t = -1;
    const int rc = eval_submit(p, dim, pos, stride, n_pos, dist, n_dist, &t);
    return rc ? rc : eval_wait(p, t);  // (eval_submit checks the arguments, a null program first)
  }
  if (int rc = eval_args_refused(p, dim, pos, dist, n_pos, n_dist)) return rc;
  HIP_TRY(hipSetDevice(p->device));
  // large calls: DMA in, kernel, DMA out on the program's stream (one caller at a time, as before)
  static std::mutex big_mu;
  std::lock_guard<std::mutex> lk(big_mu);
  if (pbytes > p->cap_pos_bytes) {
    p->d_pos.reset();
    p->cap_pos_bytes = 0;
    HIP_TRY(hipMalloc(&p->d_pos.p, pbytes));
    p->cap_pos_bytes = pbytes;
  }
  if (n_pos > p->cap_dist) {
    p->d_dist.reset();
    p->cap_dist = 0;
    HIP_TRY(hipMalloc((void**)&p->d_dist.p, n_pos * sizeof(float)));
    p->cap_dist = n_pos;
  }
  HIP_TRY(hipMemcpyAsync(p->d_pos.p, pos, pbytes, hipMemcpyHostToDevice, p->stream.s));
  int rc = eval_dev(p, dim, p->d_pos.p, stride, p->d_dist.p, n_pos, p->stream.s);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(dist, p->d_dist.p, n_pos * sizeof(float), hipMemcpyDeviceToHost, p->stream.s));
  HIP_TRY(hipStreamSynchronize(p->stream.s));
  return GSDF_OK;
}

// Pipelined form of the host-buffer API: submit returns at once with a ticket (at most 4 in flight per program: a fifth
// submit waits for a free slot), wait blocks until that call's distances are in `dist`. For callers that can prepare the
// next batch while the previous one is on the GPU. Batches of up to 2^18 points (2^20 position bytes), or any size in
// registered memory.
extern "C" int gsdf_hip_eval3_submit(gsdf_program* p, const void* pos, size_t stride, size_t n_pos, float* dist, size_t n_dist, int* ticket) {
  if (!ticket) return fail(GSDF_ERR_BAD_ARGUMENT, "null ticket");
  if (n_pos * stride > kSmallPos || n_pos > kSmallDist) {
    if (!(pos && dist && reg_device_ptr(pos, n_pos * stride) && reg_device_ptr(dist, n_pos * sizeof(float))))
      return fail(GSDF_ERR_BAD_ARGUMENT, "submit takes at most 262144 points per call unless both buffers are registered host memory");
  }
  return eval_submit(p, 3, pos, stride, n_pos, dist, n_dist, ticket);
}
extern "C" int gsdf_hip_eval_wait(gsdf_program* p, int ticket) { return eval_wait(p, ticket); }

extern "C" int gsdf_hip_eval3(gsdf_program* p, const void* pos, size_t stride, size_t n_pos, float* dist, size_t n_dist) {
  return eval_host(p, 3, pos, stride, n_pos, dist, n_dist);
}
extern "C" int gsdf_hip_eval2(gsdf_program* p, const void* pos, size_t stride, size_t n_pos, float* dist, size_t n_dist) {
  return eval_host(p, 2, pos, stride, n_pos, dist, n_dist);
}
static int eval_dev_entry(gsdf_program* p, int dim, const void* d_pos, size_t stride, float* d_dist, size_t n, void* stream) {
  if (!p || !d_pos || !d_dist) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (n == 0) return fail(GSDF_ERR_EMPTY_BUFFERS, "empty buffers");
  if (int rc = eval_dim_refused(p, dim)) return rc;
  return eval_dev(p, dim, d_pos, stride, d_dist, n, stream ? (hipStream_t)stream : p->stream.s);
}
extern "C" int gsdf_hip_eval3_dev(gsdf_program* p, const void* d_pos, size_t stride, float* d_dist, size_t n, void* stream) {
  return eval_dev_entry(p, 3, d_pos, stride, d_dist, n, stream);
}
extern "C" int gsdf_hip_eval2_dev(gsdf_program* p, const void* d_pos, size_t stride, float* d_dist, size_t n, void* stream) {
  return eval_dev_entry(p, 2, d_pos, stride, d_dist, n, stream);
}

// gleval.NormalsCentralDiff on device-resident points, enqueued on the handle's stream: the checks (`what` names the caller in the
// text of a tree too large for two points per lane) and normals_kernel over the interpreter or the handle's build of it. The
// callers synchronise and count the 6 n evaluations.
static int normals_enqueue(gsdf_program* p, const float* d_pos, float* d_nrm, size_t n, float step, const char* what) {
  step *= 0.5f;
  if (!(step > 0)) return fail(GSDF_ERR_BAD_ARGUMENT, "invalid step");
  if (n == 0) return fail(GSDF_ERR_EMPTY_BUFFERS, "empty buffers");
  if (p->prog.is2d) return fail(GSDF_ERR_DIMENSION, "program is 2D");
  if (int rc = p->normals_refused(what)) return rc;
  HIP_TRY(hipSetDevice(p->device));
  spec_adopt(p);  // (a background build that has finished: its kernels from here on)
  spec_ensure(p, SPEC_AUX);
  if (launch_kernel(normals_kernel, p->spec.f_normals, grid_for(n, p->num_cu, 8), BLOCK, p->lds_bytes(2), p->stream.s, p->d_code.p, d_pos, d_nrm, n, step) != hipSuccess)
    return fail(GSDF_ERR_HIP, "normals kernel launch failed");
  return GSDF_OK;
}

// Host buffers, blocking. (The points go to the device ahead of the checks: a refused call has paid for the copy, no more.)
extern "C" int gsdf_hip_normals3(gsdf_program* p, const float* pos, float* normals, size_t n, float step) {
  if (!p || !pos || !normals) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(p->device));
  DevBuf d_p, d_n;
  HIP_TRY(d_p.alloc(n * 12));
  HIP_TRY(d_n.alloc(n * 12));
  if (hipMemcpyAsync(d_p.p, pos, n * 12, hipMemcpyHostToDevice, p->stream.s) != hipSuccess) return fail(GSDF_ERR_HIP, "H2D copy failed");
  if (int rc = normals_enqueue(p, (const float*)d_p.p, (float*)d_n.p, n, step, "gsdf_hip_normals3")) return rc;
  if (hipMemcpyAsync(normals, d_n.p, n * 12, hipMemcpyDeviceToHost, p->stream.s) != hipSuccess) return fail(GSDF_ERR_HIP, "D2H copy failed");
  if (hipStreamSynchronize(p->stream.s) != hipSuccess) return fail(GSDF_ERR_HIP, "stream sync failed");
  p->evals += 6 * n;
  return GSDF_OK;
}

// The same on device-resident points (gsdf_hip_indexed_normals: the welded vertices of a mesh): d_pos, d_nrm 12-byte xyz on the
// program's device; blocking. The launch is gsdf_hip_normals3's, so the values are.
int normals3_dev(gsdf_program* p, const float* d_pos, float* d_nrm, size_t n, float step) {
  if (int rc = normals_enqueue(p, d_pos, d_nrm, n, step, "the normals of an indexed mesh")) return rc;
  HIP_TRY(hipStreamSynchronize(p->stream.s));
  p->evals += 6 * n;
  return GSDF_OK;
}

// One kernel with counters on the handle's stream, blocking: `cl`'s counter block (C, made at the handle's first launch of the kind,
// as are the two events) is cleared in front of `launch(counters)` and copied to *hc behind it; the stream is synchronised whatever
// failed; *ms is the device time between the two events; the handle counts hc->evals. `what` goes in front of an error's text.
// One such call per program at a time, like every call on the handle's stream.
template <typename C, typename Launch>
static int counted_launch(gsdf_program* p, gsdf_program::CountedLaunch& cl, const char* what, C* hc, float* ms, Launch&& launch) {
  if (!cl.ctr.p) HIP_TRY(hipMalloc(&cl.ctr.p, sizeof(C)));
  HIP_TRY(cl.ev.ensure());
  C* d_ctr = (C*)cl.ctr.p;
  hipError_t e = hipMemsetAsync(d_ctr, 0, sizeof(C), p->stream.s);
  if (e == hipSuccess) e = hipEventRecord(cl.ev[0], p->stream.s);
  if (e == hipSuccess) e = launch(d_ctr);
  if (e == hipSuccess) e = hipEventRecord(cl.ev[1], p->stream.s);
  if (e == hipSuccess) e = hipMemcpyAsync(hc, d_ctr, sizeof(C), hipMemcpyDeviceToHost, p->stream.s);
  if (e == hipSuccess) e = hipStreamSynchronize(p->stream.s);
  else (void)hipStreamSynchronize(p->stream.s);
  if (e == hipSuccess) e = hipEventElapsedTime(ms, cl.ev[0], cl.ev[1]);
  if (e != hipSuccess) return fail(GSDF_ERR_HIP, std::string(what) + hipGetErrorString(e));
  p->evals += hc->evals;
  return GSDF_OK;
}

// gsdf_hip_indexed_project's kernel on device-resident points (abi_program.h): project_kernel over the interpreter, or the handle's
// specialised build of it, as one counted launch.
int project_dev(gsdf_program* p, const float* d_pos, size_t n, const gsdf_project_opts* o, float* d_out_pos, float* d_before, float* d_after,
                uint8_t* d_status, gsdf_project_stats* st) {
  if (n == 0) return fail(GSDF_ERR_EMPTY_BUFFERS, "empty buffers");
  if (n >= ((size_t)1 << 32)) return fail(GSDF_ERR_CAPACITY, "project: vertices must stay below 2^32");
  if (p->prog.is2d) return fail(GSDF_ERR_DIMENSION, "program is 2D");
  if (int rc = p->normals_refused("gsdf_hip_indexed_project")) return rc;
  HIP_TRY(hipSetDevice(p->device));
  spec_adopt(p);
  spec_ensure(p, SPEC_PROJECT);
  ProjectCounters hc{};
  float ms = 0.f;
  const unsigned grid = (unsigned)((n + BLOCK - 1) / BLOCK);
  const float h = o->step * 0.5f;
  // (the kernel takes the positions as words: (const unsigned*) cannot be left to the launcher's static_cast)
  if (int rc = counted_launch(p, p->proj, "project: ", &hc, &ms, [&](ProjectCounters* d_ctr) {
        return launch_kernel(project_kernel, p->spec.f_project, grid, BLOCK, p->lds_bytes(2), p->stream.s, p->d_code.p, (const unsigned*)d_pos, n, h, o->tol, o->max_move, o->max_iters,
                             (unsigned*)d_out_pos, d_before, d_after, d_status, d_ctr);
      }))
    return rc;
  gsdf_project_stats r{};
  r.n_verts = n;
  for (int k = 0; k < 8; k++) r.count[k] = hc.count[k];
  r.evals = hc.evals; r.over_tol_before = hc.over_before; r.over_tol_after = hc.over_after;
  std::memcpy(&r.max_abs_before, &hc.max_before, 4);
  std::memcpy(&r.max_abs_after, &hc.max_after, 4);
  r.steps_max = hc.steps_max;
  r.ms_device = (double)ms;
  *st = r;
  return GSDF_OK;
}

// ---- rays (kernels_ray.h; gsdf_hip.h: "rays") -------------------------------------------------------------------------------------
int ray_opts_refused(const gsdf_ray_opts* o, const char* what) {
  const std::string w = std::string(what) + ": ";
  if (!std::isfinite(o->t0) || !(o->t0 >= 0.0f)) return fail(GSDF_ERR_BAD_ARGUMENT, w + "t0 must be finite and not negative");
  if (!(o->tmax >= o->t0)) return fail(GSDF_ERR_BAD_ARGUMENT, w + "tmax must be t0 at least");
  if (!std::isfinite(o->tol) || !(o->tol >= 0.0f)) return fail(GSDF_ERR_BAD_ARGUMENT, w + "tol must be finite and not negative");
  if (!std::isfinite(o->min_step) || !(o->min_step >= 0.0f)) return fail(GSDF_ERR_BAD_ARGUMENT, w + "min_step must be finite and not negative");
  if (o->max_steps < 1 || o->max_steps > 4096) return fail(GSDF_ERR_BAD_ARGUMENT, w + "max_steps must be 1 .. 4096");
  if (o->refine < 0 || o->refine > 32) return fail(GSDF_ERR_BAD_ARGUMENT, w + "refine must be 0 .. 32");
  if (o->flags != 0) return fail(GSDF_ERR_BAD_ARGUMENT, w + "unknown flags " + std::to_string(o->flags));
  if (o->reserved != 0) return fail(GSDF_ERR_BAD_ARGUMENT, w + "the reserved word must be 0");
  return GSDF_OK;
}

// what both entry points refuse whatever the options: no rays, too many, a 2-D program
static int ray_call_refused(const gsdf_program* p, size_t n) {
  if (n == 0) return fail(GSDF_ERR_EMPTY_BUFFERS, "empty buffers");
  if (n >= ((size_t)1 << 32)) return fail(GSDF_ERR_CAPACITY, "rays must stay below 2^32");
  if (p->prog.is2d) return fail(GSDF_ERR_DIMENSION, "rays: the program is 2D");
  return GSDF_OK;
}

// ray_kernel on device-resident rays, or on device-resident vertices (step > 0: the thickness form), over the interpreter or the
// handle's specialised build of it (abi_program.h), as one counted launch.
int ray_dev(gsdf_program* p, const float* d_in, size_t n, const gsdf_ray_opts* o, float step, float thin, float* d_t, float* d_d, uint8_t* d_status,
            uint16_t* d_steps, gsdf_ray_stats* st) {
  const bool thick = step > 0.0f;
  if (int rc = ray_call_refused(p, n)) return rc;
  if (thick) { if (int rc = p->normals_refused("gsdf_hip_indexed_thickness")) return rc; }
  HIP_TRY(hipSetDevice(p->device));
  spec_adopt(p);
  spec_ensure(p, SPEC_RAY);
  RayCounters hc{};
  float ms = 0.f;
  const unsigned grid = (unsigned)((n + BLOCK - 1) / BLOCK);
  RayParams prm{};
  prm.t0 = o->t0 + 0.0f;  // (-0 -> +0: every t a ray reports is then >= +0)
  prm.tmax = o->tmax; prm.tol = o->tol; prm.min_step = o->min_step;
  prm.h = step * 0.5f; prm.thin = thin;
  prm.max_steps = o->max_steps; prm.refine = o->refine;
  // (the kernel takes its input as words: (const unsigned*) cannot be left to the launcher's static_cast)
  if (int rc = counted_launch(p, p->ray, "rays: ", &hc, &ms, [&](RayCounters* d_ctr) {
        if (thick)
          return launch_kernel(ray_kernel<true>, p->spec.f_ray_thick, grid, BLOCK, p->lds_bytes(2), p->stream.s, p->d_code.p, (const unsigned*)d_in, n, prm, d_t, d_d, d_status,
                               (unsigned short*)d_steps, d_ctr);
        return launch_kernel(ray_kernel<false>, p->spec.f_ray, grid, BLOCK, p->lds_bytes(1), p->stream.s, p->d_code.p, (const unsigned*)d_in, n, prm, d_t, d_d, d_status,
                             (unsigned short*)d_steps, d_ctr);
      }))
    return rc;
  gsdf_ray_stats r{};
  r.n = n;
  for (int k = 0; k < 8; k++) r.count[k] = hc.count[k];
  r.evals = hc.evals; r.steps_max = hc.steps_max; r.below = hc.below;
  const unsigned tmin = RAY_INF - hc.t_min_inv;
  std::memcpy(&r.t_min, &tmin, 4);
  std::memcpy(&r.t_max, &hc.t_max, 4);
  r.ms_device = (double)ms;
  *st = r;
  return GSDF_OK;
}

// Host buffers, blocking, on the path gsdf_hip_normals3 takes: the rays in, the kernel, the outputs the caller asked for out.
extern "C" int gsdf_hip_raycast3(gsdf_program* p, const float* rays, size_t n, const gsdf_ray_opts* o, float thin, float* t_out, float* d_out, uint8_t* status_out,
                                 uint16_t* steps_out, gsdf_ray_stats* st) {
  if (!p || !rays || !o) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (!t_out && !d_out && !status_out && !steps_out && !st) return fail(GSDF_ERR_BAD_ARGUMENT, "raycast: no output asked for");
  if (int rc = ray_opts_refused(o, "raycast")) return rc;
  if (int rc = ray_call_refused(p, n)) return rc;  // (before anything is allocated; ray_dev asks again)
  HIP_TRY(hipSetDevice(p->device));
  DevBuf d_rays, d_t, d_d, d_s, d_n;
  HIP_TRY(d_rays.alloc(n * 24));
  if (t_out) HIP_TRY(d_t.alloc(n * 4));
  if (d_out) HIP_TRY(d_d.alloc(n * 4));
  if (status_out) HIP_TRY(d_s.alloc(n));
  if (steps_out) HIP_TRY(d_n.alloc(n * 2));
  HIP_TRY(hipMemcpyAsync(d_rays.p, rays, n * 24, hipMemcpyHostToDevice, p->stream.s));
  gsdf_ray_stats r{};
  if (int rc = ray_dev(p, (const float*)d_rays.p, n, o, 0.0f, thin, (float*)d_t.p, (float*)d_d.p, (uint8_t*)d_s.p, (uint16_t*)d_n.p, &r)) return rc;
  if (t_out) HIP_TRY(hipMemcpy(t_out, d_t.p, n * 4, hipMemcpyDeviceToHost));
  if (d_out) HIP_TRY(hipMemcpy(d_out, d_d.p, n * 4, hipMemcpyDeviceToHost));
  if (status_out) HIP_TRY(hipMemcpy(status_out, d_s.p, n, hipMemcpyDeviceToHost));
  if (steps_out) HIP_TRY(hipMemcpy(steps_out, d_n.p, n * 2, hipMemcpyDeviceToHost));
  if (st) *st = r;
  return GSDF_OK;
}

// ---- 2-D images (kernels_image.h) ---------------------------------------------------------------------------------------------------
// The pixel lattice of both renderers over Bounds(), image.go:82-88: dx = sz.X/dxi ; bb.Min += (dx/2, dy/2) ; y = bb.Max.Y - j*dy ;
// x = i*dx + bb.Min.X. k points per lane on `grid` workgroups.
struct ImageLattice {
  float dx, dy, xmin, ymax;
  size_t n;
  int k;
  unsigned grid;
};
static ImageLattice image_lattice(const gsdf_program* p, int w, int h) {
  ImageLattice l;
  l.n = (size_t)w * (size_t)h;
  const float szx = p->prog.bb[3] - p->prog.bb[0], szy = p->prog.bb[4] - p->prog.bb[1];
  l.dx = szx / (float)w; l.dy = szy / (float)h;
  l.xmin = p->prog.bb[0] + l.dx / 2; l.ymax = p->prog.bb[4];
  l.k = p->batch_k();
  l.grid = grid_for((l.n + l.k - 1) / l.k, p->num_cu, 8);
  return l;
}
// behind the kernel: the planes the caller asked for to the host, one synchronise, n evaluations counted
static int image_finish(gsdf_program* p, size_t n, float* dist_out, const void* d_dist, uint8_t* rgba_out, const void* d_rgba) {
  if (dist_out) HIP_TRY(hipMemcpyAsync(dist_out, d_dist, n * 4, hipMemcpyDeviceToHost, p->stream.s));
  if (rgba_out) HIP_TRY(hipMemcpyAsync(rgba_out, d_rgba, n * 4, hipMemcpyDeviceToHost, p->stream.s));
  HIP_TRY(hipStreamSynchronize(p->stream.s));
  p->evals += n;
  return GSDF_OK;
}

// glrender.ImageRendererSDF2.Render for a 2D program: w x h pixels over Bounds(); host outputs (either may be NULL).
extern "C" int gsdf_hip_image2(gsdf_program* p, int w, int h, float* dist_out, uint8_t* rgba_out) {
  if (!p) return fail(GSDF_ERR_BAD_ARGUMENT, "null program");
  if (!p->prog.is2d) return fail(GSDF_ERR_DIMENSION, "program is 3D, image2 called");
  if (w <= 0 || h <= 0) return fail(GSDF_ERR_BAD_ARGUMENT, "bad image size");
  HIP_TRY(hipSetDevice(p->device));
  spec_adopt(p);  // (a background build that has finished: its kernels from here on)
  const ImageLattice l = image_lattice(p, w, h);
  DevBuf dd, dc;  // (both planes, whichever the caller takes)
  HIP_TRY(dd.alloc(l.n * 4));
  HIP_TRY(dc.alloc(l.n * 4));
  spec_ensure(p, SPEC_AUX);
  HIP_TRY(launch_kernel(l.k == 4 ? image2_kernel<4> : (l.k == 2 ? image2_kernel<2> : image2_kernel<1>), p->spec.f_image, l.grid, BLOCK, p->lds_bytes(l.k), p->stream.s, p->d_code.p, w, h,
                        l.xmin, l.ymax, l.dx, l.dy, dd.p, dc.p));
  return image_finish(p, l.n, dist_out, dd.p, rgba_out, dc.p);
}

// ---- the UI's view of a 3-D part (gsdfaux.UI, gsdfaux/ui.go:247-355): the frame (the orbit camera: abi_evalhost.cpp) ----------------
// One UI frame (ui.go:247-355) of a 3-D program: view_kernel over the interpreter, or the handle's specialised build of it.
// The plain form runs by default: measured against the refilling one (tools/view_bench.py, profiles/view_*), it is 1.3-2x faster on
// every frame tried. GSDF_HIP_VIEW_REFILL=1 (read at every call; developer knob for the A/B and its parity
// test) runs the refilling form.
extern "C" int gsdf_hip_render3(gsdf_program* p, const gsdf_view* view, int w, int h, uint8_t* rgba_out, float* depth_out, uint32_t* evals_out) {
  if (!p || !view) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (p->prog.is2d) return fail(GSDF_ERR_DIMENSION, "program is 2D, render3 called");
  if (w <= 0 || h <= 0 || w > 16384 || h > 16384) return fail(GSDF_ERR_BAD_ARGUMENT, "bad image size (1 .. 16384 pixels per side)");
  if (view->aa < 1 || view->aa > 8) return fail(GSDF_ERR_BAD_ARGUMENT, "aa must be 1 .. 8");
  if (view->max_steps < 0 || view->max_steps > 4096) return fail(GSDF_ERR_BAD_ARGUMENT, "max_steps must be 0 .. 4096");
  if (!finite_all(view->ro, 3) || !finite_all(view->uu, 3) || !finite_all(view->vv, 3) || !finite_all(view->ww, 3) || !std::isfinite(view->char_dist))
    return fail(GSDF_ERR_BAD_ARGUMENT, "non-finite camera");
  const size_t n = (size_t)w * (size_t)h;
  if (view->max_steps == 0) {  // no sample marches: nothing hits, nothing is evaluated
    for (size_t i = 0; i < n; i++) {
      if (rgba_out) { rgba_out[4 * i] = rgba_out[4 * i + 1] = rgba_out[4 * i + 2] = 0; rgba_out[4 * i + 3] = 255; }
      if (depth_out) depth_out[i] = INFINITY;
      if (evals_out) evals_out[i] = 0;
    }
    return GSDF_OK;
  }
  HIP_TRY(hipSetDevice(p->device));
  spec_adopt(p);  // (a background build that has finished: its kernels from here on)
  spec_ensure(p, SPEC_VIEW);
  ViewCam cam;
  for (int a = 0; a < 3; a++) { cam.ro[a] = view->ro[a]; cam.uu[a] = view->uu[a]; cam.vv[a] = view->vv[a]; cam.ww[a] = view->ww[a]; }
  cam.tmax = 1.3f * view->char_dist;
  cam.aa = view->aa; cam.max_steps = view->max_steps; cam.w = w; cam.h = h;
  cam.tiles_x = (unsigned)((w + VIEW_TILE - 1) / VIEW_TILE);
  cam.n_claims = cam.tiles_x * (unsigned)((h + VIEW_TILE - 1) / VIEW_TILE) * VIEW_TILE * VIEW_TILE;
  DevBuf d_rgba, d_depth, d_evals, d_ctr;
  HIP_TRY(d_rgba.alloc(n * 4));
  HIP_TRY(d_depth.alloc(n * 4));
  HIP_TRY(d_evals.alloc(n * 4));
  HIP_TRY(d_ctr.alloc(16));
  HIP_TRY(hipMemsetAsync(d_ctr.p, 0, 16, p->stream.s));
  const bool plain = !env_flag("GSDF_HIP_VIEW_REFILL");
  const size_t lds = p->lds_bytes(1);
  // plain: one lane per claim; refilling: persistent, as many workgroups as the CUs hold at once (4 per CU: the launch bounds)
  unsigned grid = (cam.n_claims + BLOCK - 1) / BLOCK;
  if (!plain) {
    const unsigned per_cu = std::max(1u, std::min(4u, (unsigned)((size_t)160 * 1024 / (lds + 64))));
    grid = std::min(grid, (unsigned)p->num_cu * per_cu);
  }
  uint32_t* o_rgba = (uint32_t*)d_rgba.p;
  float* o_depth = (float*)d_depth.p;
  uint32_t* o_evals = (uint32_t*)d_evals.p;
  unsigned long long* o_ctr = (unsigned long long*)d_ctr.p;
  HIP_TRY(launch_kernel(plain ? view_kernel<false> : view_kernel<true>, plain ? p->spec.f_view_plain : p->spec.f_view, grid, BLOCK, lds, p->stream.s, p->d_code.p, cam, o_rgba, o_depth, o_evals,
                        o_ctr));
  unsigned long long h_ctr[2] = {0, 0};
  if (rgba_out) HIP_TRY(hipMemcpyAsync(rgba_out, d_rgba.p, n * 4, hipMemcpyDeviceToHost, p->stream.s));
  if (depth_out) HIP_TRY(hipMemcpyAsync(depth_out, d_depth.p, n * 4, hipMemcpyDeviceToHost, p->stream.s));
  if (evals_out) HIP_TRY(hipMemcpyAsync(evals_out, d_evals.p, n * 4, hipMemcpyDeviceToHost, p->stream.s));
  HIP_TRY(hipMemcpyAsync(h_ctr, d_ctr.p, 16, hipMemcpyDeviceToHost, p->stream.s));
  HIP_TRY(hipStreamSynchronize(p->stream.s));
  p->evals += h_ctr[1];
  return GSDF_OK;
}

// ---- a 2-D part's picture with gsdfaux's colour conversions (gsdfaux.RenderPNGFile, gsdfaux/gsdfaux.go:264-296; color.go) --------
// (the picture size and the conversions' constructors: abi_evalhost.cpp)
// ImageRendererSDF2.Render (image.go:76-118) with a conversion of gsdfaux: image2_color_kernel over the interpreter (the kind a
// kernel argument), or the handle's specialised build of it (one kernel per kind).
extern "C" int gsdf_hip_image2_color(gsdf_program* p, const gsdf_color2* conv, int w, int h, uint8_t* rgba_out, float* dist_out) {
  if (!p || !conv) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (!p->prog.is2d) return fail(GSDF_ERR_DIMENSION, "program is 3D, image2_color called");
  if (w <= 0 || h <= 0 || w > 16384 || h > 16384) return fail(GSDF_ERR_BAD_ARGUMENT, "bad image size (1 .. 16384 pixels per side)");
  if (conv->kind < GSDF_COLOR_DEFAULT || conv->kind > GSDF_COLOR_BW_SMOOTH) return fail(GSDF_ERR_BAD_ARGUMENT, "unknown colour conversion");
  if (conv->reserved[0] || conv->reserved[1] || conv->reserved[2] || conv->reserved[3]) return fail(GSDF_ERR_BAD_ARGUMENT, "reserved words must be 0");
  if (!std::isfinite(conv->length)) return fail(GSDF_ERR_BAD_ARGUMENT, "non-finite conversion length");
  if (conv->kind == GSDF_COLOR_IQ && !(conv->length > 0.f)) return fail(GSDF_ERR_BAD_ARGUMENT, "IQ characteristic distance must be > 0");
  if ((conv->kind == GSDF_COLOR_GRADIENT || conv->kind == GSDF_COLOR_BW_SMOOTH) && conv->length < 0.f)
    return fail(GSDF_ERR_BAD_ARGUMENT, "gradient length must be >= 0");
  HIP_TRY(hipSetDevice(p->device));
  spec_adopt(p);  // (a background build that has finished: its kernels from here on)
  spec_ensure(p, SPEC_PICTURE);
  const ImageLattice l = image_lattice(p, w, h);
  ColorConv cv;
  cv.kind = conv->kind;
  cv.length = conv->length;
  cv.c0 = (uint32_t)conv->c0[0] | ((uint32_t)conv->c0[1] << 8) | ((uint32_t)conv->c0[2] << 16) | ((uint32_t)conv->c0[3] << 24);
  cv.c1 = (uint32_t)conv->c1[0] | ((uint32_t)conv->c1[1] << 8) | ((uint32_t)conv->c1[2] << 16) | ((uint32_t)conv->c1[3] << 24);
  DevBuf dd, dc;  // (an output not asked for is neither allocated nor written)
  if (dist_out) HIP_TRY(dd.alloc(l.n * 4));
  if (rgba_out) HIP_TRY(dc.alloc(l.n * 4));
  float* o_dist = dist_out ? (float*)dd.p : nullptr;
  uint32_t* o_rgba = rgba_out ? (uint32_t*)dc.p : nullptr;
  // (the interpreter's kernel takes the conversion kind as an argument, a per-tree one is built for its kind)
  HIP_TRY(launch_kernel(l.k == 4 ? image2_color_kernel<4, -1> : (l.k == 2 ? image2_color_kernel<2, -1> : image2_color_kernel<1, -1>), p->spec.f_imgc[conv->kind], l.grid, BLOCK,
                        p->lds_bytes(l.k), p->stream.s, p->d_code.p, w, h, l.xmin, l.ymax, l.dx, l.dy, cv, o_dist, o_rgba));
  return image_finish(p, l.n, dist_out, dd.p, rgba_out, dc.p);
}
