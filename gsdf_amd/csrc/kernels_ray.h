// kernels_ray.h -- rays sphere-traced through the field of a 3-D program, from outside or inside the part, and the wall thickness of
// an indexed mesh (the same march along the inward normal of every vertex): ray_kernel. The exact float32 arithmetic per ray is
// stated in include/gsdf_hip.h ("rays"); tests/rayref.py is its CPU twin.
//
// Not part of kernels.h: abi_eval.hip includes this header for the ahead-of-time (interpreter) kernels, and a specialised handle builds
// ray_kernel in a module of its own at its first cast (abi_spec.hip: spec_ensure, SPEC_RAY; specialize.cpp: spec_includes).
//
// One ray per lane, the wave in lockstep: every trip through the loop builds one position per lane from the lane's state -- the next
// point of the march, or the midpoint of a crossing's bracket -- and makes ONE sdf_eval<1> call with all 64 lanes active (the
// evaluator's control flow is wave-uniform and each lane owns an LDS column). A finished lane re-evaluates its last position, a
// skipped lane and a padding lane the origin, and the value is dropped. A wave leaves when none of its lanes is live. No refill: the
// plain form measured faster for the view.
//   THICK = false  the lane's ray is read from memory (24 bytes: origin, direction).
//   THICK = true   the lane's vertex is read (12 bytes) and the ray is built in registers: normals_kernel's six taps as three
//                  sdf_eval<2> (two points per lane: lds_bytes(2)), the direction the inward unit normal; t_out receives the thickness.
// The counters leave by ballot + popcount (the evaluations: summed per trip in a wave-uniform register), the extremes by a wave
// reduction; the workgroup's waves add up in LDS and the workgroup issues one global atomic per counter, every one of them an integer
// sum or maximum.
#pragma once
#include "kernels_common.h"

// status of a ray (gsdf_hip.h: GSDF_RAY_*)
#define RAY_SKIPPED 0u
#define RAY_HIT 1u
#define RAY_CROSSED 2u
#define RAY_MISS 3u
#define RAY_STEPS 4u
#define RAY_NONFINITE 5u
#define RAY_FLAT 6u
#define RAY_NOT_EVALUATED 0x7fc00000u  // t and d of a SKIPPED ray; d of a NONFINITE one
#define RAY_INF 0x7f800000u
#define RAY_ACC 13u  // words of the workgroup's counters in LDS

// the options as the kernel takes them (abi_eval.hip: ray_dev fills it from a gsdf_ray_opts)
struct RayParams {
  float t0, tmax, tol, min_step;
  float h;     // THICK: half the central-difference step
  float thin;  // the counter `below`: t < thin
  int max_steps, refine;
};

// gsdf_ray_stats' leading block behind n (abi_eval.hip: ray_dev copies it over)
struct RayCounters {
  unsigned long long count[8];
  unsigned long long evals;
  unsigned long long below;
  unsigned steps_max;
  unsigned t_min_inv;  // the largest RAY_INF - bits(t): the smallest t, and +Inf where no ray counted (cleared to 0 with the rest)
  unsigned t_max;      // bits of the largest t
  unsigned pad;
};

namespace ray {
using nb::abs_bits; using nb::is_nan; using nb::abs_gt; using nb::wave_max_u32;  // (kernels_common.h; NaN by its bits: -fno-honor-nans)
__device__ __forceinline__ bool lt(float a, float b) { return !is_nan(a) && !is_nan(b) && a < b; }
__device__ __forceinline__ bool gt(float a, float b) { return !is_nan(a) && !is_nan(b) && a > b; }
__device__ __forceinline__ bool neg(float v) { return (__float_as_uint(v) >> 31) != 0u; }
__device__ __forceinline__ void wave_count(bool flag, unsigned* counter, bool lead) {
  const unsigned long long m = __ballot(flag);
  if (lead && m) atomicAdd(counter, (unsigned)__builtin_popcountll(m));
}
}  // namespace ray

// in: 6 n floats (THICK: 3 n), as words. t_out, d_out (n floats), status (n bytes), steps (n uint16): each may be null (a dry run
// passes none).
template <bool THICK>
__global__ void __launch_bounds__(BLOCK, 4) ray_kernel(const uint32_t* __restrict__ code_g, const unsigned* __restrict__ in, uint64_t n, RayParams prm,
                                                       float* __restrict__ t_out, float* __restrict__ d_out, unsigned char* __restrict__ status,
                                                       unsigned short* __restrict__ steps, RayCounters* __restrict__ ctr) {
  using namespace ray;
  code_ptr code = as_code(code_g);
  float* lds = g_smem + threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool valid = i < n;
  float ox = 0.f, oy = 0.f, oz = 0.f, rx = 0.f, ry = 0.f, rz = 0.f;
  if (valid) {
    const unsigned* q = in + (THICK ? 3 : 6) * i;
    ox = __uint_as_float(q[0]); oy = __uint_as_float(q[1]); oz = __uint_as_float(q[2]);
    if (!THICK) { rx = __uint_as_float(q[3]); ry = __uint_as_float(q[4]); rz = __uint_as_float(q[5]); }
  }
  bool live = valid && !nb::nan_or_inf(ox) && !nb::nan_or_inf(oy) && !nb::nan_or_inf(oz) && !nb::nan_or_inf(rx) && !nb::nan_or_inf(ry) && !nb::nan_or_inf(rz);
  if (!live) { ox = oy = oz = 0.f; rx = ry = rz = 0.f; }
  unsigned st = RAY_SKIPPED;
  unsigned wave_evals = 0u;  // wave-uniform: at most 64 lanes x (6 + 4096 + 32) evaluations
  if (THICK) {               // the ray of a vertex: o = x, r = the inward unit normal (normals_kernel's taps)
    wave_evals += 6u * (unsigned)__builtin_popcountll(__ballot(live));
    float g[3];
#pragma unroll 1
    for (int dim = 0; dim < 3; dim++) {
      P3 a = {ox + (dim == 0 ? prm.h : 0.f), oy + (dim == 1 ? prm.h : 0.f), oz + (dim == 2 ? prm.h : 0.f)};
      P3 b = {ox - (dim == 0 ? prm.h : 0.f), oy - (dim == 1 ? prm.h : 0.f), oz - (dim == 2 ? prm.h : 0.f)};
      P3 ab[2] = {a, b};
      float dd[2];
      gsdf_dev::sdf_eval<2>(code, ab, dd, lds, BLOCK);
      const float v = dd[0] - dd[1];
      if (dim == 0) g[0] = v; else if (dim == 1) g[1] = v; else g[2] = v;
    }
    if (live) {
      const float s = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];
      if (!__builtin_amdgcn_classf(s, 0x380)) { st = RAY_FLAT; live = false; }  // NOT (s > 0): +subnormal, +normal, +inf pass
      else {
        const float len = __builtin_sqrtf(s);
        rx = -(g[0] / len); ry = -(g[1] / len); rz = -(g[2] / len);
      }
    }
  }
  const unsigned tol_bits = abs_bits(prm.tol);
  const float nanv = __uint_as_float(RAY_NOT_EVALUATED);
  float t = nanv, d = nanv;  // what the ray reports
  float te = prm.t0;         // where the lane evaluates next
  float a = 0.f, b = 0.f, db = 0.f;  // a crossing's bracket
  bool inside = false, refining = false;
  unsigned nmarch = 0u, nref = 0u;
#pragma unroll 1
  for (;;) {
    const unsigned long long m1 = __ballot(live);
    if (m1 == 0ull) break;
    wave_evals += (unsigned)__builtin_popcountll(m1);
    P3 p[1] = {P3{ox + te * rx, oy + te * ry, oz + te * rz}};
    float dv1[1];
    gsdf_dev::sdf_eval<1>(code, p, dv1, lds, BLOCK);
    if (!live) continue;
    const float dv = dv1[0];
    bool bisect = false;  // the lane goes on to the next midpoint of its bracket, or ends there
    if (!refining) {
      nmarch++;
      if (is_nan(dv)) { st = RAY_NONFINITE; t = te; d = nanv; live = false; }
      else if (!abs_gt(dv, tol_bits)) { st = RAY_HIT; t = te; d = dv; live = false; }
      else {
        if (nmarch == 1u) inside = neg(dv);
        if (neg(dv) != inside) { st = RAY_CROSSED; a = t; b = te; db = dv; refining = true; bisect = true; }  // (t: the point before, tp)
        else if (nmarch >= (unsigned)prm.max_steps) { st = RAY_STEPS; t = te; d = dv; live = false; }
        else {
          t = te; d = dv;  // tp, dp
          float s = __uint_as_float(abs_bits(dv));
          if (s < prm.min_step) s = prm.min_step;
          const float tn = t + s;
          if (tn > prm.tmax) { st = RAY_MISS; live = false; }
          else te = tn;
        }
      }
    } else {
      nref++;
      if (is_nan(dv)) { t = b; d = db; live = false; }
      else if (!abs_gt(dv, tol_bits)) { t = te; d = dv; live = false; }
      else {
        if (neg(dv) == inside) a = te; else { b = te; db = dv; }
        bisect = true;
      }
    }
    if (bisect) {
      const float m = a + (b - a) * 0.5f;
      if (nref >= (unsigned)prm.refine || !(gt(m, a) && lt(m, b))) { t = b; d = db; live = false; }
      else te = m;
    }
  }
  const bool found = st == RAY_HIT || st == RAY_CROSSED;
  if (valid) {
    if (t_out) t_out[i] = !THICK || found ? t : __uint_as_float(st == RAY_MISS ? RAY_INF : RAY_NOT_EVALUATED);
    if (d_out) d_out[i] = d;
    if (status) status[i] = (unsigned char)st;
    if (steps) steps[i] = (unsigned short)(nmarch + nref);
  }
  // counters: the waves of a workgroup sum in LDS (the evaluator's columns are free once every wave is through), then one global
  // atomic per workgroup and counter that has something to add -- and for a maximum only where a plain load says it would still
  // raise it. Every counter is one 128-byte line of L2: one atomic per WAVE and counter serialised there and cost as much as the march
  // itself.
  unsigned* acc = (unsigned*)g_smem;  // [0..7] count, [8] evals, [9] below, [10] steps_max, [11] t_min_inv, [12] t_max
  __syncthreads();
  if (threadIdx.x < RAY_ACC) acc[threadIdx.x] = 0u;
  __syncthreads();
  const bool lead = (threadIdx.x & 63u) == 0u;
#pragma unroll 1
  for (unsigned k = 0; k < 8u; k++) wave_count(valid && st == k, &acc[k], lead);
  wave_count(found && lt(t, prm.thin), &acc[9], lead);
  const unsigned tb = __float_as_uint(t);  // (found: 0 <= t <= +Inf, its bits order as unsigned integers)
  const unsigned mn = wave_max_u32(found ? RAY_INF - tb : 0u);
  const unsigned mx = wave_max_u32(found ? tb : 0u);
  const unsigned ms = wave_max_u32(nmarch + nref);
  if (lead) {
    if (wave_evals) atomicAdd(&acc[8], wave_evals);  // (a workgroup: at most 256 x (6 + 4096 + 32) evaluations)
    if (ms) atomicMax(&acc[10], ms);
    if (mn) atomicMax(&acc[11], mn);
    if (mx) atomicMax(&acc[12], mx);
  }
  __syncthreads();
  if (threadIdx.x < RAY_ACC) {
    const unsigned v = acc[threadIdx.x], k = threadIdx.x;
    if (v) {
      if (k < 8u) atomicAdd(&ctr->count[k], (unsigned long long)v);
      else if (k == 8u) atomicAdd(&ctr->evals, (unsigned long long)v);
      else if (k == 9u) atomicAdd(&ctr->below, (unsigned long long)v);
      else {
        unsigned* dst = k == 10u ? &ctr->steps_max : (k == 11u ? &ctr->t_min_inv : &ctr->t_max);
        if (__hip_atomic_load(dst, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < v) atomicMax(dst, v);
      }
    }
  }
}
