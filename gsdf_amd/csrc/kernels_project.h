// kernels_project.h -- the vertices of an indexed mesh projected onto the field of the program that made it: project_kernel. The
// exact float32 arithmetic per vertex is stated in include/gsdf_hip.h ("indexed meshes: project onto the field"); tests/projectref.py
// is its CPU twin.
//
// Not part of kernels.h: abi_eval.hip includes this header for the ahead-of-time (interpreter) kernel, and a specialised handle builds
// project_kernel in a module of its own at its first projection (abi_eval.hip: spec_project; specialize.cpp: spec_includes).
//
// One vertex per lane, the wave in lockstep per Newton trip: one sdf_eval<1> of the lanes' positions, a ballot whether any lane goes
// on to a gradient, then the six taps as three sdf_eval<2> (normals_kernel's points and subtraction). The evaluator's control flow is
// wave-uniform and each lane owns an LDS column, so all 64 lanes stay active throughout: a finished lane, a lane whose vertex is
// skipped and a padding lane evaluate a position of their own (their last one; the origin) and the value is dropped. A wave leaves
// when none of its lanes is live. The counters leave by ballot + popcount (the evaluations: summed per trip in a wave-uniform
// register), the maxima by a wave reduction: one atomic per wave and counter, every one of them an integer sum or maximum.
#pragma once
#include "kernels_common.h"

// status of a vertex (gsdf_hip.h: GSDF_PROJECT_*)
#define PROJECT_SKIPPED 0u
#define PROJECT_ON 1u
#define PROJECT_CONVERGED 2u
#define PROJECT_ITERS 3u
#define PROJECT_FLAT 4u
#define PROJECT_CLAMPED 5u
#define PROJECT_NONFINITE 6u
#define PROJECT_REVERTED 7u
#define PROJECT_MAX_ITERS 64
#define PROJECT_NOT_EVALUATED 0x7fc00000u  // d_before / d_after of a SKIPPED vertex

// gsdf_project_stats' leading block behind n_verts (abi_eval.hip: project_dev copies it over)
struct ProjectCounters {
  unsigned long long count[8];
  unsigned long long evals;
  unsigned long long over_before, over_after;
  unsigned max_before, max_after;  // bits of the largest non-NaN |d|
  unsigned steps_max, pad;
};

namespace project {
using nb::abs_bits; using nb::is_nan; using nb::abs_gt; using nb::wave_max_u32;  // (kernels_common.h)
__device__ __forceinline__ void wave_count(bool flag, unsigned long long* counter) {
  const unsigned long long m = __ballot(flag);
  if ((threadIdx.x & 63u) == 0u && m) atomicAdd(counter, (unsigned long long)__builtin_popcountll(m));
}
}  // namespace project

// pos: 3 n floats. out_pos (3 n), d_before, d_after (n), status (n bytes): each may be null (a dry run passes none).
__global__ void __launch_bounds__(BLOCK, 4) project_kernel(const uint32_t* __restrict__ code_g, const unsigned* __restrict__ pos, uint64_t n, float h, float tol,
                                                           float max_move, int max_iters, unsigned* __restrict__ out_pos, float* __restrict__ d_before,
                                                           float* __restrict__ d_after, unsigned char* __restrict__ status, ProjectCounters* __restrict__ ctr) {
  using namespace project;
  code_ptr code = as_code(code_g);
  float* lds = g_smem + threadIdx.x;
  const uint64_t i = (uint64_t)blockIdx.x * BLOCK + threadIdx.x;
  const bool valid = i < n;
  unsigned b0x = 0u, b0y = 0u, b0z = 0u;  // the vertex, as bits: carried bit for bit where it does not move
  if (valid) { b0x = pos[3 * i]; b0y = pos[3 * i + 1]; b0z = pos[3 * i + 2]; }
  const float x0 = __uint_as_float(b0x), y0 = __uint_as_float(b0y), z0 = __uint_as_float(b0z);
  const bool finite = !nb::nan_or_inf(x0) && !nb::nan_or_inf(y0) && !nb::nan_or_inf(z0);
  const bool takes_part = valid && finite;
  bool live = takes_part;
  float x = takes_part ? x0 : 0.f, y = takes_part ? y0 : 0.f, z = takes_part ? z0 : 0.f;
  const unsigned tol_bits = abs_bits(tol);
  const float mm = max_move * max_move, h2 = h + h;
  unsigned st = PROJECT_SKIPPED, steps = 0u;
  float db = __uint_as_float(PROJECT_NOT_EVALUATED), dc = db;  // d_before; the last d of step 1
  unsigned wave_evals = 0u;                                     // wave-uniform: at most 64 lanes x (65 + 6 x 64) evaluations
#pragma unroll 1
  for (int it = 0;; it++) {
    const unsigned long long m1 = __ballot(live);
    if (m1 == 0ull) break;
    wave_evals += (unsigned)__builtin_popcountll(m1);
    {  // 1. d = sdf(x)
      P3 p[1] = {P3{x, y, z}};
      float d[1];
      gsdf_dev::sdf_eval<1>(code, p, d, lds, BLOCK);
      if (live) {
        dc = d[0];
        if (it == 0) db = dc;
        if (it == 0 && is_nan(dc)) { st = PROJECT_NONFINITE; live = false; }
        else if (!abs_gt(dc, tol_bits)) { st = it == 0 ? PROJECT_ON : PROJECT_CONVERGED; live = false; }
        else if (it >= max_iters) { st = PROJECT_ITERS; live = false; }
      }
    }
    const unsigned long long m2 = __ballot(live);
    if (m2 == 0ull) break;
    wave_evals += 6u * (unsigned)__builtin_popcountll(m2);
    float g[3];
#pragma unroll 1
    for (int dim = 0; dim < 3; dim++) {  // 2. normals_kernel's taps
      P3 a = {x + (dim == 0 ? h : 0.f), y + (dim == 1 ? h : 0.f), z + (dim == 2 ? h : 0.f)};
      P3 b = {x - (dim == 0 ? h : 0.f), y - (dim == 1 ? h : 0.f), z - (dim == 2 ? h : 0.f)};
      P3 ab[2] = {a, b};
      float dd[2];
      gsdf_dev::sdf_eval<2>(code, ab, dd, lds, BLOCK);
      const float v = dd[0] - dd[1];
      if (dim == 0) g[0] = v; else if (dim == 1) g[1] = v; else g[2] = v;
    }
    if (live) {
      const float s = (g[0] * g[0] + g[1] * g[1]) + g[2] * g[2];             // 3.
      if (!__builtin_amdgcn_classf(s, 0x380)) { st = PROJECT_FLAT; live = false; }  // NOT (s > 0): +subnormal, +normal, +inf pass
      else {
        const float t = (dc * h2) / s;                                        // 4.
        const float nx = x - t * g[0], ny = y - t * g[1], nz = z - t * g[2];
        const float ux = nx - x0, uy = ny - y0, uz = nz - z0;                // 5.
        const float r = (ux * ux + uy * uy) + uz * uz;
        // NOT (r <= mm): r is a sum of squares (its sign bit is set only on a NaN), mm >= 0 or +inf
        if (!(__float_as_uint(r) <= __float_as_uint(mm))) { st = PROJECT_CLAMPED; live = false; }
        else { x = nx; y = ny; z = nz; steps++; }
      }
    }
  }
  // the end: never further from the surface than at the start
  bool moved = false;
  if (takes_part && st != PROJECT_NONFINITE) {
    const unsigned a_after = abs_bits(dc), a_before = abs_bits(db);
    if (a_after > 0x7f800000u || a_after > a_before) { st = PROJECT_REVERTED; dc = db; }
    else moved = steps != 0u;
  }
  if (valid) {
    if (out_pos) {
      out_pos[3 * i] = moved ? __float_as_uint(x) : b0x;
      out_pos[3 * i + 1] = moved ? __float_as_uint(y) : b0y;
      out_pos[3 * i + 2] = moved ? __float_as_uint(z) : b0z;
    }
    if (d_before) d_before[i] = db;
    if (d_after) d_after[i] = dc;
    if (status) status[i] = (unsigned char)st;
  }
  // counters: one atomic per wave and counter
#pragma unroll 1
  for (unsigned k = 0; k < 8u; k++) wave_count(valid && st == k, &ctr->count[k]);
  wave_count(takes_part && (is_nan(db) || abs_gt(db, tol_bits)), &ctr->over_before);
  wave_count(takes_part && (is_nan(dc) || abs_gt(dc, tol_bits)), &ctr->over_after);
  const unsigned mb = wave_max_u32(takes_part && !is_nan(db) ? abs_bits(db) : 0u);
  const unsigned ma = wave_max_u32(takes_part && !is_nan(dc) ? abs_bits(dc) : 0u);
  const unsigned ms = wave_max_u32(steps);
  if ((threadIdx.x & 63u) == 0u) {
    if (wave_evals) atomicAdd(&ctr->evals, (unsigned long long)wave_evals);
    if (mb) atomicMax(&ctr->max_before, mb);
    if (ma) atomicMax(&ctr->max_after, ma);
    if (ms) atomicMax(&ctr->steps_max, ms);
  }
}
