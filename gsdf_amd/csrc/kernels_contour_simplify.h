// kernels_contour_simplify.h -- loops after tracing: dyadic chord simplification and the loops' measures (include/gsdf_hip.h,
// section "contours: simplify and measures", states the arithmetic; tests/contoursimpref.py restates it in numpy). abi_contour.hip
// launches these, one sequence per pass:
//   cloop_of_kernel        vertex -> its loop, by bisection of loop_start (one writer per word)
//   csimp_reject_kernel    a vertex per lane, walking its loop's levels: q2 against the chord of its span at every level where it is
//                          interior; a span that holds a vertex beyond tol gets its bit set (atomicOr of one value: idempotent)
//   csimp_mark_kernel      a vertex per lane: dropped iff some span around it kept its bit clear; the largest such span is its
//                          maximal one: q2 against that chord -> the 64-bit maximum over bit patterns, the span counted once (by its
//                          first interior vertex), the loop flagged as changed; kept vertices per block of 256
//   block_scan_kernel      (abi_host.h: launch_block_scan) the carry across blocks
//   csimp_emit_kernel      kept vertices to their places, bits and keys carried; a leader's place is its loop's new start
//   cmeas_maxbits_kernel   integer max over the coordinates' |bits|: the exponent e
//   cmeas_init_kernel, cmeas_kernel   a vertex per lane: the edge to its successor, area and length terms quantised to integers and
//                          summed as split 64-bit integers per loop, the box by order-preserving bits
// The bit of span (k, m) of a loop lives in the word of the span's FIRST vertex (loop start + m 2^k), bit k: a vertex starts at most
// one span per level. Nothing but integer atomics (or / add / max / min) reaches memory from more than one lane, so neither the order
// of arrival nor the wave's shape (a wave inside one loop reduces across its lanes first) changes a bit of the result. The report's
// helpers (kernels_topo.h: topo_ordered, topo_split) are restated here, not included: that file defines abi_indexed.hip's kernels.
#pragma once
#include "kernels_common.h"
#include "kernels_contour.h"

#define CSIMP_MAX_LEVELS 16u
#define CMEAS_BB_MIN_INIT 0xff800000u  // order-preserving bits of +inf
#define CMEAS_BB_MAX_INIT 0x007fffffu  // ... of -inf

struct CsimpCounters {
  unsigned long long spans[CSIMP_MAX_LEVELS + 1];  // maximal acceptable spans by level
  unsigned long long loops_changed;
  unsigned long long max_q2;  // bits of the largest q2 of a dropped vertex against its maximal span (non-negative doubles order like their bits)
  unsigned long long bad;     // a destination out of range: cannot happen (the scan counts what the emit writes); checked, not trusted
};

struct CmeasAcc {
  unsigned long long sum[4];  // area: low 32 bits summed, the (signed) rest summed; length likewise
  unsigned bb[4];             // order-preserving bits: min x y, max x y
};

// largest k <= levels with 3 2^k <= n
__device__ __forceinline__ unsigned csimp_kmax(unsigned n, unsigned levels) {
  unsigned k = 0;
  while (k < levels && 3ull * (2ull << k) <= (unsigned long long)n) k++;
  return k;
}

// squared distance of p to the SEGMENT a b, the contract's operations in the contract's order (float64, none contracted)
__device__ __forceinline__ double csimp_q2(double ax, double ay, double bx, double by, double px, double py) {
#pragma clang fp contract(off)
  const double ux = bx - ax, uy = by - ay;
  const double dd = ux * ux + uy * uy;
  const double wx = px - ax, wy = py - ay;
  const double t = wx * ux + wy * uy;
  if (dd == 0.0 || t <= 0.0) return wx * wx + wy * wy;
  if (t >= dd) {
    const double vx = px - bx, vy = py - by;
    return vx * vx + vy * vy;
  }
  const double cr = wx * uy - wy * ux;
  return (cr * cr) / dd;
}

// q2 of vertex j of the loop at l0 (n vertices) against the chord of its span at level k (j is interior to it)
__device__ __forceinline__ double csimp_span_q2(const float* __restrict__ xy, unsigned l0, unsigned n, unsigned j, unsigned k, unsigned* start) {
  const unsigned s = j & ~((1u << k) - 1u);
  const unsigned long long e = (unsigned long long)s + (1ull << k);
  const unsigned long long a = (unsigned long long)l0 + s, b = e >= n ? (unsigned long long)l0 : (unsigned long long)l0 + e, p = (unsigned long long)l0 + j;
  *start = s;
  return csimp_q2((double)xy[2ull * a], (double)xy[2ull * a + 1ull], (double)xy[2ull * b], (double)xy[2ull * b + 1ull], (double)xy[2ull * p], (double)xy[2ull * p + 1ull]);
}

// loop_of[v] = the q with loop_start[q] <= v < loop_start[q + 1]
__global__ void __launch_bounds__(BLOCK) cloop_of_kernel(const unsigned* __restrict__ loop_start, unsigned n_loops, unsigned n_verts, unsigned* __restrict__ loop_of) {
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= n_verts) return;
  const unsigned v = (unsigned)g;
  unsigned lo = 0, hi = n_loops;  // loop_start[lo] <= v < loop_start[hi]
  while (hi - lo > 1u) {
    const unsigned mid = lo + (hi - lo) / 2u;
    if (loop_start[mid] <= v) lo = mid;
    else hi = mid;
  }
  loop_of[v] = lo;
}

__global__ void __launch_bounds__(BLOCK) csimp_reject_kernel(const float* __restrict__ xy, const unsigned* __restrict__ loop_start, const unsigned* __restrict__ loop_of,
                                                             unsigned n_verts, unsigned levels, double tol2, unsigned* rej) {
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= n_verts) return;
  const unsigned v = (unsigned)g, q = loop_of[v], l0 = loop_start[q], n = loop_start[q + 1] - l0, j = v - l0;
  const unsigned kmax = csimp_kmax(n, levels);
  for (unsigned k = 1; k <= kmax; k++) {
    if ((j & ((1u << k) - 1u)) == 0u) continue;  // a span's first vertex is not interior to it
    unsigned s;
    const double q2 = csimp_span_q2(xy, l0, n, j, k, &s);
    if (!(q2 <= tol2)) {  // (false for a NaN: not acceptable)
      unsigned* word = rej + ((unsigned long long)l0 + s);
      if ((__atomic_load_n(word, __ATOMIC_RELAXED) & (1u << k)) == 0u) atomicOr(word, 1u << k);
    }
  }
}

__global__ void __launch_bounds__(BLOCK) csimp_mark_kernel(const float* __restrict__ xy, const unsigned* __restrict__ loop_start, const unsigned* __restrict__ loop_of,
                                                           unsigned n_verts, unsigned levels, const unsigned* __restrict__ rej, unsigned char* __restrict__ keep,
                                                           unsigned* changed, unsigned* __restrict__ blk_cnt, CsimpCounters* ctr) {
  __shared__ unsigned s_w[4];
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const bool live = g < n_verts;
  bool kept = false;
  if (live) {
    const unsigned v = (unsigned)g, q = loop_of[v], l0 = loop_start[q], n = loop_start[q + 1] - l0, j = v - l0;
    unsigned top = 0;
    for (unsigned k = csimp_kmax(n, levels); k >= 1u; k--) {
      if ((j & ((1u << k) - 1u)) == 0u) continue;
      const unsigned s = j & ~((1u << k) - 1u);
      if ((rej[(unsigned long long)l0 + s] & (1u << k)) == 0u) { top = k; break; }
    }
    kept = top == 0u;
    keep[v] = kept ? 1 : 0;
    if (!kept) {
      unsigned s;
      const unsigned long long bits = (unsigned long long)__double_as_longlong(csimp_span_q2(xy, l0, n, j, top, &s));
      if (bits > __atomic_load_n(&ctr->max_q2, __ATOMIC_RELAXED)) atomicMax(&ctr->max_q2, bits);
      if (j == s + 1u) atomicAdd(&ctr->spans[top], 1ull);
      if (__atomic_load_n(changed + q, __ATOMIC_RELAXED) == 0u && atomicOr(changed + q, 1u) == 0u) atomicAdd(&ctr->loops_changed, 1ull);
    }
  }
  unsigned total;
  (void)contour_block_excl(kept ? 1u : 0u, s_w, &total);
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = total;
}

// xy as words: the coordinates are carried bit for bit
__global__ void __launch_bounds__(BLOCK) csimp_emit_kernel(const unsigned* __restrict__ xy, const unsigned* __restrict__ keys, const unsigned* __restrict__ loop_start,
                                                           const unsigned* __restrict__ loop_of, unsigned n_verts, unsigned n_loops,
                                                           const unsigned char* __restrict__ keep, const unsigned* __restrict__ blk_base, unsigned n_out,
                                                           unsigned* __restrict__ xy_out, unsigned* __restrict__ keys_out, unsigned* __restrict__ loop_start_out,
                                                           CsimpCounters* ctr) {
  __shared__ unsigned s_w[4];
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const bool live = g < n_verts;
  const bool kept = live && keep[g] != 0;
  unsigned total;
  const unsigned dst = blk_base[blockIdx.x] + contour_block_excl(kept ? 1u : 0u, s_w, &total);
  if (!live) return;
  const unsigned v = (unsigned)g;
  if (v + 1u == n_verts) loop_start_out[n_loops] = dst + (kept ? 1u : 0u);
  if (!kept) return;
  if (dst >= n_out) { atomicAdd(&ctr->bad, 1ull); return; }
  const unsigned q = loop_of[v];
  if (loop_start[q] == v) loop_start_out[q] = dst;  // (a leader is never interior: always kept)
  xy_out[2ull * dst] = xy[2ull * v];
  xy_out[2ull * dst + 1ull] = xy[2ull * v + 1ull];
  keys_out[dst] = keys[v];
}

// ---- measures ----------------------------------------------------------------------------------------------------------------------
// a float's bits, monotone in its value (-0 below +0)
__device__ __forceinline__ unsigned cmeas_ordered(unsigned bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }

__global__ void __launch_bounds__(BLOCK) cmeas_maxbits_kernel(const float* __restrict__ xy, unsigned long long n, unsigned long long* __restrict__ maxbits) {
  unsigned m = 0;
  const unsigned long long step = (unsigned long long)gridDim.x * BLOCK;
  for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += step) {
    const unsigned a = __float_as_uint(xy[i]) & 0x7fffffffu;
    if (a < 0x7f800000u && a > m) m = a;
  }
  m = nb::wave_max_u32(m);
  if ((threadIdx.x & 63u) == 0u && m) atomicMax(maxbits, (unsigned long long)m);
}

__global__ void __launch_bounds__(BLOCK) cmeas_init_kernel(CmeasAcc* __restrict__ acc, unsigned n_loops) {
  const unsigned long long q = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  if (q >= n_loops) return;
  acc[q].sum[0] = acc[q].sum[1] = acc[q].sum[2] = acc[q].sum[3] = 0ull;
  acc[q].bb[0] = acc[q].bb[1] = CMEAS_BB_MIN_INIT;
  acc[q].bb[2] = acc[q].bb[3] = CMEAS_BB_MAX_INIT;
}

// 2^x as a double, -1022 <= x <= 1023
__device__ __forceinline__ double cmeas_pow2(int x) { return __longlong_as_double((long long)(1023 + x) << 52); }
__device__ __forceinline__ void cmeas_split(double term, double scale, unsigned long long* lo, unsigned long long* hi) {
  const long long q = (long long)__builtin_rint(term * scale);  // |q| <= 2^62
  *lo = (unsigned long long)q & 0xffffffffull;
  *hi = (unsigned long long)(q >> 32);
}
__device__ __forceinline__ unsigned long long cmeas_wave_sum(unsigned long long v) {
  unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned l2 = __shfl_down(lo, off, 64), h2 = __shfl_down(hi, off, 64);
    const unsigned long long t = ((((unsigned long long)hi) << 32) | lo) + ((((unsigned long long)h2) << 32) | l2);  // (mod 2^64: two's complement)
    lo = (unsigned)t;
    hi = (unsigned)(t >> 32);
  }
  return (((unsigned long long)hi) << 32) | lo;  // lane 0 has the wave's sum
}

// *maxbits: cmeas_maxbits_kernel's result; e = max(biased exponent, 1) - 126; the scales 2^(61 - 2 e) and 2^(60 - e)
__global__ void __launch_bounds__(BLOCK) cmeas_kernel(const float* __restrict__ xy, const unsigned* __restrict__ loop_start, const unsigned* __restrict__ loop_of,
                                                      unsigned n_verts, const unsigned long long* __restrict__ maxbits, CmeasAcc* acc) {
#pragma clang fp contract(off)
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const bool live = g < n_verts;
  unsigned q = CONTOUR_NONE;
  unsigned long long s[4] = {0ull, 0ull, 0ull, 0ull};
  unsigned bmin[2] = {0xffffffffu, 0xffffffffu}, bmax[2] = {0u, 0u};
  if (live) {
    const unsigned v = (unsigned)g;
    q = loop_of[v];
    const unsigned l0 = loop_start[q], l1 = loop_start[q + 1];
    const unsigned long long nx = v + 1u == l1 ? l0 : (unsigned long long)v + 1ull;
    const unsigned biased = (unsigned)(*maxbits >> 23);
    const int e = (int)(biased > 1u ? biased : 1u) - 126;
    const float fx = xy[2ull * v], fy = xy[2ull * v + 1ull];
    const double x0 = (double)fx, y0 = (double)fy, x1 = (double)xy[2ull * nx], y1 = (double)xy[2ull * nx + 1ull];
    const double a = x0 * y1 - x1 * y0;  // (both products exact: 24 x 24 bits)
    const double dx = x1 - x0, dy = y1 - y0;
    const double len = __builtin_sqrt(dx * dx + dy * dy);
    cmeas_split(a, cmeas_pow2(61 - 2 * e), &s[0], &s[1]);
    cmeas_split(len, cmeas_pow2(60 - e), &s[2], &s[3]);
    bmin[0] = bmax[0] = cmeas_ordered(__float_as_uint(fx));
    bmin[1] = bmax[1] = cmeas_ordered(__float_as_uint(fy));
  }
  // a wave inside one loop: one atomic per quantity; a mixed wave: each lane's own
  const unsigned long long m = __ballot(live);
  if (m == 0ull) return;  // (the whole wave)
  const unsigned q0 = (unsigned)__shfl((int)q, __builtin_ctzll(m), 64);
  const bool uniform = __ballot(live && q != q0) == 0ull;
  if (uniform) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const unsigned long long t = cmeas_wave_sum(s[k]);
      if ((threadIdx.x & 63u) == 0u && t) atomicAdd(&acc[q0].sum[k], t);
    }
#pragma unroll
    for (int k = 0; k < 2; k++) {
      unsigned lo = bmin[k], hi = bmax[k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) {
        const unsigned o_lo = __shfl_down(lo, off, 64), o_hi = __shfl_down(hi, off, 64);
        lo = o_lo < lo ? o_lo : lo;
        hi = o_hi > hi ? o_hi : hi;
      }
      if ((threadIdx.x & 63u) == 0u) {
        atomicMin(&acc[q0].bb[k], lo);
        atomicMax(&acc[q0].bb[2 + k], hi);
      }
    }
  } else if (live) {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (s[k]) atomicAdd(&acc[q].sum[k], s[k]);
#pragma unroll
    for (int k = 0; k < 2; k++) {
      atomicMin(&acc[q].bb[k], bmin[k]);
      atomicMax(&acc[q].bb[2 + k], bmax[k]);
    }
  }
}
