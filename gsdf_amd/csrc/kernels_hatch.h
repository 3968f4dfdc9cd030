// kernels_hatch.h -- hatch fill: the segments of a family of parallel lines inside the loops of every layer (include/gsdf_hip.h,
// section "contours: hatch fill", states the arithmetic; tests/hatchref.py restates it in numpy). abi_contour.hip launches these,
// after cmeas_maxbits_kernel (the exponent) and cloop_of_kernel, one workgroup per 256 elements each:
//   hatch_init_kernel        a layer per lane: its line range emptied, its length sum cleared
//   hatch_range_kernel       an edge per lane (a vertex and its successor): s of both ends, the lines k_first .. k_first + n - 1 it
//                            crosses (an estimate from (s - offset) / spacing, corrected with the predicate), the layer's smallest
//                            and largest k by integer atomics, the crossings of the call, n per block of 256 edges
//   hatch_scan_kernel        counts -> exclusive offsets with the carry of launch_block_scan (abi_host.h): edges, then line slots
//   hatch_count_kernel       a crossing per lane: its edge by bisection of the edges' offsets, its line slot; crossings per slot
//   hatch_lines_kernel       a line slot per lane: slots per block for the scan; lines with a crossing, the largest bucket; an odd
//                            bucket is counted as bad (a closed loop crosses a line an even number of times)
//   hatch_emit_kernel        a crossing per lane: t, u_c, x_c, y_c; the record goes into its line's bucket in ARRIVAL order
//   hatch_rank_kernel        a record per lane: its rank = the records of its bucket that are smaller under (u_c, j), a total order,
//                            so the place line_start + rank does not depend on the arrival; it writes its end of its segment
//   hatch_layer_start_kernel layer -> its first segment
//   hatch_length_kernel      a segment per lane: u_c1 - u_c0 quantised and summed per layer as split integers (cmeas_kernel's two
//                            paths), segments whose two ends have the same bits counted
// A line slot is (layer, k - k_min of the layer): the host lays the layers' slots behind one another between the range pass and the
// count. Nothing but integer atomics reaches memory from more than one lane, except the buckets' arrival order, which the rank
// removes. The rank reads its bucket from L2: m^2 comparisons for a line with m crossings (the statistics give the largest m).
#pragma once
#include "kernels_common.h"
#include "kernels_contour_simplify.h"

#define HATCH_K_LIMIT 1073741832.0  // 2^30 + 8: beyond every k the host's check on spacing admits

struct HatchParams {
  double offset, spacing;
  double dx0, dy0, dx1, dy1, dx2, dy2, dx3, dy3;
  unsigned n_dirs;
};

struct HatchCounters {
  unsigned long long n_crossings, n_lines, max_line, zero_length;
  unsigned long long bad;  // an odd bucket, a record or a segment out of range: cannot happen for closed loops; checked, not trusted
};

struct HatchLayerAcc {
  unsigned long long sum[2];  // length: low 32 bits summed, the (signed) rest summed
  int k_min, k_max;           // INT_MAX, INT_MIN: no crossing
};

// (dx, dy) of a layer: dir[layer % n_dirs], selected without indexing the argument record
__device__ __forceinline__ void hatch_dir(const HatchParams& P, unsigned layer, double* dx, double* dy) {
  const unsigned m = layer % P.n_dirs;
  *dx = m == 0u ? P.dx0 : (m == 1u ? P.dx1 : (m == 2u ? P.dx2 : P.dx3));
  *dy = m == 0u ? P.dy0 : (m == 1u ? P.dy1 : (m == 2u ? P.dy2 : P.dy3));
}

__device__ __forceinline__ double hatch_line(int k, double offset, double spacing) {
#pragma clang fp contract(off)
  return offset + ((double)k * spacing);
}

// the smallest k with s < c_k (c_k is non-decreasing in k)
__device__ __forceinline__ int hatch_first_above(double s, double offset, double spacing) {
#pragma clang fp contract(off)
  double q = __builtin_floor((s - offset) / spacing);
  q = q < -HATCH_K_LIMIT ? -HATCH_K_LIMIT : (q > HATCH_K_LIMIT ? HATCH_K_LIMIT : q);
  int k = (int)q;  // (the quotient's two roundings move it by less than 2^-23 of a line: k is right or one off)
  for (int i = 0; i < 64 && s < hatch_line(k, offset, spacing); i++) k--;
  for (int i = 0; i < 64 && !(s < hatch_line(k + 1, offset, spacing)); i++) k++;
  return k + 1;
}

// what an edge is to the hatch: the tail v, its successor in the loop, the layer's direction
struct HatchEdge {
  double xa, ya, xb, yb, dx, dy, sa, sb;
  unsigned layer;
};
__device__ __forceinline__ HatchEdge hatch_edge(const float* __restrict__ xy, const unsigned* __restrict__ loop_start, const unsigned* __restrict__ loop_of,
                                                const unsigned* __restrict__ loop_layer, unsigned v, const HatchParams& P) {
#pragma clang fp contract(off)
  HatchEdge e;
  const unsigned q = loop_of[v], l0 = loop_start[q], l1 = loop_start[q + 1];
  const unsigned long long nx = v + 1u == l1 ? l0 : (unsigned long long)v + 1ull;
  e.layer = loop_layer[q];
  hatch_dir(P, e.layer, &e.dx, &e.dy);
  e.xa = (double)xy[2ull * v];
  e.ya = (double)xy[2ull * v + 1ull];
  e.xb = (double)xy[2ull * nx];
  e.yb = (double)xy[2ull * nx + 1ull];
  e.sa = ((-e.dy) * e.xa) + (e.dx * e.ya);
  e.sb = ((-e.dy) * e.xb) + (e.dx * e.yb);
  return e;
}

__global__ void __launch_bounds__(BLOCK) hatch_init_kernel(HatchLayerAcc* __restrict__ acc, unsigned n_layers) {
  const unsigned long long l = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  if (l >= n_layers) return;
  acc[l].sum[0] = acc[l].sum[1] = 0ull;
  acc[l].k_min = 0x7fffffff;
  acc[l].k_max = -0x7fffffff - 1;
}

__global__ void __launch_bounds__(BLOCK) hatch_range_kernel(const float* __restrict__ xy, const unsigned* __restrict__ loop_start, const unsigned* __restrict__ loop_of,
                                                            const unsigned* __restrict__ loop_layer, unsigned n_verts, unsigned n_layers, HatchParams P,
                                                            int* __restrict__ k_first, unsigned* __restrict__ cnt, unsigned* __restrict__ blk_cnt,
                                                            HatchLayerAcc* acc, HatchCounters* ctr) {
  __shared__ unsigned s_w[4];
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  unsigned n = 0;
  bool bad = false;
  if (g < n_verts) {
    const unsigned v = (unsigned)g;
    const HatchEdge e = hatch_edge(xy, loop_start, loop_of, loop_layer, v, P);
    const double lo = e.sa < e.sb ? e.sa : e.sb, hi = e.sa < e.sb ? e.sb : e.sa;
    // crossed iff lo < c_k <= hi: from the first k above lo to the one before the first k above hi
    const int kf = hatch_first_above(lo, P.offset, P.spacing), ke = hatch_first_above(hi, P.offset, P.spacing);
    n = (unsigned)(ke - kf);
    k_first[v] = kf;
    cnt[v] = n;
    bad = e.layer >= n_layers;
    if (n != 0u && !bad) {
      if (kf < __atomic_load_n(&acc[e.layer].k_min, __ATOMIC_RELAXED)) atomicMin(&acc[e.layer].k_min, kf);
      if (ke - 1 > __atomic_load_n(&acc[e.layer].k_max, __ATOMIC_RELAXED)) atomicMax(&acc[e.layer].k_max, ke - 1);
    }
  }
  const unsigned long long wave_n = cmeas_wave_sum((unsigned long long)n);
  if ((threadIdx.x & 63u) == 0u && wave_n) atomicAdd(&ctr->n_crossings, wave_n);
  contour_tally(bad, &ctr->bad);
  unsigned total;
  (void)contour_block_excl(n, s_w, &total);  // (wraps with 2^32 crossings or more in a block: the host refuses on n_crossings first)
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = total;
}

// out[i] = the sum of cnt[0 .. i), out[n] = the whole sum; blk_base: launch_block_scan's carry of the blocks' sums
__global__ void __launch_bounds__(BLOCK) hatch_scan_kernel(const unsigned* __restrict__ cnt, unsigned n, const unsigned* __restrict__ blk_base,
                                                           unsigned* __restrict__ out) {
  __shared__ unsigned s_w[4];
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const unsigned v = g < n ? cnt[g] : 0u;
  unsigned total;
  const unsigned at = blk_base[blockIdx.x] + contour_block_excl(v, s_w, &total);
  if (g < n) out[g] = at;
  if (g + 1ull == n) out[n] = at + v;
}

// the last i with start[i] <= x (start[0] <= x < start[n])
__device__ __forceinline__ unsigned hatch_bisect(const unsigned* __restrict__ start, unsigned n, unsigned x) {
  unsigned lo = 0, hi = n;
  while (hi - lo > 1u) {
    const unsigned mid = lo + (hi - lo) / 2u;
    if (start[mid] <= x) lo = mid;
    else hi = mid;
  }
  return lo;
}

__global__ void __launch_bounds__(BLOCK) hatch_count_kernel(const unsigned* __restrict__ edge_off, unsigned n_verts, const int* __restrict__ k_first,
                                                            const unsigned* __restrict__ loop_of, const unsigned* __restrict__ loop_layer,
                                                            const unsigned* __restrict__ slot_base, const int* __restrict__ layer_kmin, unsigned n_layers,
                                                            unsigned n_slots, unsigned n_cross, unsigned* __restrict__ cross_edge,
                                                            unsigned* __restrict__ cross_slot, unsigned* line_cnt, HatchCounters* ctr) {
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  bool bad = false;
  if (g < n_cross) {
    const unsigned c = (unsigned)g;
    const unsigned v = hatch_bisect(edge_off, n_verts, c);
    const unsigned layer = loop_layer[loop_of[v]];
    unsigned slot = n_slots;
    if (layer < n_layers) {
      const long long k = (long long)k_first[v] + (long long)(c - edge_off[v]);
      const long long at = (long long)slot_base[layer] + (k - (long long)layer_kmin[layer]);
      if (at >= (long long)slot_base[layer] && at < (long long)slot_base[layer + 1u]) slot = (unsigned)at;
    }
    bad = slot >= n_slots;
    cross_edge[c] = v;
    cross_slot[c] = slot;  // (n_slots: none)
    if (!bad) atomicAdd(&line_cnt[slot], 1u);
  }
  contour_tally(bad, &ctr->bad);
}

__global__ void __launch_bounds__(BLOCK) hatch_lines_kernel(const unsigned* __restrict__ line_cnt, unsigned n_slots, unsigned* __restrict__ blk_cnt, HatchCounters* ctr) {
  __shared__ unsigned s_w[4];
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const unsigned m = g < n_slots ? line_cnt[g] : 0u;
  contour_tally(m != 0u, &ctr->n_lines);
  contour_tally((m & 1u) != 0u, &ctr->bad);
  const unsigned wave_max = nb::wave_max_u32(m);
  if ((threadIdx.x & 63u) == 0u && wave_max > __atomic_load_n(&ctr->max_line, __ATOMIC_RELAXED)) atomicMax(&ctr->max_line, (unsigned long long)wave_max);
  unsigned total;
  (void)contour_block_excl(m, s_w, &total);
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = total;
}

// The crossing of an edge with line k (gsdf_hip.h, "Crossings"): one IEEE float64 operation each, in the contract's order.
__global__ void __launch_bounds__(BLOCK) hatch_emit_kernel(const float* __restrict__ xy, const unsigned* __restrict__ loop_start, const unsigned* __restrict__ loop_of,
                                                           const unsigned* __restrict__ loop_layer, HatchParams P, const unsigned* __restrict__ edge_off,
                                                           const int* __restrict__ k_first, const unsigned* __restrict__ cross_edge,
                                                           const unsigned* __restrict__ cross_slot, const unsigned* __restrict__ line_start, unsigned n_slots,
                                                           unsigned n_cross, unsigned* cursor, double* __restrict__ rec_u, unsigned* __restrict__ rec_j,
                                                           float* __restrict__ rec_xy, unsigned* __restrict__ rec_slot, int* __restrict__ rec_k,
                                                           HatchCounters* ctr) {
#pragma clang fp contract(off)
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  bool bad = false;
  if (g < n_cross) {
    const unsigned c = (unsigned)g, v = cross_edge[c], slot = cross_slot[c];
    bad = slot >= n_slots;
    if (!bad) {
      const HatchEdge e = hatch_edge(xy, loop_start, loop_of, loop_layer, v, P);
      const int k = k_first[v] + (int)(c - edge_off[v]);
      const double ck = hatch_line(k, P.offset, P.spacing);
      const double ua = (e.dx * e.xa) + (e.dy * e.ya), ub = (e.dx * e.xb) + (e.dy * e.yb);
      const double t = (ck - e.sa) / (e.sb - e.sa);
      const double uc = ua + (t * (ub - ua));
      const float xc = (float)(e.xa + (t * (e.xb - e.xa))), yc = (float)(e.ya + (t * (e.yb - e.ya)));
      const unsigned b0 = line_start[slot], b1 = line_start[slot + 1u];
      const unsigned at = b0 + atomicAdd(&cursor[slot], 1u);
      bad = at >= b1 || at >= n_cross;
      if (!bad) {
        rec_u[at] = uc;
        rec_j[at] = v;
        rec_xy[2ull * at] = xc;
        rec_xy[2ull * at + 1ull] = yc;
        rec_slot[at] = slot;
        rec_k[at] = k;
      }
    }
  }
  contour_tally(bad, &ctr->bad);
}

// record p is in the bucket line_start[slot] .. line_start[slot + 1]; (u_c, j) orders it: doubles compared as doubles (-0 == +0),
// j (the tail's global vertex number: no two records of a line share it) breaks ties
__global__ void __launch_bounds__(BLOCK) hatch_rank_kernel(const double* __restrict__ rec_u, const unsigned* __restrict__ rec_j, const float* __restrict__ rec_xy,
                                                           const unsigned* __restrict__ rec_slot, const int* __restrict__ rec_k,
                                                           const unsigned* __restrict__ line_start, unsigned n_slots, unsigned n_cross,
                                                           float* __restrict__ seg, int* __restrict__ line, double* __restrict__ u_sorted,
                                                           HatchCounters* ctr) {
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  bool bad = false;
  if (g < n_cross && rec_slot[g] >= n_slots) bad = true;  // (a place no record reached: rec_slot starts as all ones)
  else if (g < n_cross) {
    const unsigned p = (unsigned)g, slot = rec_slot[p];
    const unsigned b0 = line_start[slot], b1 = line_start[slot + 1u];
    const double u = rec_u[p];
    const unsigned j = rec_j[p];
    unsigned rank = 0;
    for (unsigned i = b0; i < b1; i++) {
      const double ui = rec_u[i];
      rank += (ui < u || (ui == u && rec_j[i] < j)) ? 1u : 0u;
    }
    const unsigned long long at = (unsigned long long)b0 + rank;
    bad = at >= b1 || at >= n_cross;
    if (!bad) {
      u_sorted[at] = u;
      seg[2ull * at] = rec_xy[2ull * p];  // (segment at / 2, its end at % 2: four floats per segment)
      seg[2ull * at + 1ull] = rec_xy[2ull * p + 1ull];
      if ((at & 1ull) == 0ull) line[at >> 1] = rec_k[p];
    }
  }
  contour_tally(bad, &ctr->bad);
}

__global__ void __launch_bounds__(BLOCK) hatch_layer_start_kernel(const unsigned* __restrict__ line_start, const unsigned* __restrict__ slot_base, unsigned n_layers,
                                                                  unsigned* __restrict__ layer_start) {
  const unsigned long long l = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  if (l > n_layers) return;
  layer_start[l] = line_start[slot_base[l]] / 2u;
}

// *maxbits: cmeas_maxbits_kernel's result, as cmeas_kernel reads it; the scale 2^(58 - e)
__global__ void __launch_bounds__(BLOCK) hatch_length_kernel(const double* __restrict__ u_sorted, const unsigned* __restrict__ seg,
                                                             const unsigned* __restrict__ layer_start, unsigned n_layers, unsigned n_segs,
                                                             const unsigned long long* __restrict__ maxbits, HatchLayerAcc* acc, HatchCounters* ctr) {
#pragma clang fp contract(off)
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const bool live = g < n_segs;
  unsigned layer = CONTOUR_NONE;
  unsigned long long s[2] = {0ull, 0ull};
  bool zero = false;
  if (live) {
    const unsigned i = (unsigned)g;
    layer = hatch_bisect(layer_start, n_layers, i);
    const unsigned biased = (unsigned)(*maxbits >> 23);
    const int e = (int)(biased > 1u ? biased : 1u) - 126;
    cmeas_split(u_sorted[2ull * i + 1ull] - u_sorted[2ull * i], cmeas_pow2(58 - e), &s[0], &s[1]);
    zero = seg[4ull * i] == seg[4ull * i + 2ull] && seg[4ull * i + 1ull] == seg[4ull * i + 3ull];
  }
  contour_tally(zero, &ctr->zero_length);
  // a wave inside one layer: one atomic per word; a mixed wave: each lane's own
  const unsigned long long m = __ballot(live);
  if (m == 0ull) return;  // (the whole wave)
  const unsigned l0 = (unsigned)__shfl((int)layer, __builtin_ctzll(m), 64);
  const bool uniform = __ballot(live && layer != l0) == 0ull;
  if (uniform) {
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const unsigned long long t = cmeas_wave_sum(s[k]);
      if ((threadIdx.x & 63u) == 0u && t) atomicAdd(&acc[l0].sum[k], t);
    }
  } else if (live) {
#pragma unroll
    for (int k = 0; k < 2; k++)
      if (s[k]) atomicAdd(&acc[layer].sum[k], s[k]);
  }
}
