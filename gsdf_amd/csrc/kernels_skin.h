// kernels_skin.h -- skin classification of the hatch: every layer's hatch lines cut against the loops of the layers below and above
// it, each piece of a line classed as inner (0), bottom (1), top (2) or both (3) (include/gsdf_hip.h, section "contours: skin
// classification of the hatch", states the arithmetic; tests/skinref.py restates it in numpy). abi_contour.hip launches these behind
// the hatch's own range pass (hatch_init_kernel, cloop_of_kernel, hatch_range_kernel: the layers' own k_min / k_max), one workgroup
// per 256 elements each:
//   skin_init_kernel         a layer per lane: its sums, counts and piece range cleared
//   skin_range_kernel        an (edge, source number r) per lane: the target layer l the edge is source r of, s of both ends under
//                            l's direction, the lines it crosses clipped to l's own k_min .. k_max; n per block of 256
//   hatch_scan_kernel        (kernels_hatch.h) counts -> offsets: the pairs, then the line slots
//   skin_count_kernel        a crossing per lane: its pair by bisection, its line slot; crossings and own crossings per slot
//   skin_lines_kernel        a line slot per lane: a slot without an own crossing is emptied (its line does not exist); the lines,
//                            the crossings on them, the own ones, the largest bucket; an odd count is bad
//   skin_emit_kernel         a crossing per lane: t, u_c, x_c, y_c under the TARGET's direction; into its line's bucket in ARRIVAL order
//   skin_rank_kernel         a record per lane, one sweep of its bucket: its rank under (u_c, r, j), the sources' parity below and
//                            up to its value, whether it leads its tie group; a leader whose class changes is a BOUNDARY
//   skin_flags_kernel, skin_compact_kernel   boundaries and pieces (boundaries whose class is not OUTSIDE) numbered by two scans
//   skin_piece_kernel        a piece per lane: from its boundary to the next one of its line; class, line, end points, the length
//                            term into its (layer, class) as split integers, the layer's piece range, equal end points counted
//   skin_layer_start_kernel  layer -> its first piece
// Nothing but integer atomics reaches memory from more than one lane, except the buckets' arrival order, which the rank removes.
// The sweep reads 16 B per record of the bucket: where a whole wave sits in one bucket (the common case, and the only one that
// costs: m^2 grows with (1 + below + above)^2) the bucket's bounds are made wave-uniform and the records come through the scalar
// cache, one load per wave and record, not 64.
#pragma once
#include "kernels_hatch.h"

#define SKIN_MAX_WINDOW 8u
#define SKIN_OUTSIDE 4u

struct SkinParams {
  unsigned below, above, n_src;    // n_src = 1 + below + above
  unsigned need_below, need_above; // the mask bits of the sources 1 .. below, below + 1 .. below + above
};

struct SkinCounters {
  unsigned long long n_cand;  // crossings of the range pass (inside the layers' own line ranges; lines without an own crossing included)
  unsigned long long n_crossings, n_own, n_lines, max_line, zero_length, n_bnd, n_pieces;
  unsigned long long bad;     // an odd bucket, a record, boundary or piece out of range, a line that does not end OUTSIDE: checked, not trusted
};

struct SkinLayerAcc {
  unsigned long long sum[4][2];  // by class: low 32 bits summed, the (signed) rest summed
  unsigned long long n[4];       // pieces by class
  int k_min, k_max;              // over the pieces; INT_MAX, INT_MIN: none
};

struct SkinRec {
  double u;
  unsigned long long key;  // r << 32 | j: (u, key) is the total order
};

// the layer that source number r of it is layer m: r = 0 itself, r = i (1 .. below) layer l - i, r = below + i layer l + i
__device__ __forceinline__ long long skin_target(unsigned m, unsigned r, unsigned below) {
  return r == 0u ? (long long)m : (r <= below ? (long long)m + (long long)r : (long long)m - (long long)(r - below));
}

__device__ __forceinline__ unsigned skin_class(unsigned mask, const SkinParams& K) {
  if ((mask & 1u) == 0u) return SKIN_OUTSIDE;
  return ((mask & K.need_below) != K.need_below ? 1u : 0u) | ((mask & K.need_above) != K.need_above ? 2u : 0u);
}

// hatch_edge with s of both ends under the direction of `layer` instead of the edge's own
__device__ __forceinline__ HatchEdge skin_edge(const float* __restrict__ xy, const unsigned* __restrict__ loop_start, const unsigned* __restrict__ loop_of,
                                               const unsigned* __restrict__ loop_layer, unsigned v, unsigned layer, const HatchParams& P) {
#pragma clang fp contract(off)
  HatchEdge e = hatch_edge(xy, loop_start, loop_of, loop_layer, v, P);
  hatch_dir(P, layer, &e.dx, &e.dy);
  e.sa = ((-e.dy) * e.xa) + (e.dx * e.ya);
  e.sb = ((-e.dy) * e.xb) + (e.dx * e.yb);
  return e;
}

__global__ void __launch_bounds__(BLOCK) skin_init_kernel(SkinLayerAcc* __restrict__ acc, unsigned n_layers) {
  const unsigned long long l = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  if (l >= n_layers) return;
#pragma unroll
  for (int c = 0; c < 4; c++) acc[l].sum[c][0] = acc[l].sum[c][1] = acc[l].n[c] = 0ull;
  acc[l].k_min = 0x7fffffff;
  acc[l].k_max = -0x7fffffff - 1;
}

// pair g = r n_verts + v (r-major: neighbouring lanes read neighbouring vertices)
__global__ void __launch_bounds__(BLOCK) skin_range_kernel(const float* __restrict__ xy, const unsigned* __restrict__ loop_start, const unsigned* __restrict__ loop_of,
                                                           const unsigned* __restrict__ loop_layer, unsigned n_verts, unsigned n_layers, HatchParams P, SkinParams K,
                                                           const int* __restrict__ layer_kmin, const int* __restrict__ layer_kmax, int* __restrict__ k_first,
                                                           unsigned* __restrict__ cnt, unsigned* __restrict__ blk_cnt, SkinCounters* ctr) {
  __shared__ unsigned s_w[4];
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const unsigned long long n_pairs = (unsigned long long)n_verts * K.n_src;
  unsigned n = 0;
  bool bad = false;
  if (g < n_pairs) {
    const unsigned r = (unsigned)(g / n_verts), v = (unsigned)(g - (unsigned long long)r * n_verts);
    const unsigned m = loop_layer[loop_of[v]];
    bad = m >= n_layers;
    const long long l = skin_target(m, r, K.below);
    int kf = 0;
    if (!bad && l >= 0 && l < (long long)n_layers) {
      const int k_min = layer_kmin[l], k_max = layer_kmax[l];
      if (k_min <= k_max) {
        const HatchEdge e = skin_edge(xy, loop_start, loop_of, loop_layer, v, (unsigned)l, P);
        const double lo = e.sa < e.sb ? e.sa : e.sb, hi = e.sa < e.sb ? e.sb : e.sa;
        // crossed iff lo < c_k <= hi, as in hatch_range_kernel; only the target's own lines count
        const int k0 = hatch_first_above(lo, P.offset, P.spacing), k1 = hatch_first_above(hi, P.offset, P.spacing);
        kf = k0 > k_min ? k0 : k_min;
        const long long ke = (long long)k1 < (long long)k_max + 1ll ? (long long)k1 : (long long)k_max + 1ll;
        n = ke > (long long)kf ? (unsigned)(ke - (long long)kf) : 0u;
      }
    }
    k_first[g] = kf;
    cnt[g] = n;
  }
  const unsigned long long wave_n = cmeas_wave_sum((unsigned long long)n);
  if ((threadIdx.x & 63u) == 0u && wave_n) atomicAdd(&ctr->n_cand, wave_n);
  contour_tally(bad, &ctr->bad);
  unsigned total;
  (void)contour_block_excl(n, s_w, &total);  // (wraps with 2^32 crossings or more in a block: the host refuses on n_cand first)
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = total;
}

__global__ void __launch_bounds__(BLOCK) skin_count_kernel(const unsigned* __restrict__ pair_off, unsigned n_pairs, unsigned n_verts, const int* __restrict__ k_first,
                                                           const unsigned* __restrict__ loop_of, const unsigned* __restrict__ loop_layer, SkinParams K,
                                                           const unsigned* __restrict__ slot_base, const int* __restrict__ layer_kmin, unsigned n_layers,
                                                           unsigned n_slots, unsigned n_cand, unsigned* __restrict__ cross_pair, unsigned* __restrict__ cross_slot,
                                                           unsigned* line_cnt, unsigned* own_cnt, SkinCounters* ctr) {
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  bool bad = false;
  if (g < n_cand) {
    const unsigned c = (unsigned)g;
    const unsigned pair = hatch_bisect(pair_off, n_pairs, c);
    const unsigned r = pair / n_verts, v = pair - r * n_verts;
    const unsigned m = loop_layer[loop_of[v]];
    const long long l = m < n_layers ? skin_target(m, r, K.below) : -1ll;
    unsigned slot = n_slots;
    if (l >= 0 && l < (long long)n_layers) {
      const long long k = (long long)k_first[pair] + (long long)(c - pair_off[pair]);
      const long long at = (long long)slot_base[l] + (k - (long long)layer_kmin[l]);
      if (at >= (long long)slot_base[l] && at < (long long)slot_base[l + 1]) slot = (unsigned)at;
    }
    bad = slot >= n_slots;
    cross_pair[c] = pair;
    cross_slot[c] = slot;  // (n_slots: none)
    if (!bad) {
      atomicAdd(&line_cnt[slot], 1u);
      if (r == 0u) atomicAdd(&own_cnt[slot], 1u);
    }
  }
  contour_tally(bad, &ctr->bad);
}

// a slot without an own crossing is no line: its count becomes 0, so its bucket is empty and nothing of it is counted
__global__ void __launch_bounds__(BLOCK) skin_lines_kernel(unsigned* __restrict__ line_cnt, const unsigned* __restrict__ own_cnt, unsigned n_slots,
                                                           unsigned* __restrict__ blk_cnt, SkinCounters* ctr) {
  __shared__ unsigned s_w[4];
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const unsigned own = g < n_slots ? own_cnt[g] : 0u;
  const unsigned m = own != 0u ? line_cnt[g] : 0u;
  if (g < n_slots) line_cnt[g] = m;
  contour_tally(m != 0u, &ctr->n_lines);
  contour_tally(((m | own) & 1u) != 0u, &ctr->bad);
  const unsigned long long wave_m = cmeas_wave_sum((unsigned long long)m), wave_own = cmeas_wave_sum((unsigned long long)own);
  if ((threadIdx.x & 63u) == 0u && wave_m) atomicAdd(&ctr->n_crossings, wave_m);
  if ((threadIdx.x & 63u) == 0u && wave_own) atomicAdd(&ctr->n_own, wave_own);
  const unsigned wave_max = nb::wave_max_u32(m);
  if ((threadIdx.x & 63u) == 0u && wave_max > __atomic_load_n(&ctr->max_line, __ATOMIC_RELAXED)) atomicMax(&ctr->max_line, (unsigned long long)wave_max);
  unsigned total;
  (void)contour_block_excl(m, s_w, &total);
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = total;
}

// The crossing of an edge of a source layer with line k of the target (gsdf_hip.h, the hatch's "Crossings" under the target's
// direction): one IEEE float64 operation each, in the contract's order.
__global__ void __launch_bounds__(BLOCK) skin_emit_kernel(const float* __restrict__ xy, const unsigned* __restrict__ loop_start, const unsigned* __restrict__ loop_of,
                                                          const unsigned* __restrict__ loop_layer, HatchParams P, SkinParams K, unsigned n_verts, unsigned n_layers,
                                                          const unsigned* __restrict__ pair_off, const int* __restrict__ k_first,
                                                          const unsigned* __restrict__ cross_pair, const unsigned* __restrict__ cross_slot,
                                                          const unsigned* __restrict__ line_start, unsigned n_slots, unsigned n_cand, unsigned* cursor,
                                                          SkinRec* __restrict__ rec, float* __restrict__ rec_xy, unsigned* __restrict__ rec_slot, int* __restrict__ rec_k,
                                                          SkinCounters* ctr) {
#pragma clang fp contract(off)
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  bool bad = false;
  if (g < n_cand) {
    const unsigned c = (unsigned)g, pair = cross_pair[c], slot = cross_slot[c];
    bad = slot >= n_slots;
    const unsigned b0 = bad ? 0u : line_start[slot], b1 = bad ? 0u : line_start[slot + 1u];
    if (!bad && b0 != b1) {  // (b0 == b1: a slot without an own crossing)
      const unsigned r = pair / n_verts, v = pair - r * n_verts;
      const long long l = skin_target(loop_layer[loop_of[v]], r, K.below);
      bad = l < 0 || l >= (long long)n_layers;
      if (!bad) {
        const HatchEdge e = skin_edge(xy, loop_start, loop_of, loop_layer, v, (unsigned)l, P);
        const int k = k_first[pair] + (int)(c - pair_off[pair]);
        const double ck = hatch_line(k, P.offset, P.spacing);
        const double ua = (e.dx * e.xa) + (e.dy * e.ya), ub = (e.dx * e.xb) + (e.dy * e.yb);
        const double t = (ck - e.sa) / (e.sb - e.sa);
        const double uc = ua + (t * (ub - ua));
        const float xc = (float)(e.xa + (t * (e.xb - e.xa))), yc = (float)(e.ya + (t * (e.yb - e.ya)));
        const unsigned at = b0 + atomicAdd(&cursor[slot], 1u);
        bad = at >= b1 || at >= n_cand;
        if (!bad) {
          rec[at].u = uc;
          rec[at].key = (unsigned long long)r << 32 | (unsigned long long)v;
          rec_xy[2ull * at] = xc;
          rec_xy[2ull * at + 1ull] = yc;
          rec_slot[at] = slot;
          rec_k[at] = k;
        }
      }
    }
  }
  contour_tally(bad, &ctr->bad);
}

// what one record of the bucket does to record (u, key)'s sums
struct SkinSweep {
  unsigned rank = 0, below_mask = 0, upto_mask = 0;  // the records before it; the sources' parity below its value, and up to it
  bool led = false;                                  // a record of its value comes before it
  __device__ __forceinline__ void take(const SkinRec q, double u, unsigned long long key) {
    const bool lt = q.u < u, eq = q.u == u, first = eq && q.key < key;
    const unsigned bit = 1u << (unsigned)(q.key >> 32);
    rank += (lt || first) ? 1u : 0u;
    below_mask ^= lt ? bit : 0u;
    upto_mask ^= (lt || eq) ? bit : 0u;
    led = led || first;
  }
};

// Record p is in the bucket line_start[slot] .. line_start[slot + 1]. Its place is line_start + its rank under (u_c, r, j): doubles
// compared as doubles (-0 == +0); no two records of a line share (r, j). flag at that place: 0, or 1 + the class that begins at its
// value where it leads its tie group and that class differs from the one before the value (a line starts OUTSIDE).
__global__ void __launch_bounds__(BLOCK) skin_rank_kernel(const SkinRec* __restrict__ rec, const float* __restrict__ rec_xy, const unsigned* __restrict__ rec_slot,
                                                          const unsigned* __restrict__ line_start, unsigned n_slots, unsigned n_cand, SkinParams K,
                                                          double* __restrict__ u_sorted, float* __restrict__ xy_sorted, unsigned char* __restrict__ flag,
                                                          SkinCounters* ctr) {
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const unsigned n_rec = line_start[n_slots] < n_cand ? line_start[n_slots] : n_cand;
  bool live = g < n_rec, bad = false;
  unsigned slot = 0, b0 = 0, b1 = 0;
  SkinRec me{0.0, 0ull};
  if (live) {
    slot = rec_slot[g];
    bad = slot >= n_slots;  // (a place no record reached: rec_slot starts as all ones)
    live = !bad;
  }
  if (live) {
    b0 = line_start[slot];
    b1 = line_start[slot + 1u];
    bad = b1 > n_rec || b0 > b1;
    live = !bad;
    me = rec[g];
  }
  contour_tally(bad, &ctr->bad);
  const unsigned long long m = __ballot(live);
  if (m == 0ull) return;  // (the whole wave)
  SkinSweep sw;
  const unsigned slot0 = (unsigned)__shfl((int)slot, __builtin_ctzll(m), 64);
  if (__ballot(live && slot != slot0) == 0ull) {
    // the whole wave in one bucket: uniform bounds, the records by scalar loads
    const unsigned u0 = __builtin_amdgcn_readfirstlane(__shfl((int)b0, __builtin_ctzll(m), 64));
    const unsigned u1 = __builtin_amdgcn_readfirstlane(__shfl((int)b1, __builtin_ctzll(m), 64));
#pragma unroll 4
    for (unsigned i = u0; i < u1; i++) sw.take(rec[i], me.u, me.key);  // (four loads in flight: a scalar load waits for no lane)
  } else if (live) {
    for (unsigned i = b0; i < b1; i++) sw.take(rec[i], me.u, me.key);
  }
  if (!live) return;
  const unsigned long long at = (unsigned long long)b0 + sw.rank;
  if (at >= b1) { atomicAdd(&ctr->bad, 1ull); return; }
  const unsigned before = skin_class(sw.below_mask, K), after = skin_class(sw.upto_mask, K);
  u_sorted[at] = me.u;
  xy_sorted[2ull * at] = rec_xy[2ull * g];
  xy_sorted[2ull * at + 1ull] = rec_xy[2ull * g + 1ull];
  flag[at] = (!sw.led && before != after) ? (unsigned char)(1u + after) : (unsigned char)0;
}

__device__ __forceinline__ bool skin_is_piece(unsigned f) { return f != 0u && f - 1u != SKIN_OUTSIDE; }

__global__ void __launch_bounds__(BLOCK) skin_flags_kernel(const unsigned char* __restrict__ flag, const unsigned* __restrict__ line_start, unsigned n_slots,
                                                           unsigned n_cand, unsigned* __restrict__ blk_bnd, unsigned* __restrict__ blk_piece, SkinCounters* ctr) {
  __shared__ unsigned s_a[4], s_b[4];
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const unsigned n_rec = line_start[n_slots] < n_cand ? line_start[n_slots] : n_cand;
  const unsigned f = g < n_rec ? flag[g] : 0u;
  contour_tally(f != 0u, &ctr->n_bnd);
  contour_tally(skin_is_piece(f), &ctr->n_pieces);
  unsigned bnd, pieces;
  (void)contour_block_excl(f != 0u ? 1u : 0u, s_a, &bnd);
  (void)contour_block_excl(skin_is_piece(f) ? 1u : 0u, s_b, &pieces);
  if (threadIdx.x == 0) { blk_bnd[blockIdx.x] = bnd; blk_piece[blockIdx.x] = pieces; }
}

// bnd_off, piece_off: the boundaries and the pieces before each place (piece_off[n_rec]: all); bnd_pos: boundary -> its place
__global__ void __launch_bounds__(BLOCK) skin_compact_kernel(const unsigned char* __restrict__ flag, const unsigned* __restrict__ line_start, unsigned n_slots,
                                                             unsigned n_cand, const unsigned* __restrict__ base_bnd, const unsigned* __restrict__ base_piece,
                                                             unsigned* __restrict__ bnd_off, unsigned* __restrict__ piece_off, unsigned* __restrict__ bnd_pos,
                                                             SkinCounters* ctr) {
  __shared__ unsigned s_a[4], s_b[4];
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const unsigned n_rec = line_start[n_slots] < n_cand ? line_start[n_slots] : n_cand;
  const unsigned f = g < n_rec ? flag[g] : 0u;
  unsigned t;
  const unsigned b = base_bnd[blockIdx.x] + contour_block_excl(f != 0u ? 1u : 0u, s_a, &t);
  const unsigned p = base_piece[blockIdx.x] + contour_block_excl(skin_is_piece(f) ? 1u : 0u, s_b, &t);
  bool bad = false;
  if (g < n_rec) {
    bnd_off[g] = b;
    piece_off[g] = p;
    if (g + 1ull == n_rec) piece_off[n_rec] = p + (skin_is_piece(f) ? 1u : 0u);
    if (f != 0u) {
      bad = b >= n_cand;
      if (!bad) bnd_pos[b] = (unsigned)g;
    }
  }
  contour_tally(bad, &ctr->bad);
}

// *maxbits: cmeas_maxbits_kernel's result, as cmeas_kernel reads it; the scale 2^(58 - e)
__global__ void __launch_bounds__(BLOCK) skin_piece_kernel(const unsigned char* __restrict__ flag, const double* __restrict__ u_sorted, const unsigned* __restrict__ xy_sorted,
                                                           const unsigned* __restrict__ rec_slot, const int* __restrict__ rec_k, const unsigned* __restrict__ line_start,
                                                           const unsigned* __restrict__ slot_base, unsigned n_layers, unsigned n_slots, unsigned n_cand,
                                                           const unsigned* __restrict__ bnd_off, const unsigned* __restrict__ piece_off,
                                                           const unsigned* __restrict__ bnd_pos, unsigned n_bnd, unsigned n_pieces,
                                                           const unsigned long long* __restrict__ maxbits, unsigned* __restrict__ seg, int* __restrict__ line,
                                                           unsigned char* __restrict__ cls, SkinLayerAcc* acc, SkinCounters* ctr) {
#pragma clang fp contract(off)
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const unsigned n_rec = line_start[n_slots] < n_cand ? line_start[n_slots] : n_cand;
  const unsigned f = g < n_rec ? flag[g] : 0u;
  bool live = skin_is_piece(f), bad = false, zero = false;
  unsigned layer = CONTOUR_NONE, c = 0;
  unsigned long long s[2] = {0ull, 0ull};
  if (live) {
    const unsigned pos = (unsigned)g, b = bnd_off[pos], p = piece_off[pos], slot = rec_slot[pos];
    // the piece ends at the next boundary, which is of the same line: a line ends OUTSIDE
    const unsigned end = b + 1u < n_bnd ? bnd_pos[b + 1u] : n_rec;
    bad = end >= n_rec || end <= pos || p >= n_pieces || slot >= n_slots;
    if (!bad) bad = rec_slot[end] != slot;
    live = !bad;
    if (live) {
      c = f - 1u;
      layer = hatch_bisect(slot_base, n_layers, slot);
      const int k = rec_k[pos];
      const unsigned x0 = xy_sorted[2ull * pos], y0 = xy_sorted[2ull * pos + 1ull], x1 = xy_sorted[2ull * end], y1 = xy_sorted[2ull * end + 1ull];
      seg[4ull * p] = x0;
      seg[4ull * p + 1ull] = y0;
      seg[4ull * p + 2ull] = x1;
      seg[4ull * p + 3ull] = y1;
      line[p] = k;
      cls[p] = (unsigned char)c;
      zero = x0 == x1 && y0 == y1;
      const unsigned biased = (unsigned)(*maxbits >> 23);
      const int e = (int)(biased > 1u ? biased : 1u) - 126;
      cmeas_split(u_sorted[end] - u_sorted[pos], cmeas_pow2(58 - e), &s[0], &s[1]);
      if (k < __atomic_load_n(&acc[layer].k_min, __ATOMIC_RELAXED)) atomicMin(&acc[layer].k_min, k);
      if (k > __atomic_load_n(&acc[layer].k_max, __ATOMIC_RELAXED)) atomicMax(&acc[layer].k_max, k);
    }
  }
  contour_tally(bad, &ctr->bad);
  contour_tally(zero, &ctr->zero_length);
  // a wave inside one layer: one atomic per class and word; a mixed wave: each lane's own
  const unsigned long long m = __ballot(live);
  if (m == 0ull) return;  // (the whole wave)
  const unsigned l0 = (unsigned)__shfl((int)layer, __builtin_ctzll(m), 64);
  if (__ballot(live && layer != l0) == 0ull) {
#pragma unroll
    for (unsigned q = 0; q < 4u; q++) {
      const bool mine = live && c == q;
      const unsigned long long members = __ballot(mine);
      if (members == 0ull) continue;
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const unsigned long long t = cmeas_wave_sum(mine ? s[k] : 0ull);
        if ((threadIdx.x & 63u) == 0u && t) atomicAdd(&acc[l0].sum[q][k], t);
      }
      if ((threadIdx.x & 63u) == 0u) atomicAdd(&acc[l0].n[q], (unsigned long long)__builtin_popcountll(members));
    }
  } else if (live) {
#pragma unroll
    for (int k = 0; k < 2; k++)
      if (s[k]) atomicAdd(&acc[layer].sum[c][k], s[k]);
    atomicAdd(&acc[layer].n[c], 1ull);
  }
}

__global__ void __launch_bounds__(BLOCK) skin_layer_start_kernel(const unsigned* __restrict__ line_start, const unsigned* __restrict__ slot_base,
                                                                 const unsigned* __restrict__ piece_off, unsigned n_layers, unsigned n_slots, unsigned n_cand,
                                                                 unsigned* __restrict__ layer_start) {
  const unsigned long long l = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  if (l > n_layers) return;
  const unsigned n_rec = line_start[n_slots] < n_cand ? line_start[n_slots] : n_cand;
  const unsigned at = line_start[slot_base[l]];
  layer_start[l] = piece_off[at < n_rec ? at : n_rec];
}
