// kernels_contour.h -- part outlines and z-slices as ordered closed loops (include/gsdf_hip.h, section "contours", states the
// arithmetic; tests/contourref.py restates it in numpy). One chunk of whole layers per sequence of launches (abi_contour.hip):
//   contour_pos_kernel<DIM>     the chunk's lattice positions, for the program's ordinary Evaluate (gsdf_hip_eval2_dev / eval3_dev)
//   contour_cells_kernel        one lane per cell: its case, succ[tail] = head for its segments, the node statistics
//   contour_count_kernel        cut edges per block of 256 edge slots -> the carry across blocks (abi_host.h: launch_block_scan)
//   contour_layer_base_kernel   the first vertex number of every layer of the chunk, and their total
//   contour_number_kernel       cut edge -> vertex number, in (layer, key) order
//   contour_link_kernel         succ in vertex numbers, its inverse pred; the first state of the minimum pass
//   contour_min_kernel          one round of pointer jumping: the smallest vertex number of each cycle (its leader)
//   contour_rank_init_kernel, contour_rank_kernel   Wyllie's list ranking along pred, the cycle cut in front of its leader
//   contour_leader_count_kernel, contour_leader_number_kernel   leaders -> loop numbers and loop starts, in (layer, leader) order
//   contour_emit_kernel         every vertex to loop_start + rank: its coordinates, its key
// No atomics on the data path (every succ / pred slot has one writer), integers only behind the cell pass; a slot is g = layer * E +
// key with E = 2 nx ny edge keys per layer, below 2^32 for a chunk (the host sizes chunks so).
#pragma once
#include "kernels_common.h"

#define CONTOUR_NONE 0xffffffffu

struct ContourCounters {
  unsigned long long border_inside, nonfinite_nodes, saddle_cells;
  unsigned long long bad;  // a link or a destination out of range: cannot happen (succ is a permutation of the cut edges); checked, not trusted
};

struct ContourLattice {
  unsigned nx, ny;
  float x0, y0, res;
};

__device__ __forceinline__ float contour_coord(float c0, unsigned i, float res) { return c0 + (float)i * res; }

// exclusive prefix of v over the workgroup (every thread calls it; s_w: 4 words of LDS of its own per call site)
__device__ __forceinline__ unsigned contour_block_excl(unsigned v, unsigned* s_w, unsigned* total) {
  const unsigned incl = wave_incl_scan_u32(v), wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63u) == 63u) s_w[wave] = incl;
  __syncthreads();
  const unsigned w0 = s_w[0], w1 = s_w[1], w2 = s_w[2], w3 = s_w[3];
  *total = w0 + w1 + w2 + w3;
  return (wave > 0 ? w0 : 0u) + (wave > 1 ? w1 : 0u) + (wave > 2 ? w2 : 0u) + incl - v;
}

// one atomic per wave and counter; every lane of the wave calls it
__device__ __forceinline__ void contour_tally(bool flag, unsigned long long* ctr) {
  const unsigned long long m = __ballot(flag);
  if (m != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(ctr, (unsigned long long)__builtin_popcountll(m));
}

template <int DIM>
__global__ void __launch_bounds__(BLOCK) contour_pos_kernel(ContourLattice lat, const float* __restrict__ z, unsigned long long n_nodes, float* __restrict__ pos) {
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= n_nodes) return;
  const unsigned long long per = (unsigned long long)lat.nx * lat.ny;
  const unsigned layer = (unsigned)(g / per), n = (unsigned)(g % per);
  const unsigned j = n / lat.nx, i = n % lat.nx;
  float* dst = pos + (unsigned long long)DIM * g;
  dst[0] = contour_coord(lat.x0, i, lat.res);
  dst[1] = contour_coord(lat.y0, j, lat.res);
  if (DIM == 3) dst[2] = z[layer];
}

// A node is inside iff d < 0 (false for NaN and both zeros) and it is not on the lattice border.
__device__ __forceinline__ bool contour_inside(const ContourLattice& lat, unsigned i, unsigned j, float d) {
  return nb::lt0(d) && i > 0u && j > 0u && i + 1u < lat.nx && j + 1u < lat.ny;
}

// The segments of the sixteen cases, corners c0 (i, j), c1 (i+1, j), c2 (i+1, j+1), c3 (i, j+1), case = sum of 2^c over the inside
// corners; cell edges B 0 (bottom), R 1, T 2, L 3; a nibble per case: tail | head << 2, the part on the left of tail -> head.
// Cases 5 and 10 have a second segment (T -> R, L -> T): the two inside corners of a saddle are never joined.
#define CONTOUR_SEG0 0x0347918BE2C6D1C0ull

__global__ void __launch_bounds__(BLOCK) contour_cells_kernel(ContourLattice lat, const float* __restrict__ dist, unsigned long long n_nodes,
                                                              unsigned* __restrict__ succ, ContourCounters* __restrict__ ctr) {
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const bool live = g < n_nodes;
  bool border_in = false, nonfinite = false, saddle = false;
  if (live) {
    const unsigned per = lat.nx * lat.ny;
    const unsigned layer = (unsigned)(g / per), n = (unsigned)(g % per);
    const unsigned j = n / lat.nx, i = n % lat.nx;
    const float d0 = dist[g];
    const bool in0 = contour_inside(lat, i, j, d0);
    border_in = nb::lt0(d0) && !in0;
    nonfinite = nb::nan_or_inf(d0);
    if (i + 1u < lat.nx && j + 1u < lat.ny) {
      const bool in1 = contour_inside(lat, i + 1u, j, dist[g + 1]);
      const bool in2 = contour_inside(lat, i + 1u, j + 1u, dist[g + lat.nx + 1]);
      const bool in3 = contour_inside(lat, i, j + 1u, dist[g + lat.nx]);
      const unsigned c = (in0 ? 1u : 0u) | (in1 ? 2u : 0u) | (in2 ? 4u : 0u) | (in3 ? 8u : 0u);
      saddle = c == 5u || c == 10u;
      if (c != 0u && c != 15u) {
        const unsigned base = layer * (2u * per);  // (< 2^32: the host sizes chunks so)
        // slots of the cell's edges B, R, T, L
        const unsigned e[4] = {base + 2u * n, base + 2u * (n + 1u) + 1u, base + 2u * (n + lat.nx), base + 2u * n + 1u};
        const unsigned s = (unsigned)(CONTOUR_SEG0 >> (4u * c)) & 15u;
        const unsigned t0 = s & 3u, h0 = s >> 2;
        succ[t0 == 0u ? e[0] : (t0 == 1u ? e[1] : (t0 == 2u ? e[2] : e[3]))] = h0 == 0u ? e[0] : (h0 == 1u ? e[1] : (h0 == 2u ? e[2] : e[3]));
        if (c == 5u) succ[e[2]] = e[1];
        if (c == 10u) succ[e[3]] = e[2];
      }
    }
  }
  contour_tally(border_in, &ctr->border_inside);
  contour_tally(nonfinite, &ctr->nonfinite_nodes);
  contour_tally(saddle, &ctr->saddle_cells);
}

__global__ void __launch_bounds__(BLOCK) contour_count_kernel(const unsigned* __restrict__ succ, unsigned long long n_slots, unsigned* __restrict__ blk_cnt) {
  __shared__ unsigned s_w[4];
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  unsigned total;
  (void)contour_block_excl(g < n_slots && succ[g] != CONTOUR_NONE ? 1u : 0u, s_w, &total);
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = total;
}

// layer_base[l] = cut edges in slots below l * per_layer (l < n_layers); layer_base[n_layers] = the chunk's total
__global__ void __launch_bounds__(BLOCK) contour_layer_base_kernel(const unsigned* __restrict__ succ, const unsigned* __restrict__ blk_base,
                                                                   const unsigned long long* __restrict__ total, unsigned per_layer, unsigned n_layers,
                                                                   unsigned* __restrict__ layer_base) {
  const unsigned l = blockIdx.x * BLOCK + threadIdx.x;
  if (l > n_layers) return;
  if (l == n_layers) { layer_base[l] = (unsigned)*total; return; }
  const unsigned long long g = (unsigned long long)l * per_layer;
  unsigned acc = blk_base[g / BLOCK];
  for (unsigned long long k = g - g % BLOCK; k < g; k++) acc += succ[k] != CONTOUR_NONE ? 1u : 0u;
  layer_base[l] = acc;
}

__global__ void __launch_bounds__(BLOCK) contour_number_kernel(const unsigned* __restrict__ succ, unsigned long long n_slots, const unsigned* __restrict__ blk_base,
                                                               unsigned n_verts, unsigned* __restrict__ vnum, unsigned* __restrict__ slot_of,
                                                               ContourCounters* __restrict__ ctr) {
  __shared__ unsigned s_w[4];
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const bool cut = g < n_slots && succ[g] != CONTOUR_NONE;
  unsigned total;
  const unsigned v = blk_base[blockIdx.x] + contour_block_excl(cut ? 1u : 0u, s_w, &total);
  if (!cut) return;
  if (v >= n_verts) { atomicAdd(&ctr->bad, 1ull); return; }
  vnum[g] = v;
  slot_of[v] = (unsigned)g;
}

__global__ void __launch_bounds__(BLOCK) contour_link_kernel(const unsigned* __restrict__ succ, unsigned long long n_slots, const unsigned* __restrict__ vnum,
                                                             const unsigned* __restrict__ slot_of, unsigned n_verts, unsigned* __restrict__ pred,
                                                             unsigned* __restrict__ mn, unsigned* __restrict__ nxt, ContourCounters* __restrict__ ctr) {
  const unsigned v = blockIdx.x * BLOCK + threadIdx.x;
  if (v >= n_verts) return;
  const unsigned head = succ[slot_of[v]];
  unsigned s = head < n_slots && succ[head] != CONTOUR_NONE ? vnum[head] : CONTOUR_NONE;
  if (s >= n_verts) { atomicAdd(&ctr->bad, 1ull); s = v; }
  pred[s] = v;
  mn[v] = v;
  nxt[v] = s;
}

__global__ void __launch_bounds__(BLOCK) contour_min_kernel(const unsigned* __restrict__ mn_in, const unsigned* __restrict__ nxt_in, unsigned n_verts,
                                                            unsigned* __restrict__ mn_out, unsigned* __restrict__ nxt_out) {
  const unsigned v = blockIdx.x * BLOCK + threadIdx.x;
  if (v >= n_verts) return;
  const unsigned n = nxt_in[v], a = mn_in[v], b = mn_in[n];
  mn_out[v] = a < b ? a : b;
  nxt_out[v] = nxt_in[n];
}

// the list of a loop runs along pred from any vertex back to the leader: rank = hops to the leader = the place behind it along succ
__global__ void __launch_bounds__(BLOCK) contour_rank_init_kernel(const unsigned* __restrict__ leader, const unsigned* __restrict__ pred, unsigned n_verts,
                                                                  unsigned* __restrict__ rank, unsigned* __restrict__ link) {
  const unsigned v = blockIdx.x * BLOCK + threadIdx.x;
  if (v >= n_verts) return;
  const bool is_leader = leader[v] == v;
  rank[v] = is_leader ? 0u : 1u;
  link[v] = is_leader ? CONTOUR_NONE : pred[v];
}

__global__ void __launch_bounds__(BLOCK) contour_rank_kernel(const unsigned* __restrict__ rank_in, const unsigned* __restrict__ link_in, unsigned n_verts,
                                                             unsigned* __restrict__ rank_out, unsigned* __restrict__ link_out) {
  const unsigned v = blockIdx.x * BLOCK + threadIdx.x;
  if (v >= n_verts) return;
  const unsigned p = link_in[v];
  unsigned r = rank_in[v], q = CONTOUR_NONE;
  if (p != CONTOUR_NONE) { r += rank_in[p]; q = link_in[p]; }
  rank_out[v] = r;
  link_out[v] = q;
}

// per block of vertices: its leaders, and the vertices of their loops (a loop's length is the rank of the leader's predecessor + 1)
__global__ void __launch_bounds__(BLOCK) contour_leader_count_kernel(const unsigned* __restrict__ leader, const unsigned* __restrict__ pred,
                                                                     const unsigned* __restrict__ rank, unsigned n_verts, unsigned* __restrict__ blk_loops,
                                                                     unsigned* __restrict__ blk_len) {
  __shared__ unsigned s_a[4], s_b[4];
  const unsigned v = blockIdx.x * BLOCK + threadIdx.x;
  const bool is_leader = v < n_verts && leader[v] == v;
  const unsigned len = is_leader ? rank[pred[v]] + 1u : 0u;
  unsigned loops, verts;
  (void)contour_block_excl(is_leader ? 1u : 0u, s_a, &loops);
  (void)contour_block_excl(len, s_b, &verts);
  if (threadIdx.x == 0) { blk_loops[blockIdx.x] = loops; blk_len[blockIdx.x] = verts; }
}

__global__ void __launch_bounds__(BLOCK) contour_leader_number_kernel(const unsigned* __restrict__ leader, const unsigned* __restrict__ pred,
                                                                      const unsigned* __restrict__ rank, const unsigned* __restrict__ slot_of, unsigned n_verts,
                                                                      const unsigned* __restrict__ base_loops, const unsigned* __restrict__ base_len,
                                                                      unsigned n_loops, unsigned per_layer, unsigned layer0, unsigned vert0,
                                                                      unsigned* __restrict__ start_of, unsigned* __restrict__ loop_start,
                                                                      unsigned* __restrict__ loop_layer, ContourCounters* __restrict__ ctr) {
  __shared__ unsigned s_a[4], s_b[4];
  const unsigned v = blockIdx.x * BLOCK + threadIdx.x;
  const bool is_leader = v < n_verts && leader[v] == v;
  const unsigned len = is_leader ? rank[pred[v]] + 1u : 0u;
  unsigned t;
  const unsigned loop = base_loops[blockIdx.x] + contour_block_excl(is_leader ? 1u : 0u, s_a, &t);
  const unsigned start = base_len[blockIdx.x] + contour_block_excl(len, s_b, &t);
  if (!is_leader) return;
  start_of[v] = start;
  if (loop >= n_loops) { atomicAdd(&ctr->bad, 1ull); return; }
  loop_start[loop] = vert0 + start;
  loop_layer[loop] = layer0 + slot_of[v] / per_layer;
}

// The vertex of a cut edge (gsdf_hip.h, "Vertices"): t = d_lo / (d_lo - d_hi) when both distances are finite and the outside node
// has d >= 0, else one half; the cut coordinate is c_lo + t res, the other one the node's own. Correctly rounded float32 throughout
// (this unit is built with -ffp-contract=off and without fast-math: `/` is the IEEE division).
__global__ void __launch_bounds__(BLOCK) contour_emit_kernel(ContourLattice lat, const float* __restrict__ dist, const unsigned* __restrict__ slot_of,
                                                             const unsigned* __restrict__ leader, const unsigned* __restrict__ rank,
                                                             const unsigned* __restrict__ start_of, unsigned n_verts, unsigned per_layer,
                                                             float* __restrict__ xy, unsigned* __restrict__ keys, ContourCounters* __restrict__ ctr) {
  const unsigned v = blockIdx.x * BLOCK + threadIdx.x;
  if (v >= n_verts) return;
  const unsigned g = slot_of[v];
  const unsigned layer = g / per_layer, key = g % per_layer;
  const unsigned axis = key & 1u, n = key >> 1;
  const unsigned j = n / lat.nx, i = n % lat.nx;
  const unsigned long long node = (unsigned long long)layer * (per_layer >> 1) + n;
  const float d_lo = dist[node], d_hi = dist[node + (axis ? lat.nx : 1u)];
  const bool lo_in = contour_inside(lat, i, j, d_lo);
  const float d_out = lo_in ? d_hi : d_lo;
  float t = 0.5f;
  if (!nb::nan_or_inf(d_lo) && !nb::nan_or_inf(d_hi) && nb::ge0(d_out)) t = d_lo / (d_lo - d_hi);
  const float step = t * lat.res;
  const float x = contour_coord(lat.x0, i, lat.res), y = contour_coord(lat.y0, j, lat.res);
  const unsigned dst = start_of[leader[v]] + rank[v];
  if (dst >= n_verts) { atomicAdd(&ctr->bad, 1ull); return; }
  xy[2ull * dst] = axis ? x : x + step;
  xy[2ull * dst + 1ull] = axis ? y + step : y;
  keys[dst] = key;
}
