// kernels_dc_indexed.h -- dual contouring straight to an indexed mesh: the quad stage of gsdf_hip_mesh_dualcontour_indexed
// (include/gsdf_hip.h: "indexed meshes: dual contouring" states the contract; abi_mesh.hip launches these after dc_place_kernel, in
// the place of dc_quads_kernel). Not part of the run-time specialiser's sources: no kernel here evaluates the field.
//
// dc_quads_kernel has the four cube indices of every quad in registers and copies 6 x 12 bytes of fv per quad to wherever its
// workgroup's atomic landed. Here the four indices are the output, and they are put into LATTICE ORDER -- quads by (z, y, x, axis),
// the order the reference emits them in -- by a counting sort over the lattice rows (z, y), without a library sort:
//   dci_count_kernel      A  one lane per active edge: dc_quads_kernel's validity test; a valid quad takes a place in its row with
//                            ONE returning atomicAdd on the row's counter (n^2 counters: they spread, unlike the lists' words) and
//                            leaves its four cubes, flipped as the reference flips them, and that place at its edge's index
//   dci_row_sum_kernel    B  exclusive scan of the rows' counts: sums of 256 rows, the scan across them (kernels_weld.h:
//   dci_row_base_kernel      block_scan_kernel, launched by abi_indexed.hip), a row's base = its block's carry + its rank inside
//   dci_scatter_kernel    C  a valid quad writes x << 2 | axis and its edge's index at row base + place: the row's segment, unordered
//   dci_rank_kernel       D  an entry's rank in its row = the entries of the segment with a smaller x << 2 | axis (they are distinct:
//                            an edge is listed once); its six slots' cube indices go to 6 (row base + rank)
// Which place a quad takes in A depends on the order of arrival; C puts it there and D reads the whole segment, so nothing of it
// reaches the output. Bytes per quad: A writes 20, C reads 4 + writes 8, D reads 8 + 16 + the row's segment (4 bytes per entry of
// the row, from cache: the lanes of a wave sit in the same one or two rows) and writes 24; per lattice row 4 (clear) + 12 (scan).
#pragma once
#include "kernels_dc.h"

// What holds by construction, and what is done about it if it should not: the rows' segments tile [0, n_quads) and a row's places
// are 0 .. count - 1, each taken once, so C writes every entry once and D every slot once, with a cube index that came out of the
// grid (>= 0, below the cubes' capacity). C and D test what they index by all the same, and a test that fails is COUNTED in *bad and
// the write left out; the host reads *bad before the slots are numbered and fails the call (nothing reads a slot that was not written).
#define DCI_NONE 0xffffffffu  // place of an edge without a quad

// Pass A. place[e], quad[e]: indexed like edges[] (part p's share starts at p * edge_cap / DC_PARTS). row_cnt[n * n] cleared.
__global__ void __launch_bounds__(BLOCK) dci_count_kernel(const Cube* __restrict__ cubes, const float4* __restrict__ dists, const unsigned* __restrict__ edges,
                                                          unsigned long long edge_cap, const int* __restrict__ grid, int nshift,
                                                          unsigned* __restrict__ row_cnt, unsigned* __restrict__ place, uint4* __restrict__ quad,
                                                          DCCounters* __restrict__ ctr) {
  const unsigned long long eseg = edge_cap / DC_PARTS;
  unsigned long long np[DC_PARTS];
  const unsigned long long n = dc_part_counts<false>(ctr->edges_w, eseg, np);  // the edges of all parts, one after the other
  const int nn = 1 << nshift;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t base = (uint64_t)blockIdx.x * BLOCK; base < n; base += step) {
    unsigned pp = 0;
    unsigned long long kk = 0;
    if (!dc_flat_to_part(base + threadIdx.x, np, pp, kk)) continue;
    const uint64_t ei = (uint64_t)pp * eseg + kk;
    const unsigned e = edges[ei];
    const unsigned ci = e >> 2, a = e & 3u;
    const Cube c = cubes[ci];
    const float4 d = dists[ci];
    const bool flip = nb::lt0((a == 0 ? d.y : (a == 1 ? d.z : d.w)) - d.x);
    // EdgeNeighborsX/Y/Z (dual_contour.go:271-287): offsets in cube units, as dc_quads_kernel has them
    const int off[3][4][3] = {{{0, -1, -1}, {0, 0, -1}, {0, 0, 0}, {0, -1, 0}},
                              {{-1, 0, -1}, {-1, 0, 0}, {0, 0, 0}, {0, 0, -1}},
                              {{-1, -1, 0}, {0, -1, 0}, {0, 0, 0}, {-1, 0, 0}}};
    int q[4] = {-1, -1, -1, -1};
    bool ok = true;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int x = c.x + off[a][k][0], y = c.y + off[a][k][1], z = c.z + off[a][k][2];
      int idx = -1;
      if (x >= 0 && y >= 0 && z >= 0 && x < nn && y < nn && z < nn) idx = grid[((size_t)z * nn + y) * nn + x];
      q[k] = idx;
      ok = ok && idx >= 0;
    }
    unsigned pl = DCI_NONE;
    if (ok) {
      pl = atomicAdd(&row_cnt[((unsigned)c.z << nshift) + (unsigned)c.y], 1u);
      quad[ei] = flip ? make_uint4((unsigned)q[3], (unsigned)q[2], (unsigned)q[1], (unsigned)q[0])
                      : make_uint4((unsigned)q[0], (unsigned)q[1], (unsigned)q[2], (unsigned)q[3]);
    }
    place[ei] = pl;
  }
}

// Pass B, around block_scan_kernel: blk_cnt[b] = quads of rows [256 b, 256 b + 256) ...
__global__ void __launch_bounds__(BLOCK) dci_row_sum_kernel(const unsigned* __restrict__ row_cnt, unsigned n_rows, unsigned* __restrict__ blk_cnt) {
  __shared__ unsigned s_w[4];
  const unsigned r = blockIdx.x * BLOCK + threadIdx.x;
  const unsigned incl = wave_incl_scan_u32(r < n_rows ? row_cnt[r] : 0u);
  if ((threadIdx.x & 63u) == 63u) s_w[threadIdx.x >> 6] = incl;
  __syncthreads();
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
// ... and row_base[r] = blk_base[r / 256] + the quads of the block's rows before r.
__global__ void __launch_bounds__(BLOCK) dci_row_base_kernel(const unsigned* __restrict__ row_cnt, unsigned n_rows, const unsigned* __restrict__ blk_base,
                                                             unsigned* __restrict__ row_base) {
  __shared__ unsigned s_w[4];
  const unsigned r = blockIdx.x * BLOCK + threadIdx.x, wave = threadIdx.x >> 6;
  const unsigned mine = r < n_rows ? row_cnt[r] : 0u;
  const unsigned incl = wave_incl_scan_u32(mine);
  if ((threadIdx.x & 63u) == 63u) s_w[wave] = incl;
  __syncthreads();
  const unsigned before = (wave > 0 ? s_w[0] : 0u) + (wave > 1 ? s_w[1] : 0u) + (wave > 2 ? s_w[2] : 0u) + (incl - mine);
  if (r < n_rows) row_base[r] = blk_base[blockIdx.x] + before;
}

// Pass C. xa[n_quads], src[n_quads].
__global__ void __launch_bounds__(BLOCK) dci_scatter_kernel(const Cube* __restrict__ cubes, const unsigned* __restrict__ edges, unsigned long long edge_cap,
                                                            int nshift, const unsigned* __restrict__ row_base, const unsigned* __restrict__ place,
                                                            unsigned long long n_quads, unsigned* __restrict__ xa, unsigned* __restrict__ src,
                                                            unsigned long long* __restrict__ bad, DCCounters* __restrict__ ctr) {
  const unsigned long long eseg = edge_cap / DC_PARTS;
  unsigned long long np[DC_PARTS];
  const unsigned long long n = dc_part_counts<false>(ctr->edges_w, eseg, np);
  const uint64_t step = (uint64_t)gridDim.x * BLOCK;
  for (uint64_t base = (uint64_t)blockIdx.x * BLOCK; base < n; base += step) {
    unsigned pp = 0;
    unsigned long long kk = 0;
    if (!dc_flat_to_part(base + threadIdx.x, np, pp, kk)) continue;
    const uint64_t ei = (uint64_t)pp * eseg + kk;
    const unsigned pl = place[ei];
    if (pl == DCI_NONE) continue;
    const unsigned e = edges[ei];
    const Cube c = cubes[e >> 2];
    const unsigned long long at = (unsigned long long)row_base[((unsigned)c.z << nshift) + (unsigned)c.y] + pl;
    if (at >= n_quads) { atomicAdd(bad, 1ull); continue; }
    xa[at] = ((unsigned)c.x << 2) | (e & 3u);
    src[at] = (unsigned)ei;  // (edge_cap = 3 x the cubes' capacity, and a cube's index has 30 bits: below 2^32)
  }
}

// Pass D. slot_cube[6 n_quads]: quad g = faces 2 g = (q0, q1, q2) and 2 g + 1 = (q2, q3, q0), slot 3 t + c -> the cube of corner c.
__global__ void __launch_bounds__(BLOCK) dci_rank_kernel(const Cube* __restrict__ cubes, const unsigned* __restrict__ edges, unsigned long long edge_cap, int nshift,
                                                         const unsigned* __restrict__ row_base, const unsigned* __restrict__ row_cnt,
                                                         const unsigned* __restrict__ xa, const unsigned* __restrict__ src, const uint4* __restrict__ quad,
                                                         unsigned long long n_quads, unsigned long long n_cubes, unsigned* __restrict__ slot_cube,
                                                         unsigned long long* __restrict__ bad) {
  const unsigned long long p = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  if (p >= n_quads) return;
  const unsigned ei = src[p];
  if ((unsigned long long)ei >= edge_cap) { atomicAdd(bad, 1ull); return; }
  const Cube c = cubes[edges[ei] >> 2];
  const unsigned row = ((unsigned)c.z << nshift) + (unsigned)c.y;
  const unsigned long long rb = row_base[row], len = row_cnt[row];
  const uint4 o = quad[ei];
  if (rb + len > n_quads || o.x >= n_cubes || o.y >= n_cubes || o.z >= n_cubes || o.w >= n_cubes) { atomicAdd(bad, 1ull); return; }
  const unsigned mine = xa[p];
  unsigned rank = 0;
  for (unsigned long long j = 0; j < len; j++) rank += xa[rb + j] < mine ? 1u : 0u;
  if (rank >= len) { atomicAdd(bad, 1ull); return; }  // (its own entry is in the segment and is not smaller than itself)
  const unsigned long long g = rb + rank;
  unsigned* dst = slot_cube + 6ull * g;
  dst[0] = o.x; dst[1] = o.y; dst[2] = o.z;
  dst[3] = o.z; dst[4] = o.w; dst[5] = o.x;
}
