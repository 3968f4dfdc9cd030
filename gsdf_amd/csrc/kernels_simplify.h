// kernels_simplify.h -- an indexed mesh made smaller by vertex clustering: used vertices fall into the cells of a cubic grid, a
// cluster is the set of vertices of one cell, its position their mean, and the faces that still span three clusters are kept
// (include/gsdf_hip.h: "indexed meshes: simplify" states the contract; abi_indexed.hip launches these; a numpy restatement:
// tests/simplifyref.py). Independent of any SDF tree: these kernels live in the shipped code object only.
//
//   simplify_mark_kernel     a face per lane: its three vertices are USED (plain stores of one value); degenerate faces counted
//   topo_maxbits_kernel      (kernels_topo.h) the exponent e of the contract
//   simplify_insert_kernel   a used vertex per lane: its key (two float64 operations and a floor per coordinate), the key into the
//                            open-addressing table (kernels_weld.h: table_claim), 32-bit atomicMin of the vertex number on the cell's
//                            label; vcell[v] = the cell. Non-finite and out-of-range vertices are counted and left out.
//   simplify_sum_kernel      once the table is settled, a vertex per lane: n += 1 and S_k += q_k on its cell's record, 64-bit
//                            integer atomics (kernels_topo.h: topo_count / topo_add, one atomic per wave where the wave is of one cell)
//   simplify_faces_kernel    a face per lane: kept iff non-degenerate and its corners are three distinct cells; the cells of a kept
//                            face are flagged; kept faces counted per block of 256 (collapsed = non-degenerate - kept)
//   simplify_place_kernel    cells, grid-stride: the largest n, the number of flagged cells, and (not in a dry run) the flagged
//                            cells' positions by the contract, float64
//   topo_compact_kernel .. topo_renumber_kernel, remap_kernel   (kernels_topo.h, kernels_weld.h) extract's kernels, with the table's
//                            cell standing where extract has the old vertex number: kept faces in order, clusters numbered by
//                            their smallest kept slot, positions and keys gathered from the per-cell arrays
//
// Every sum is an integer sum and every label a minimum, so neither the order in which threads arrive nor the cell a key happens to
// land in changes a bit of the result.
#pragma once
#include "kernels_common.h"
#include "kernels_weld.h"
#include "kernels_topo.h"

#define SIMPLIFY_KIND 4ull        // after the weld's kinds 0 .. 3; bits 60 .. 63 = 0100: never WELD_EMPTY_KEY
#define SIMPLIFY_BIAS 524288.0    // 2^19
static_assert(((SIMPLIFY_KIND << 60) | 0x0fffffffffffffffull) != WELD_EMPTY_KEY, "a cluster key cannot be the table's empty value");

// What the host reads after every attempt of the table (table_build: a head record begins with its TableCounters). tab .. used -- what
// simplify_insert_kernel counts -- are cleared for every attempt (SIMPLIFY_HEAD_RESET_BYTES), maxbits and degenerate once.
struct SimplifyHead {
  TableCounters tab;
  unsigned long long nonfinite;     // used vertices with a NaN or infinite coordinate
  unsigned long long out_of_range;  // used vertices with some |c_k| >= 2^19
  unsigned long long first_bad;     // 0xffffffff - the smallest of those vertices
  unsigned long long used;          // used vertices
  unsigned long long maxbits;       // topo_maxbits_kernel
  unsigned long long degenerate;    // simplify_mark_kernel
};
#define SIMPLIFY_HEAD_RESET_BYTES offsetof(SimplifyHead, maxbits)
struct SimplifyTail {
  unsigned long long kept;     // block_scan_kernel over simplify_faces_kernel's counts: the kept faces
  unsigned long long named;    // simplify_place_kernel: cells a kept face names
  unsigned long long largest;  // ... the largest n
};
struct SimplifyCounters {
  SimplifyHead head;
  SimplifyTail tail;
};
// One record per table cell: the cluster's count and the integer sums of its members' quantised coordinates (two's complement).
struct SimplifyCell {
  unsigned long long n;
  unsigned long long s[3];
};
#define SIMPLIFY_F_N 0
#define SIMPLIFY_F_SUM 1

__global__ void __launch_bounds__(BLOCK) simplify_mark_kernel(const unsigned* __restrict__ idx, unsigned long long n_tris, unsigned* __restrict__ used,
                                                              SimplifyHead* __restrict__ head) {
  const unsigned long long f = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  bool deg = false;
  if (f < n_tris) {
    const unsigned a = idx[3ull * f], b = idx[3ull * f + 1ull], c = idx[3ull * f + 2ull];
    deg = a == b || b == c || a == c;
    if (!deg) { used[a] = 1u; used[b] = 1u; used[c] = 1u; }  // (plain stores of one value)
  }
  const unsigned n_deg = (unsigned)__builtin_popcountll(__ballot(deg));
  if ((threadIdx.x & 63u) == 0u && n_deg) atomicAdd(&head->degenerate, (unsigned long long)n_deg);
}

// tab_key[cells] and tab_label[cells] = 0xff.. before the pass (one memset); mask = cells - 1. ox, oy, oz, cell: the options as float64.
__global__ void __launch_bounds__(BLOCK) simplify_insert_kernel(const float* __restrict__ verts, const unsigned* __restrict__ used, unsigned long long n_verts,
                                                                double ox, double oy, double oz, double cell, unsigned long long* __restrict__ tab_key,
                                                                unsigned* __restrict__ tab_label, unsigned mask, unsigned* __restrict__ vcell,
                                                                SimplifyHead* __restrict__ head) {
#pragma clang fp contract(off)
  unsigned my_probes = 0, my_new = 0, my_used = 0, my_nonfinite = 0, my_range = 0, my_bad = 0xffffffffu;
  bool lost = false;
  const double o[3] = {ox, oy, oz};
  const unsigned long long step = (unsigned long long)gridDim.x * BLOCK;
  for (unsigned long long v = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; v < n_verts; v += step) {
    unsigned at = TOPO_NONE;
    if (used[v] != 0u) {
      my_used++;
      const float p[3] = {verts[3ull * v], verts[3ull * v + 1ull], verts[3ull * v + 2ull]};
      bool finite = true, inside = true;
      unsigned long long key = SIMPLIFY_KIND << 60;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        finite = finite && (__float_as_uint(p[k]) & 0x7fffffffu) < 0x7f800000u;
        const double c = __builtin_floor(((double)p[k] - o[k]) / cell);
        const bool ok = __builtin_fabs(c) < SIMPLIFY_BIAS;  // (false for a NaN)
        inside = inside && ok;
        key |= (unsigned long long)(ok ? (long long)(c + SIMPLIFY_BIAS) : 0ll) << (20 * k);
      }
      if (!finite) {
        my_nonfinite++;
      } else if (!inside) {
        my_range++;
        my_bad = min(my_bad, (unsigned)v);
      } else {
        const unsigned long long h = table_claim(tab_key, mask, key, &my_probes, &my_new);
        if (h != TABLE_NONE) {
          atomicMin(&tab_label[h], (unsigned)v);
          at = (unsigned)h;
        } else {
          lost = true;
        }
      }
    }
    vcell[v] = at;
  }
  table_stats(my_probes, my_new, lost, &head->tab);
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    my_used += __shfl_down(my_used, off, 64);
    my_nonfinite += __shfl_down(my_nonfinite, off, 64);
    my_range += __shfl_down(my_range, off, 64);
    my_bad = min(my_bad, (unsigned)__shfl_down(my_bad, off, 64));
  }
  if ((threadIdx.x & 63u) == 0u) {
    if (my_used) atomicAdd(&head->used, (unsigned long long)my_used);
    if (my_nonfinite) atomicAdd(&head->nonfinite, (unsigned long long)my_nonfinite);
    if (my_range) {
      atomicAdd(&head->out_of_range, (unsigned long long)my_range);
      atomicMax(&head->first_bad, (unsigned long long)(0xffffffffu - my_bad));
    }
  }
}

// acc[cells] = 0 before the pass. scale: the power of two 2^(30 - e).
__global__ void __launch_bounds__(BLOCK) simplify_sum_kernel(const float* __restrict__ verts, const unsigned* __restrict__ vcell, unsigned long long n_verts,
                                                             double scale, SimplifyCell* __restrict__ acc) {
#pragma clang fp contract(off)
  const unsigned long long v = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const unsigned at = v < n_verts ? vcell[v] : TOPO_NONE;
  unsigned long long q[3] = {0ull, 0ull, 0ull};
  if (at != TOPO_NONE) {
#pragma unroll
    for (int k = 0; k < 3; k++) q[k] = (unsigned long long)(long long)__builtin_rint((double)verts[3ull * v + k] * scale);  // |q| <= 2^30
  }
  const TopoWave w = topo_wave(at);
  topo_count(w, at, true, acc, SIMPLIFY_F_N);
#pragma unroll
  for (int k = 0; k < 3; k++) topo_add(w, at, q[k], acc, SIMPLIFY_F_SUM + k);
}

// flag[cells] = 0 before the pass. keep, fcell: NULL in a dry run (both or none). fcell[3 f + c] = the cell of corner c (0 for a face
// that is not kept); blk_cnt[b] = kept faces among [256 b, 256 b + 256): their sum (block_scan_kernel) is n_tris, and the collapsed
// faces are the non-degenerate ones that are not among them -- no counter word that every wave would have to add to.
__global__ void __launch_bounds__(BLOCK) simplify_faces_kernel(const unsigned* __restrict__ idx, unsigned long long n_tris, const unsigned* __restrict__ vcell,
                                                               unsigned* __restrict__ flag, unsigned char* __restrict__ keep, unsigned* __restrict__ fcell,
                                                               unsigned* __restrict__ blk_cnt) {
  __shared__ unsigned s_w[4];
  const unsigned long long f = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  bool kept = false;
  if (f < n_tris) {
    const unsigned a = idx[3ull * f], b = idx[3ull * f + 1ull], c = idx[3ull * f + 2ull];
    unsigned ca = 0u, cb = 0u, cc = 0u;
    if (!(a == b || b == c || a == c)) {
      ca = vcell[a]; cb = vcell[b]; cc = vcell[c];
      const bool placed = ca != TOPO_NONE && cb != TOPO_NONE && cc != TOPO_NONE;  // (always: every used vertex has its cell by now)
      kept = placed && !(ca == cb || cb == cc || ca == cc);
    }
    if (kept) { flag[ca] = 1u; flag[cb] = 1u; flag[cc] = 1u; }  // (plain stores of one value)
    if (keep) {
      keep[f] = kept ? 1 : 0;
      fcell[3ull * f] = kept ? ca : 0u;
      fcell[3ull * f + 1ull] = kept ? cb : 0u;
      fcell[3ull * f + 2ull] = kept ? cc : 0u;
    }
  }
  const unsigned total = block_count(kept, s_w);
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = total;
}

// Cells in a grid-stride loop, so that a wave ends in ONE atomic per counter however many cells it saw (a counter word that every
// wave of a cell-per-lane pass adds to costs more than the pass: same-address atomics serialise). cpos: NULL in a dry run, else 3
// floats per cell, written for the flagged cells. inv_scale: 2^(e - 30).
__global__ void __launch_bounds__(BLOCK) simplify_place_kernel(const unsigned long long* __restrict__ tab_key, const unsigned* __restrict__ tab_label,
                                                               const SimplifyCell* __restrict__ acc, const unsigned* __restrict__ flag, unsigned long long cells,
                                                               const float* __restrict__ verts, double inv_scale, float* __restrict__ cpos,
                                                               SimplifyTail* __restrict__ tail) {
#pragma clang fp contract(off)
  unsigned largest = 0, n_named = 0;
  const unsigned long long step = (unsigned long long)gridDim.x * BLOCK;
  for (unsigned long long c = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; c < cells; c += step) {
    if (tab_key[c] == WELD_EMPTY_KEY) continue;
    const SimplifyCell a = acc[c];
    const unsigned n = (unsigned)a.n;  // (V < 2^32)
    largest = n > largest ? n : largest;
    if (flag[c] == 0u) continue;
    n_named++;
    if (!cpos) continue;
    if (n == 1u) {
      const unsigned v = tab_label[c];
#pragma unroll
      for (int k = 0; k < 3; k++) cpos[3ull * c + k] = verts[3ull * v + k];
    } else {
#pragma unroll
      for (int k = 0; k < 3; k++) cpos[3ull * c + k] = (float)(((double)(long long)a.s[k] / (double)n) * inv_scale);
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned o = __shfl_down(largest, off, 64);
    largest = o > largest ? o : largest;
    n_named += __shfl_down(n_named, off, 64);
  }
  if ((threadIdx.x & 63u) == 0u) {
    if (n_named) atomicAdd(&tail->named, (unsigned long long)n_named);
    if (largest) atomicMax(&tail->largest, (unsigned long long)largest);
  }
}
