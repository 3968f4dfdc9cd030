// kernels_simplify_adaptive.h -- an indexed mesh made smaller by ERROR-BOUNDED clustering over nested grids: a used vertex lies in one
// cell per level (the level-0 cell of kernels_simplify.h, shifted right by the level), a cell's position is the mean of its vertices,
// its error the largest distance from that position to the plane of a face with a corner in it, and a vertex goes to its coarsest
// ancestor whose error is within the tolerance (include/gsdf_hip.h: "indexed meshes: adaptive simplify" states the contract;
// abi_indexed.hip launches these; a numpy restatement: tests/adaptiveref.py). Independent of any SDF tree.
//
//   simplify_mark_kernel, topo_maxbits_kernel   (kernels_simplify.h, kernels_topo.h) used vertices, degenerate faces, the exponent
//   adaptive_insert_kernel   a used vertex per lane: its level-0 cell, then per level the key into the one table all levels share
//                            (table_claim) and a 32-bit minimum of the vertex number on the cell's label; vcell[l V + v] = the cell
//   adaptive_sum_kernel      a vertex per lane, per level: n += 1 and S_k += q_k on the cell's record (topo_count / topo_add: one
//                            atomic per wave where the wave is of one cell -- at the upper levels almost always)
//   adaptive_place_kernel    cells, grid-stride: every occupied cell's position by the contract
//   adaptive_error_kernel    a face per lane: its plane ONCE, then per corner and level the distance of the cell's position to it,
//                            a 64-bit unsigned maximum of the float64's bits. The cell's word is read first and the atomic is left
//                            out where the term is not larger, or the word is beyond the tolerance already (only an accepted cell
//                            needs its complete maximum); a wave of one cell reduces to one lane first
//   adaptive_choose_kernel   a vertex per lane: the coarsest level whose cell is accepted; vchoice[v] = that cell if it has more than
//                            one member, else cells + v (SINGLE). The cell's smallest member counts it: per level, largest, max_err
//   simplify_faces_kernel    (kernels_simplify.h) over vchoice: kept faces, flags of the clusters they name
//   adaptive_named_kernel    the flagged ones counted
//   topo_compact_kernel .. topo_renumber_kernel, remap_kernel   as the uniform simplifier, over cells + V cluster numbers
//
// Sums are integer sums, labels minima, errors maxima of non-negative float64 bit patterns: no order of arrival changes a bit.
#pragma once
#include "kernels_common.h"
#include "kernels_weld.h"
#include "kernels_topo.h"
#include "kernels_simplify.h"

#define ADAPTIVE_KIND 6ull       // after dual contouring's kind 5; bits 60 .. 63 = 0110: never WELD_EMPTY_KEY
#define ADAPTIVE_BIAS 131072.0   // 2^17
#define ADAPTIVE_MAX_LEVELS 16
static_assert(((ADAPTIVE_KIND << 60) | 0x0fffffffffffffffull) != WELD_EMPTY_KEY, "a cluster key cannot be the table's empty value");

// (the head record is the uniform simplifier's SimplifyHead: out_of_range counts |c_k| >= 2^17 here)
struct AdaptiveTail {
  unsigned long long kept;     // block_scan_kernel over simplify_faces_kernel's counts: the kept faces
  unsigned long long named;    // adaptive_named_kernel: clusters and singles a kept face names
  unsigned long long largest;  // adaptive_choose_kernel: the largest chosen n (1 where only singles are)
  unsigned long long singles;  // ... used vertices that stay alone
  unsigned long long max_err;  // ... bits of the largest error of a chosen cluster of more than one member
  unsigned long long chosen[ADAPTIVE_MAX_LEVELS];  // ... such clusters per level
};
struct AdaptiveCounters {
  SimplifyHead head;
  AdaptiveTail tail;
};

// the key of cell (c >> level) of level `level`
__device__ __forceinline__ unsigned long long adaptive_key(const long long* c, unsigned level) {
  unsigned long long key = (ADAPTIVE_KIND << 60) | ((unsigned long long)level << 54);
#pragma unroll
  for (int k = 0; k < 3; k++) key |= (unsigned long long)((c[k] >> level) + 131072ll) << (18 * k);  // (arithmetic shift: the grids nest)
  return key;
}

// tab_key[cells] and tab_label[cells] = 0xff.. before the pass (one memset); mask = cells - 1. vcell: levels x n_verts words.
__global__ void __launch_bounds__(BLOCK) adaptive_insert_kernel(const float* __restrict__ verts, const unsigned* __restrict__ used, unsigned long long n_verts,
                                                                double ox, double oy, double oz, double cell, unsigned levels,
                                                                unsigned long long* __restrict__ tab_key, unsigned* tab_label, unsigned mask,
                                                                unsigned* __restrict__ vcell, SimplifyHead* __restrict__ head) {
#pragma clang fp contract(off)
  unsigned my_probes = 0, my_new = 0, my_used = 0, my_nonfinite = 0, my_range = 0, my_bad = 0xffffffffu;
  bool lost = false;
  const double o[3] = {ox, oy, oz};
  const unsigned long long step = (unsigned long long)gridDim.x * BLOCK;
  for (unsigned long long v = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; v < n_verts; v += step) {
    bool place = false;
    long long c[3] = {0ll, 0ll, 0ll};
    if (used[v] != 0u) {
      my_used++;
      const float p[3] = {verts[3ull * v], verts[3ull * v + 1ull], verts[3ull * v + 2ull]};
      bool finite = true, inside = true;
#pragma unroll
      for (int k = 0; k < 3; k++) {
        finite = finite && (__float_as_uint(p[k]) & 0x7fffffffu) < 0x7f800000u;
        const double f = __builtin_floor(((double)p[k] - o[k]) / cell);
        const bool ok = __builtin_fabs(f) < ADAPTIVE_BIAS;  // (false for a NaN)
        inside = inside && ok;
        c[k] = ok ? (long long)f : 0ll;
      }
      if (!finite) {
        my_nonfinite++;
      } else if (!inside) {
        my_range++;
        my_bad = min(my_bad, (unsigned)v);
      } else {
        place = true;
      }
    }
    for (unsigned l = 0; l < levels; l++) {
      unsigned at = TOPO_NONE;
      if (place) {
        const unsigned long long h = table_claim(tab_key, mask, adaptive_key(c, l), &my_probes, &my_new);
        if (h != TABLE_NONE) {
          // (a coarse cell's label is one word for thousands of vertices: the atomic only where it can still lower it)
          if (__atomic_load_n(&tab_label[h], __ATOMIC_RELAXED) > (unsigned)v) atomicMin(&tab_label[h], (unsigned)v);
          at = (unsigned)h;
        } else {
          lost = true;
        }
      }
      vcell[(unsigned long long)l * n_verts + v] = at;
    }
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
__global__ void __launch_bounds__(BLOCK) adaptive_sum_kernel(const float* __restrict__ verts, const unsigned* __restrict__ vcell, unsigned long long n_verts,
                                                             unsigned levels, double scale, SimplifyCell* __restrict__ acc) {
#pragma clang fp contract(off)
  const unsigned long long v = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const bool in = v < n_verts && vcell[v] != TOPO_NONE;  // (a vertex has its cell at every level or at none)
  unsigned long long q[3] = {0ull, 0ull, 0ull};
  if (in) {
#pragma unroll
    for (int k = 0; k < 3; k++) q[k] = (unsigned long long)(long long)__builtin_rint((double)verts[3ull * v + k] * scale);  // |q| <= 2^30
  }
  for (unsigned l = 0; l < levels; l++) {  // (uniform: every lane of the wave shuffles)
    const unsigned at = in ? vcell[(unsigned long long)l * n_verts + v] : TOPO_NONE;
    const TopoWave w = topo_wave(at);
    topo_count(w, at, true, acc, SIMPLIFY_F_N);
#pragma unroll
    for (int k = 0; k < 3; k++) topo_add(w, at, q[k], acc, SIMPLIFY_F_SUM + k);
  }
}

// cpos: 3 floats per cell, written for every occupied cell. inv_scale: 2^(e - 30).
__global__ void __launch_bounds__(BLOCK) adaptive_place_kernel(const unsigned long long* __restrict__ tab_key, const unsigned* __restrict__ tab_label,
                                                               const SimplifyCell* __restrict__ acc, unsigned long long cells, const float* __restrict__ verts,
                                                               double inv_scale, float* __restrict__ cpos) {
#pragma clang fp contract(off)
  const unsigned long long step = (unsigned long long)gridDim.x * BLOCK;
  for (unsigned long long c = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; c < cells; c += step) {
    if (tab_key[c] == WELD_EMPTY_KEY) continue;
    const SimplifyCell a = acc[c];
    const unsigned n = (unsigned)a.n;  // (V < 2^32)
    if (n == 1u) {
      const unsigned v = tab_label[c];
#pragma unroll
      for (int k = 0; k < 3; k++) cpos[3ull * c + k] = verts[3ull * v + k];
    } else {
#pragma unroll
      for (int k = 0; k < 3; k++) cpos[3ull * c + k] = (float)(((double)(long long)a.s[k] / (double)n) * inv_scale);
    }
  }
}

// err[cells] = 0 before the pass (the bits of +0.0). tol: the option as float64.
__global__ void __launch_bounds__(BLOCK) adaptive_error_kernel(const float* __restrict__ verts, const unsigned* __restrict__ idx, unsigned long long n_tris,
                                                               const unsigned* __restrict__ vcell, unsigned long long n_verts, unsigned levels,
                                                               const float* __restrict__ cpos, unsigned long long* err, double tol) {
#pragma clang fp contract(off)
  const unsigned long long f = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  bool plane = false;
  unsigned vtx[3] = {0u, 0u, 0u};
  double pa[3] = {0, 0, 0}, n[3] = {0, 0, 0}, L = 0;
  if (f < n_tris) {
#pragma unroll
    for (int c = 0; c < 3; c++) vtx[c] = idx[3ull * f + c];
    if (!(vtx[0] == vtx[1] || vtx[1] == vtx[2] || vtx[0] == vtx[2])) {
      double u[3], w[3];
#pragma unroll
      for (int k = 0; k < 3; k++) {
        pa[k] = (double)verts[3ull * vtx[0] + k];
        u[k] = (double)verts[3ull * vtx[1] + k] - pa[k];
        w[k] = (double)verts[3ull * vtx[2] + k] - pa[k];
      }
      n[0] = u[1] * w[2] - u[2] * w[1];
      n[1] = u[2] * w[0] - u[0] * w[2];
      n[2] = u[0] * w[1] - u[1] * w[0];
      L = __builtin_sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]);
      plane = L > 0.0;  // (false for a NaN: a face of non-finite vertices; the host has refused the mesh by then)
    }
  }
  for (unsigned c = 0; c < 3u; c++) {
    for (unsigned l = 0; l < levels; l++) {  // (uniform: every lane of the wave shuffles)
      unsigned at = plane ? vcell[(unsigned long long)l * n_verts + vtx[c]] : TOPO_NONE;
      unsigned long long bits = 0ull;
      if (at != TOPO_NONE) {
        const double cur = __longlong_as_double((long long)__atomic_load_n(&err[at], __ATOMIC_RELAXED));
        if (cur > tol) {
          at = TOPO_NONE;  // not accepted whatever this term is
        } else {
          double g[3];
#pragma unroll
          for (int k = 0; k < 3; k++) g[k] = (double)cpos[3ull * at + k] - pa[k];
          const double t = __builtin_fabs((n[0] * g[0] + n[1] * g[1]) + n[2] * g[2]) / L;
          bits = (unsigned long long)__double_as_longlong(t);
          if (!(t > cur)) at = TOPO_NONE;
        }
      }
      const TopoWave w = topo_wave(at);
      if (w.s0 == TOPO_NONE) continue;
      if (w.uniform) {
        if (at == TOPO_NONE) bits = 0ull;
        unsigned lo = (unsigned)bits, hi = (unsigned)(bits >> 32);
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
          const unsigned l2 = __shfl_down(lo, off, 64), h2 = __shfl_down(hi, off, 64);
          const unsigned long long mine = (((unsigned long long)hi) << 32) | lo, other = (((unsigned long long)h2) << 32) | l2;
          const unsigned long long m = other > mine ? other : mine;
          lo = (unsigned)m;
          hi = (unsigned)(m >> 32);
        }
        if ((threadIdx.x & 63u) == 0u) atomicMax(&err[w.s0], (((unsigned long long)hi) << 32) | lo);
      } else if (at != TOPO_NONE) {
        atomicMax(&err[at], bits);
      }
    }
  }
}

// vchoice[v]: the cell of v's cluster, cells + v for a SINGLE vertex, TOPO_NONE for an unused one. tail: zero before the pass.
__global__ void __launch_bounds__(BLOCK) adaptive_choose_kernel(const unsigned* __restrict__ vcell, unsigned long long n_verts, unsigned levels,
                                                                const unsigned* __restrict__ tab_label, const SimplifyCell* __restrict__ acc,
                                                                const unsigned long long* __restrict__ err, double tol, unsigned cells,
                                                                unsigned* __restrict__ vchoice, AdaptiveTail* __restrict__ tail) {
  __shared__ unsigned s_chosen[ADAPTIVE_MAX_LEVELS], s_singles, s_largest;
  __shared__ unsigned long long s_err;
  if (threadIdx.x < ADAPTIVE_MAX_LEVELS) s_chosen[threadIdx.x] = 0u;
  if (threadIdx.x == 0) { s_singles = 0u; s_largest = 0u; s_err = 0ull; }
  __syncthreads();
  const unsigned long long v = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  if (v < n_verts) {
    unsigned choice = TOPO_NONE;
    if (vcell[v] != TOPO_NONE) {
      choice = cells + (unsigned)v;
      for (int l = (int)levels - 1; l >= 0; l--) {
        const unsigned c = vcell[(unsigned long long)l * n_verts + v];
        const unsigned long long e = err[c];
        if (!(__longlong_as_double((long long)e) <= tol)) continue;
        const unsigned n = (unsigned)acc[c].n;
        if (n > 1u) {
          choice = c;
          if (tab_label[c] == (unsigned)v) {  // the cluster's smallest member speaks for it
            atomicAdd(&s_chosen[l], 1u);
            atomicMax(&s_largest, n);
            atomicMax(&s_err, e);
          }
        }
        break;
      }
      if (choice >= cells) { atomicAdd(&s_singles, 1u); atomicMax(&s_largest, 1u); }
    }
    vchoice[v] = choice;
  }
  __syncthreads();
  if (threadIdx.x < ADAPTIVE_MAX_LEVELS && s_chosen[threadIdx.x]) atomicAdd(&tail->chosen[threadIdx.x], (unsigned long long)s_chosen[threadIdx.x]);
  if (threadIdx.x == 0) {
    if (s_singles) atomicAdd(&tail->singles, (unsigned long long)s_singles);
    if (s_largest) atomicMax(&tail->largest, (unsigned long long)s_largest);
    if (s_err) atomicMax(&tail->max_err, s_err);
  }
}

// flag[n]: simplify_faces_kernel's, over cells + V cluster numbers
__global__ void __launch_bounds__(BLOCK) adaptive_named_kernel(const unsigned* __restrict__ flag, unsigned long long n, AdaptiveTail* __restrict__ tail) {
  unsigned n_named = 0;
  const unsigned long long step = (unsigned long long)gridDim.x * BLOCK;
  for (unsigned long long c = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; c < n; c += step) n_named += flag[c] != 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n_named += __shfl_down(n_named, off, 64);
  if ((threadIdx.x & 63u) == 0u && n_named) atomicAdd(&tail->named, (unsigned long long)n_named);
}
