// kernels_clean.h -- an indexed mesh cleaned: vertices with equal positions merged, degenerate faces dropped, and of the faces over
// one set of three vertices at most one kept (include/gsdf_hip.h: "indexed meshes: clean" states the contract; abi_indexed.hip launches
// these; a numpy restatement: tests/cleanref.py). Integers only: no kernel here does a float operation. Independent of any SDF tree:
// these kernels live in the shipped code object only.
//
// Both groupings are by a 96-bit key (three position words / three sorted vertex numbers), which no single compare-and-swap can
// claim. So a table cell holds a 32-bit REPRESENTATIVE instead -- a vertex number or a face number, 0xffffffff = empty -- and the
// key of a cell is read from its representative in the immutable input (clean_claim). Any member of a class is a valid
// representative, so a reader stays correct while the cell's atomicMin settles on the smallest.
//
//   clean_vert_insert_kernel  a vertex per lane: its key into the vertex table; vcls[v] = the cell (none for a non-finite vertex)
//   clean_vert_class_kernel   once the table is settled: vcls[v] = the cell's minimum = the class's smallest vertex; merged counted
//   remap_kernel              (kernels_weld.h) a copy of the faces with every index replaced by its class
//   clean_face_insert_kernel  a face per lane: its set into the face table; per cell and orientation an integer count and the
//                             smallest face number; fcell[f] = the cell. A wave whose faces are all of one set sends one lane.
//   clean_decide_kernel       a face per lane: degenerate / kept by the rule; the classes of a kept face flagged; the set's smallest
//                             face adds the set's figures to the stats; kept faces counted per block of 256
//   clean_named_kernel        the flagged classes counted (n_verts, also of a dry run)
//   topo_compact_kernel .. topo_renumber_kernel, remap_kernel   (kernels_topo.h, kernels_weld.h) extract's kernels, as they are
//
// Every count is an integer sum and every representative a minimum, so neither the order in which threads arrive nor the cell a key
// happens to land in changes a bit of the result.
#pragma once
#include "kernels_common.h"
#include "kernels_weld.h"
#include "kernels_topo.h"

#define CLEAN_NONE 0xffffffffu  // an empty cell / no cell (a vertex number is below 2^32 - 1, a face number below 2^32 / 3)

// What the host reads: each table's counters are cleared for every attempt of that table (table_build), the rest once.
struct CleanCounters {
  TableCounters vtab;
  TableCounters ftab;
  unsigned long long merged;          // clean_vert_class_kernel
  unsigned long long degenerate;      // clean_decide_kernel, as the five below
  unsigned long long face_sets;
  unsigned long long cancelled_sets;
  unsigned long long duplicate;
  unsigned long long opposite;
  unsigned long long largest;
  unsigned long long named;           // clean_named_kernel
  unsigned long long kept;            // block_scan_kernel over clean_decide_kernel's counts
};

__device__ __forceinline__ unsigned clean_hash(unsigned x, unsigned y, unsigned z) {
  return weld_hash(((((unsigned long long)x) << 32) | y) ^ ((unsigned long long)z * 0x9e3779b97f4a7c15ull));
}

// The cell of the key (x, y, z) in tab[mask + 1] (every cell CLEAN_NONE before the pass), `me` being a member of the key's class:
// an empty cell is claimed with me by a 32-bit compare-and-swap (*is_new += 1 then); an occupied cell is the key's iff its
// representative's key, key_of(representative, &x, &y, &z), equals it, and then the cell becomes min(cell, me). Linear probing,
// *probes += the cells inspected. CLEAN_NONE after WELD_MAX_PROBES cells: the host grows the table and runs the pass again.
template <typename KeyOf>
__device__ __forceinline__ unsigned clean_claim(unsigned* tab, unsigned mask, unsigned x, unsigned y, unsigned z, unsigned me, const KeyOf& key_of,
                                                unsigned* probes, unsigned* is_new) {
  unsigned h = clean_hash(x, y, z) & mask;
  for (unsigned n = 0; n < WELD_MAX_PROBES && n <= mask; n++) {
    (*probes)++;
    unsigned seen = topo_load(&tab[h]);
    if (seen == CLEAN_NONE) {
      seen = atomicCAS(&tab[h], CLEAN_NONE, me);
      if (seen == CLEAN_NONE) { (*is_new)++; return h; }
    }
    unsigned kx, ky, kz;
    key_of(seen, &kx, &ky, &kz);
    if (kx == x && ky == y && kz == z) {
      if (me < seen) atomicMin(&tab[h], me);  // (the cell only ever falls: nothing to do for a larger number)
      return h;
    }
    h = (h + 1u) & mask;
  }
  return CLEAN_NONE;
}

// ---- merge -------------------------------------------------------------------------------------------------------------------------
// a coordinate's word of the position key: its bits, -0 as +0
__device__ __forceinline__ unsigned clean_word(unsigned bits) { return bits == 0x80000000u ? 0u : bits; }
__device__ __forceinline__ bool clean_finite(unsigned x, unsigned y, unsigned z) {
  return (x & 0x7fffffffu) < 0x7f800000u && (y & 0x7fffffffu) < 0x7f800000u && (z & 0x7fffffffu) < 0x7f800000u;
}

// verts: the positions as their bits. tab[cells] = 0xff.. before the pass; mask = cells - 1.
__global__ void __launch_bounds__(BLOCK) clean_vert_insert_kernel(const unsigned* __restrict__ verts, unsigned long long n_verts, unsigned* tab, unsigned mask,
                                                                  unsigned* __restrict__ vcls, TableCounters* __restrict__ ctr) {
  unsigned my_probes = 0, my_new = 0;
  bool lost = false;
  const auto key_of = [verts](unsigned v, unsigned* x, unsigned* y, unsigned* z) {
    *x = clean_word(verts[3ull * v]); *y = clean_word(verts[3ull * v + 1ull]); *z = clean_word(verts[3ull * v + 2ull]);
  };
  const unsigned long long step = (unsigned long long)gridDim.x * BLOCK;
  for (unsigned long long v = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; v < n_verts; v += step) {
    unsigned x, y, z, at = CLEAN_NONE;
    key_of((unsigned)v, &x, &y, &z);
    if (clean_finite(x, y, z)) {
      at = clean_claim(tab, mask, x, y, z, (unsigned)v, key_of, &my_probes, &my_new);
      lost = lost || at == CLEAN_NONE;
    }
    vcls[v] = at;
  }
  table_stats(my_probes, my_new, lost, ctr);
}

// vcls[v]: the cell -> the class (the cell's settled minimum; v itself for a non-finite vertex). Grid-stride: one atomic per wave.
__global__ void __launch_bounds__(BLOCK) clean_vert_class_kernel(const unsigned* __restrict__ tab, unsigned long long n_verts, unsigned* __restrict__ vcls,
                                                                 CleanCounters* __restrict__ ctr) {
  unsigned merged = 0;
  const unsigned long long step = (unsigned long long)gridDim.x * BLOCK;
  for (unsigned long long v = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; v < n_verts; v += step) {
    const unsigned at = vcls[v];
    const unsigned c = at == CLEAN_NONE ? (unsigned)v : tab[at];
    vcls[v] = c;
    merged += c != (unsigned)v ? 1u : 0u;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) merged += __shfl_down(merged, off, 64);
  if ((threadIdx.x & 63u) == 0u && merged) atomicAdd(&ctr->merged, (unsigned long long)merged);
}

// ---- face sets -----------------------------------------------------------------------------------------------------------------------
// Face f of idx: false if degenerate; else its set lo < mid < hi, and *minus = it is a rotation of (lo, hi, mid).
__device__ __forceinline__ bool clean_face_key(const unsigned* __restrict__ idx, unsigned long long f, unsigned* lo, unsigned* mid, unsigned* hi, unsigned* minus) {
  const unsigned a = idx[3ull * f], b = idx[3ull * f + 1ull], c = idx[3ull * f + 2ull];
  if (a == b || b == c || a == c) return false;
  *lo = min(a, min(b, c));
  *hi = max(a, max(b, c));
  *mid = a ^ b ^ c ^ *lo ^ *hi;
  const unsigned next = a == *lo ? b : (b == *lo ? c : a);  // the corner that follows lo
  *minus = next != *mid ? 1u : 0u;
  return true;
}

// idx: the faces after the merge (immutable in this pass). tab[cells] and fmin[2 cells] = 0xff.., cnt[2 cells] = 0 before the pass;
// mask = cells - 1. cnt[2 h + o] / fmin[2 h + o]: the faces of cell h's set with orientation o (0: +, 1: -) / the smallest of them.
// fcell[f] = the cell (CLEAN_NONE for a degenerate face). Where all non-degenerate faces of a wave are of ONE set -- the copies of
// a folded sheet, the soup of a welded mesh -- its first such lane claims the cell and adds the wave's counts: one atomic per wave
// and word, not one per lane.
__global__ void __launch_bounds__(BLOCK) clean_face_insert_kernel(const unsigned* __restrict__ idx, unsigned long long n_tris, unsigned* tab,
                                                                  unsigned* __restrict__ fmin, unsigned* __restrict__ cnt, unsigned mask,
                                                                  unsigned* __restrict__ fcell, TableCounters* __restrict__ ctr) {
  const unsigned long long f = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const unsigned lane = threadIdx.x & 63u;
  unsigned my_probes = 0, my_new = 0, lo = 0, mid = 0, hi = 0, minus = 0, at = CLEAN_NONE;
  const bool valid = f < n_tris && clean_face_key(idx, f, &lo, &mid, &hi, &minus);
  const auto key_of = [idx](unsigned g, unsigned* x, unsigned* y, unsigned* z) {
    unsigned m;
    (void)clean_face_key(idx, g, x, y, z, &m);  // (a representative is never degenerate)
  };
  const unsigned long long m = __ballot(valid);
  if (m != 0ull) {  // wave-uniform
    const int leader = __builtin_ctzll(m);
    const unsigned l0 = (unsigned)__shfl((int)lo, leader, 64), m0 = (unsigned)__shfl((int)mid, leader, 64), h0 = (unsigned)__shfl((int)hi, leader, 64);
    const bool one_set = __ballot(valid && (lo != l0 || mid != m0 || hi != h0)) == 0ull;
    const unsigned long long mp = __ballot(valid && minus == 0u), mm = m & ~mp;
    if (one_set) {
      if ((int)lane == leader) {
        at = clean_claim(tab, mask, lo, mid, hi, (unsigned)f, key_of, &my_probes, &my_new);
        if (at != CLEAN_NONE) {
          const unsigned f0 = (unsigned)f - lane;  // lane 0's face
          if (mp) {
            atomicAdd(&cnt[2ull * at], (unsigned)__builtin_popcountll(mp));
            atomicMin(&fmin[2ull * at], f0 + (unsigned)__builtin_ctzll(mp));
          }
          if (mm) {
            atomicAdd(&cnt[2ull * at + 1ull], (unsigned)__builtin_popcountll(mm));
            atomicMin(&fmin[2ull * at + 1ull], f0 + (unsigned)__builtin_ctzll(mm));
          }
        }
      }
      at = (unsigned)__shfl((int)at, leader, 64);
      if (!valid) at = CLEAN_NONE;
    } else if (valid) {
      at = clean_claim(tab, mask, lo, mid, hi, (unsigned)f, key_of, &my_probes, &my_new);
      if (at != CLEAN_NONE) {
        atomicAdd(&cnt[2ull * at + minus], 1u);
        atomicMin(&fmin[2ull * at + minus], (unsigned)f);
      }
    }
  }
  if (f < n_tris) fcell[f] = at;
  table_stats(my_probes, my_new, valid && at == CLEAN_NONE, ctr);
}

// The rule. fcell: NULL without GSDF_CLEAN_FACES (every non-degenerate face is kept, tab / fmin / cnt are not read). named[V] = 0
// before the pass: the classes a kept face names get 1 (plain stores of one value). keep: NULL in a dry run. blk_cnt[b] = kept faces
// among [256 b, 256 b + 256). The figures of a set are added by ONE of its faces, its smallest (the table's settled representative).
__global__ void __launch_bounds__(BLOCK) clean_decide_kernel(const unsigned* __restrict__ idx, unsigned long long n_tris, const unsigned* __restrict__ tab,
                                                             const unsigned* __restrict__ fmin, const unsigned* __restrict__ cnt,
                                                             const unsigned* __restrict__ fcell, unsigned* __restrict__ named,
                                                             unsigned char* __restrict__ keep, unsigned* __restrict__ blk_cnt, CleanCounters* __restrict__ ctr) {
  __shared__ unsigned s_w[4];
  const unsigned long long f = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  bool deg = false, kept = false;
  unsigned sets = 0, cancelled = 0, dup = 0, opp = 0, largest = 0;
  if (f < n_tris) {
    unsigned lo, mid, hi, minus;
    deg = !clean_face_key(idx, f, &lo, &mid, &hi, &minus);
    if (!deg) {
      if (!fcell) {
        kept = true;
      } else {
        const unsigned at = fcell[f];  // (never CLEAN_NONE: the pass that left a face out was repeated)
        const unsigned nf = cnt[2ull * at], nr = cnt[2ull * at + 1ull];
        kept = nf != nr && minus == (nr > nf ? 1u : 0u) && fmin[2ull * at + minus] == (unsigned)f;
        if (tab[at] == (unsigned)f) {
          const unsigned less = min(nf, nr), more = max(nf, nr);
          sets = 1u;
          cancelled = nf == nr ? 1u : 0u;
          largest = nf + nr;
          opp = 2u * less;
          dup = nf == nr ? 0u : more - less - 1u;
        }
      }
      if (kept) { named[lo] = 1u; named[mid] = 1u; named[hi] = 1u; }
    }
    if (keep) keep[f] = kept ? 1 : 0;
  }
  const unsigned total = block_count(kept, s_w);
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = total;
  const unsigned n_deg = (unsigned)__builtin_popcountll(__ballot(deg));
  if (__ballot(sets != 0u) != 0ull) {  // (the sets' faces are disjoint: the sums stay below the number of faces, below 2^32)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      sets += __shfl_down(sets, off, 64);
      cancelled += __shfl_down(cancelled, off, 64);
      dup += __shfl_down(dup, off, 64);
      opp += __shfl_down(opp, off, 64);
      const unsigned o = __shfl_down(largest, off, 64);
      largest = o > largest ? o : largest;
    }
  }
  if ((threadIdx.x & 63u) == 0u) {
    if (n_deg) atomicAdd(&ctr->degenerate, (unsigned long long)n_deg);
    if (sets) atomicAdd(&ctr->face_sets, (unsigned long long)sets);
    if (cancelled) atomicAdd(&ctr->cancelled_sets, (unsigned long long)cancelled);
    if (dup) atomicAdd(&ctr->duplicate, (unsigned long long)dup);
    if (opp) atomicAdd(&ctr->opposite, (unsigned long long)opp);
    if ((unsigned long long)largest > __atomic_load_n(&ctr->largest, __ATOMIC_RELAXED)) atomicMax(&ctr->largest, (unsigned long long)largest);  // (only where it can still raise it)
  }
}

__global__ void __launch_bounds__(BLOCK) clean_named_kernel(const unsigned* __restrict__ named, unsigned long long n_verts, CleanCounters* __restrict__ ctr) {
  unsigned n = 0;
  const unsigned long long step = (unsigned long long)gridDim.x * BLOCK;
  for (unsigned long long v = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; v < n_verts; v += step) n += named[v] != 0u ? 1u : 0u;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) n += __shfl_down(n, off, 64);
  if ((threadIdx.x & 63u) == 0u && n) atomicAdd(&ctr->named, (unsigned long long)n);
}
