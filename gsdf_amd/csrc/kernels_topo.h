// kernels_topo.h -- what an indexed mesh is, topologically and in measure: edge classes, shells, area / volume / moments, and the
// extraction of shells into a new mesh (include/gsdf_hip.h: "indexed meshes: report and extract" states the contract; abi_indexed.hip
// launches these). Independent of any SDF tree: these kernels live in the shipped code object only.
//
//   topo_maxbits_kernel      integer max over the finite coordinates' |bits|: the exponent e of the contract
//   topo_edge_insert_kernel  a face per lane -> its three unordered pairs into the open-addressing table (kernels_weld.h:
//                            table_claim) and +1 on the pair's forward or reverse counter
//   topo_union_kernel        a face per lane -> union (a, b), (b, c): lock-free union-find, every write an atomicMin, so that
//                            parent[x] <= x always and a component's root is its smallest vertex whatever the order of arrival
//   topo_root_kernel         vertex -> root (read-only chase); roots of used vertices counted per block of 256
//   block_scan_kernel        (kernels_weld.h) the carry across blocks
//   topo_number_kernel       block_rank + the block's carry: root -> shell number, in increasing order of the root
//   topo_vertex_shell_kernel vertex -> shell number; the shells' vertex counts
//   topo_measure_kernel      a face per lane: shell of the face, the contract's float64 terms quantised to integers, summed as integers
//   topo_classify_kernel     a CELL per lane: the pair's class, counted on its shell (the shell of its smaller vertex)
//   topo_keep_kernel .. topo_renumber_kernel, remap_kernel   extract: kept faces compacted in order, vertices renumbered by their smallest kept slot
//   cube_first_kernel, cube_number_kernel                     dual contouring's indexed mesh: extract's owner / number steps over kept cubes
//
// Sums. A wave whose lanes all belong to one shell (the common case: a shell's faces are runs in mesher order) reduces across the
// wave and issues ONE atomic per quantity; a mixed wave issues per-lane atomics on each lane's shell. Every quantity is an integer
// (counts; terms split into a low 32-bit and a high signed part, each summed in a 64-bit word that 2^31 terms cannot overflow), so
// neither path nor order changes a bit of the result.
#pragma once
#include "kernels_common.h"
#include "kernels_weld.h"

#define TOPO_NONE 0xffffffffu
#define TOPO_BB_MIN_INIT 0xff800000u  // order-preserving bits of +inf
#define TOPO_BB_MAX_INIT 0x007fffffu  // ... of -inf

struct TopoCounters {
  TableCounters tab;              // topo_edge_insert_kernel: the pairs' table (the host reads this head as it reads the weld's)
  unsigned long long degenerate;  // faces with two equal indices
  unsigned long long used_verts;  // topo_root_kernel
  unsigned long long n_shells;    // block_scan_kernel over topo_root_kernel's counts
  unsigned long long maxbits;     // topo_maxbits_kernel
};

// One record per shell; the host adds the shells up for the mesh's totals (integers: exact).
struct TopoShellAcc {
  unsigned long long n_verts, n_tris, nonfinite, edges, boundary, nonmanifold, misoriented;
  unsigned long long sum[10];  // area, volume, moment x / y / z: low 32 bits summed, then the (signed) rest summed
  unsigned bb[6];              // order-preserving bits: min x y z, max x y z
  unsigned label, pad;
};
#define TOPO_F_NVERTS 0
#define TOPO_F_NTRIS 1
#define TOPO_F_NONFINITE 2
#define TOPO_F_EDGES 3
#define TOPO_F_BOUNDARY 4
#define TOPO_F_NONMANIFOLD 5
#define TOPO_F_MISORIENTED 6
#define TOPO_F_SUM 7
#define TOPO_BB_WORD 34  // index of bb[0] in 32-bit words

// a float's bits, monotone in its value (-0 below +0)
__device__ __forceinline__ unsigned topo_ordered(unsigned bits) { return bits ^ ((bits >> 31) ? 0xffffffffu : 0x80000000u); }

// The lanes' shells of one wave: s0 = the first lane's that has one (TOPO_NONE: no lane has), uniform = every lane that has one has s0.
struct TopoWave {
  unsigned s0;
  bool uniform;
};
__device__ __forceinline__ TopoWave topo_wave(unsigned shell) {
  TopoWave w;
  const unsigned long long m = __ballot(shell != TOPO_NONE);
  w.s0 = TOPO_NONE;
  w.uniform = true;
  if (m != 0ull) {
    w.s0 = (unsigned)__shfl((int)shell, __builtin_ctzll(m), 64);
    w.uniform = __ballot(shell != TOPO_NONE && shell != w.s0) == 0ull;
  }
  return w;
}
// Every lane of the wave calls these (they shuffle). Acc: a record of 64-bit words (TopoShellAcc; kernels_simplify.h: SimplifyCell, with the
// table's cell where the report has the shell), `field` the word's index in it.
template <typename Acc>
__device__ __forceinline__ void topo_count(const TopoWave& w, unsigned shell, bool flag, Acc* acc, unsigned field) {
  if (w.s0 == TOPO_NONE) return;
  flag = flag && shell != TOPO_NONE;
  if (w.uniform) {
    const unsigned n = (unsigned)__builtin_popcountll(__ballot(flag));
    if ((threadIdx.x & 63u) == 0u && n) atomicAdd((unsigned long long*)&acc[w.s0] + field, (unsigned long long)n);
  } else if (flag) {
    atomicAdd((unsigned long long*)&acc[shell] + field, 1ull);
  }
}
template <typename Acc>
__device__ __forceinline__ void topo_add(const TopoWave& w, unsigned shell, unsigned long long v, Acc* acc, unsigned field) {
  if (w.s0 == TOPO_NONE) return;
  if (shell == TOPO_NONE) v = 0ull;
  if (w.uniform) {
    unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned l2 = __shfl_down(lo, off, 64), h2 = __shfl_down(hi, off, 64);
      const unsigned long long t = ((((unsigned long long)hi) << 32) | lo) + ((((unsigned long long)h2) << 32) | l2);  // (mod 2^64: two's complement)
      lo = (unsigned)t;
      hi = (unsigned)(t >> 32);
    }
    const unsigned long long t = (((unsigned long long)hi) << 32) | lo;
    if ((threadIdx.x & 63u) == 0u && t) atomicAdd((unsigned long long*)&acc[w.s0] + field, t);
  } else if (v) {
    atomicAdd((unsigned long long*)&acc[shell] + field, v);
  }
}
// is_max: atomicMax, else atomicMin; v = the neutral element where the lane has nothing to say
__device__ __forceinline__ void topo_minmax(const TopoWave& w, unsigned shell, unsigned v, bool is_max, TopoShellAcc* acc, unsigned word) {
  if (w.s0 == TOPO_NONE) return;
  const unsigned neutral = is_max ? 0u : 0xffffffffu;
  if (shell == TOPO_NONE) v = neutral;
  if (w.uniform) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const unsigned o = __shfl_down(v, off, 64);
      v = is_max ? (o > v ? o : v) : (o < v ? o : v);
    }
    if ((threadIdx.x & 63u) == 0u && v != neutral) {
      if (is_max) atomicMax((unsigned*)&acc[w.s0] + word, v);
      else atomicMin((unsigned*)&acc[w.s0] + word, v);
    }
  } else if (v != neutral) {
    if (is_max) atomicMax((unsigned*)&acc[shell] + word, v);
    else atomicMin((unsigned*)&acc[shell] + word, v);
  }
}

// ---- the exponent ----------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(BLOCK) topo_maxbits_kernel(const float* __restrict__ verts, unsigned long long n, unsigned long long* __restrict__ maxbits) {
  unsigned m = 0;
  const unsigned long long step = (unsigned long long)gridDim.x * BLOCK;
  for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += step) {
    const unsigned a = __float_as_uint(verts[i]) & 0x7fffffffu;
    if (a < 0x7f800000u && a > m) m = a;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    const unsigned o = __shfl_down(m, off, 64);
    m = o > m ? o : m;
  }
  if ((threadIdx.x & 63u) == 0u && m) atomicMax(maxbits, (unsigned long long)m);
}

// ---- the edge table ----------------------------------------------------------------------------------------------------------------
// tab_key[cells] = WELD_EMPTY_KEY (memset 0xff), tab_cnt[2 cells] = 0 before the pass; mask = cells - 1. A pair {a, b}, a < b, has the
// key a << 32 | b (never the empty key: a < b); tab_cnt[2 h] counts its uses as (a, b), tab_cnt[2 h + 1] as (b, a).
__global__ void __launch_bounds__(BLOCK) topo_edge_insert_kernel(const unsigned* __restrict__ idx, unsigned long long n_tris,
                                                                 unsigned long long* __restrict__ tab_key, unsigned* __restrict__ tab_cnt, unsigned mask,
                                                                 TopoCounters* __restrict__ ctr) {
  const unsigned long long f = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  unsigned my_probes = 0, my_new = 0;
  bool lost = false, deg = false;
  if (f < n_tris) {
    const unsigned v[3] = {idx[3ull * f], idx[3ull * f + 1ull], idx[3ull * f + 2ull]};
    deg = v[0] == v[1] || v[1] == v[2] || v[0] == v[2];
    if (!deg) {
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const unsigned p = v[j], q = v[j == 2 ? 0 : j + 1];
        const bool fwd = p < q;
        const unsigned long long key = fwd ? (((unsigned long long)p << 32) | q) : (((unsigned long long)q << 32) | p);
        const unsigned long long cell = table_claim(tab_key, mask, key, &my_probes, &my_new);
        if (cell != TABLE_NONE) atomicAdd(&tab_cnt[2ull * cell + (fwd ? 0u : 1u)], 1u);
        else lost = true;
      }
    }
  }
  table_stats(my_probes, my_new, lost, &ctr->tab);
  const unsigned n_deg = (unsigned)__builtin_popcountll(__ballot(deg));
  if ((threadIdx.x & 63u) == 0u && n_deg) atomicAdd(&ctr->degenerate, (unsigned long long)n_deg);
}

// ---- shells ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned topo_load(const unsigned* p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

// The root of x's tree, halving the path on the way. Every write is an atomicMin with an ancestor: parent[] only ever decreases.
__device__ __forceinline__ unsigned topo_find(unsigned* parent, unsigned x) {
  for (;;) {
    const unsigned p = topo_load(parent + x);
    if (p == x) return x;
    const unsigned gp = topo_load(parent + p);
    if (gp == p) return p;
    atomicMin(parent + x, gp);
    x = gp;
  }
}
// Hooks the larger root under the smaller. If the larger one stopped being a root meanwhile, the atomicMin may have replaced its link
// to `old` by a link to b: (old, b) is united next, which restores what the lost link said. Ends: a strictly decreases.
__device__ __forceinline__ void topo_union(unsigned* parent, unsigned a, unsigned b) {
  for (;;) {
    a = topo_find(parent, a);
    b = topo_find(parent, b);
    if (a == b) return;
    if (a < b) { const unsigned t = a; a = b; b = t; }
    const unsigned old = atomicMin(parent + a, b);
    if (old == a) return;
    a = old;
  }
}

__global__ void __launch_bounds__(BLOCK) topo_parent_init_kernel(unsigned* __restrict__ parent, unsigned* __restrict__ used, unsigned long long n_verts) {
  const unsigned long long v = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  if (v < n_verts) { parent[v] = (unsigned)v; used[v] = 0u; }
}

__global__ void __launch_bounds__(BLOCK) topo_union_kernel(const unsigned* __restrict__ idx, unsigned long long n_tris, unsigned* parent, unsigned* used) {
  const unsigned long long f = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  if (f >= n_tris) return;
  const unsigned a = idx[3ull * f], b = idx[3ull * f + 1ull], c = idx[3ull * f + 2ull];
  if (a == b || b == c || a == c) return;
  used[a] = 1u; used[b] = 1u; used[c] = 1u;  // (plain stores of one value)
  topo_union(parent, a, b);
  topo_union(parent, b, c);
}

// root_of[v]; blk_cnt[b] = used vertices that are their own root among [256 b, 256 b + 256)
__global__ void __launch_bounds__(BLOCK) topo_root_kernel(const unsigned* __restrict__ parent, const unsigned* __restrict__ used, unsigned long long n_verts,
                                                          unsigned* __restrict__ root_of, unsigned* __restrict__ blk_cnt, TopoCounters* __restrict__ ctr) {
  __shared__ unsigned s_w[4];
  const unsigned long long v = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  bool is_root = false, is_used = false;
  if (v < n_verts) {
    unsigned x = (unsigned)v;
    for (;;) {
      const unsigned p = parent[x];
      if (p == x) break;
      x = p;
    }
    root_of[v] = x;
    is_used = used[v] != 0u;
    is_root = is_used && x == (unsigned)v;
  }
  const unsigned n_used = (unsigned)__builtin_popcountll(__ballot(is_used));
  if ((threadIdx.x & 63u) == 0u && n_used) atomicAdd(&ctr->used_verts, (unsigned long long)n_used);
  const unsigned total = block_count(is_root, s_w);
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = total;
}

// shell_num[root] = its number; the shell's record gets its label and its empty box (acc was zeroed)
__global__ void __launch_bounds__(BLOCK) topo_number_kernel(const unsigned* __restrict__ root_of, const unsigned* __restrict__ used, unsigned long long n_verts,
                                                            const unsigned* __restrict__ blk_base, unsigned* __restrict__ shell_num, TopoShellAcc* __restrict__ acc) {
  __shared__ unsigned s_w[4];
  const unsigned long long v = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const bool is_root = v < n_verts && used[v] != 0u && root_of[v] == (unsigned)v;
  const unsigned rank = block_rank(is_root, s_w);
  if (is_root) {
    const unsigned s = blk_base[blockIdx.x] + rank;
    shell_num[v] = s;
    acc[s].label = (unsigned)v;
    acc[s].bb[0] = acc[s].bb[1] = acc[s].bb[2] = TOPO_BB_MIN_INIT;
    acc[s].bb[3] = acc[s].bb[4] = acc[s].bb[5] = TOPO_BB_MAX_INIT;
  }
}

__global__ void __launch_bounds__(BLOCK) topo_vertex_shell_kernel(const unsigned* __restrict__ root_of, const unsigned* __restrict__ used, unsigned long long n_verts,
                                                                  const unsigned* __restrict__ shell_num, unsigned* __restrict__ shell_of_vertex,
                                                                  TopoShellAcc* __restrict__ acc) {
  const unsigned long long v = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  unsigned shell = TOPO_NONE;
  if (v < n_verts) {
    if (used[v] != 0u) shell = shell_num[root_of[v]];
    shell_of_vertex[v] = shell;
  }
  const TopoWave w = topo_wave(shell);
  topo_count(w, shell, true, acc, TOPO_F_NVERTS);
}

// ---- measures ----------------------------------------------------------------------------------------------------------------------
// The contract's terms (gsdf_hip.h), float64, no contraction (the library is built with -ffp-contract=off; the pragma says it again).
// sc_area / sc_vol / sc_mom: the powers of two 2^(59 - 2 e), 2^(62 - 3 e), 2^(62 - 4 e).
__device__ __forceinline__ void topo_split(double term, double scale, unsigned long long* lo, unsigned long long* hi) {
  const long long q = (long long)__builtin_rint(term * scale);  // |q| <= 2^62
  *lo = (unsigned long long)q & 0xffffffffull;
  *hi = (unsigned long long)(q >> 32);
}

__global__ void __launch_bounds__(BLOCK) topo_measure_kernel(const float* __restrict__ verts, const unsigned* __restrict__ idx, unsigned long long n_tris,
                                                             const unsigned* __restrict__ shell_of_vertex, unsigned* __restrict__ shell_of_face,
                                                             TopoShellAcc* __restrict__ acc, double sc_area, double sc_vol, double sc_mom) {
#pragma clang fp contract(off)
  const unsigned long long f = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  unsigned shell = TOPO_NONE;
  bool finite = false;
  unsigned long long s[10];
  unsigned bmin[3], bmax[3];
#pragma unroll
  for (int k = 0; k < 10; k++) s[k] = 0ull;
#pragma unroll
  for (int k = 0; k < 3; k++) { bmin[k] = 0xffffffffu; bmax[k] = 0u; }
  if (f < n_tris) {
    const unsigned ia = idx[3ull * f], ib = idx[3ull * f + 1ull], ic = idx[3ull * f + 2ull];
    if (!(ia == ib || ib == ic || ia == ic)) {
      shell = shell_of_vertex[ia];
      float p[9];
#pragma unroll
      for (int k = 0; k < 3; k++) { p[k] = verts[3ull * ia + k]; p[3 + k] = verts[3ull * ib + k]; p[6 + k] = verts[3ull * ic + k]; }
      finite = true;
#pragma unroll
      for (int k = 0; k < 9; k++) finite = finite && (__float_as_uint(p[k]) & 0x7fffffffu) < 0x7f800000u;
      if (finite) {
        const double ax = (double)p[0], ay = (double)p[1], az = (double)p[2];
        const double bx = (double)p[3], by = (double)p[4], bz = (double)p[5];
        const double cx = (double)p[6], cy = (double)p[7], cz = (double)p[8];
        const double ux = bx - ax, uy = by - ay, uz = bz - az, wx = cx - ax, wy = cy - ay, wz = cz - az;
        const double nx = uy * wz - uz * wy, ny = uz * wx - ux * wz, nz = ux * wy - uy * wx;
        const double area = 0.5 * __builtin_sqrt((nx * nx + ny * ny) + nz * nz);
        const double mx = by * cz - bz * cy, my = bz * cx - bx * cz, mz = bx * cy - by * cx;
        const double det = (ax * mx + ay * my) + az * mz;
        topo_split(area, sc_area, &s[0], &s[1]);
        topo_split(det / 6.0, sc_vol, &s[2], &s[3]);
        topo_split((det * ((ax + bx) + cx)) / 24.0, sc_mom, &s[4], &s[5]);
        topo_split((det * ((ay + by) + cy)) / 24.0, sc_mom, &s[6], &s[7]);
        topo_split((det * ((az + bz) + cz)) / 24.0, sc_mom, &s[8], &s[9]);
#pragma unroll
        for (int k = 0; k < 3; k++) {
          const unsigned o0 = topo_ordered(__float_as_uint(p[k])), o1 = topo_ordered(__float_as_uint(p[3 + k])), o2 = topo_ordered(__float_as_uint(p[6 + k]));
          bmin[k] = min(o0, min(o1, o2));
          bmax[k] = max(o0, max(o1, o2));
        }
      }
    }
    shell_of_face[f] = shell;
  }
  const TopoWave w = topo_wave(shell);
  topo_count(w, shell, true, acc, TOPO_F_NTRIS);
  topo_count(w, shell, !finite, acc, TOPO_F_NONFINITE);
#pragma unroll
  for (int k = 0; k < 10; k++) topo_add(w, shell, s[k], acc, TOPO_F_SUM + k);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    topo_minmax(w, shell, bmin[k], false, acc, TOPO_BB_WORD + k);
    topo_minmax(w, shell, bmax[k], true, acc, TOPO_BB_WORD + 3 + k);
  }
}

// A cell per lane: f uses forward, r reverse. boundary f + r == 1; non-manifold f + r > 2; misoriented f + r == 2 and f != 1.
__global__ void __launch_bounds__(BLOCK) topo_classify_kernel(const unsigned long long* __restrict__ tab_key, const unsigned* __restrict__ tab_cnt,
                                                              unsigned long long cells, const unsigned* __restrict__ shell_of_vertex, TopoShellAcc* __restrict__ acc) {
  const unsigned long long c = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  unsigned shell = TOPO_NONE, fw = 0, rv = 0;
  if (c < cells) {
    const unsigned long long key = tab_key[c];
    if (key != WELD_EMPTY_KEY) {
      shell = shell_of_vertex[(unsigned)(key >> 32)];
      fw = tab_cnt[2ull * c];
      rv = tab_cnt[2ull * c + 1ull];
    }
  }
  const unsigned long long uses = (unsigned long long)fw + rv;
  const TopoWave w = topo_wave(shell);
  topo_count(w, shell, true, acc, TOPO_F_EDGES);
  topo_count(w, shell, uses == 1ull, acc, TOPO_F_BOUNDARY);
  topo_count(w, shell, uses > 2ull, acc, TOPO_F_NONMANIFOLD);
  topo_count(w, shell, uses == 2ull && fw != 1u, acc, TOPO_F_MISORIENTED);
}

// ---- extract -----------------------------------------------------------------------------------------------------------------------
// keep[f]: the face's shell is kept (keep_shell NULL: every shell), or the face is degenerate and keep_degenerate says so.
__global__ void __launch_bounds__(BLOCK) topo_keep_kernel(const unsigned* __restrict__ shell_of_face, unsigned long long n_tris, const unsigned char* __restrict__ keep_shell,
                                                          int keep_degenerate, unsigned char* __restrict__ keep, unsigned* __restrict__ blk_cnt) {
  __shared__ unsigned s_w[4];
  const unsigned long long f = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  bool k = false;
  if (f < n_tris) {
    const unsigned s = shell_of_face[f];
    k = s == TOPO_NONE ? keep_degenerate != 0 : (keep_shell ? keep_shell[s] != 0 : true);
    keep[f] = k ? 1 : 0;
  }
  const unsigned total = block_count(k, s_w);
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = total;
}

// Kept faces in their order -> out[3 g + c] = the OLD vertex numbers; first[v] = the smallest new slot that names v (memset 0xff before)
__global__ void __launch_bounds__(BLOCK) topo_compact_kernel(const unsigned* __restrict__ idx, const unsigned char* __restrict__ keep, unsigned long long n_tris,
                                                             const unsigned* __restrict__ blk_base, unsigned* __restrict__ out, unsigned* __restrict__ first) {
  __shared__ unsigned s_w[4];
  const unsigned long long f = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const bool k = f < n_tris && keep[f] != 0;
  const unsigned rank = block_rank(k, s_w);
  if (k) {
    const unsigned long long g = (unsigned long long)blk_base[blockIdx.x] + rank;
#pragma unroll
    for (unsigned c = 0; c < 3u; c++) {
      const unsigned v = idx[3ull * f + c];
      out[3ull * g + c] = v;
      atomicMin(first + v, (unsigned)(3ull * g + c));
    }
  }
}

__global__ void __launch_bounds__(BLOCK) topo_owner_kernel(const unsigned* __restrict__ out, unsigned long long n_slots, const unsigned* __restrict__ first,
                                                           unsigned* __restrict__ blk_cnt) {
  __shared__ unsigned s_w[4];
  const unsigned long long s = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const bool owner = s < n_slots && first[out[s]] == (unsigned)s;
  const unsigned total = block_count(owner, s_w);
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = total;
}

// Owners -> new vertex numbers in slot order; positions, keys and normals carried bit for bit (as integers).
__global__ void __launch_bounds__(BLOCK) topo_renumber_kernel(const unsigned* __restrict__ out, unsigned long long n_slots, const unsigned* __restrict__ first,
                                                              const unsigned* __restrict__ blk_base, unsigned* __restrict__ vnum,
                                                              const unsigned* __restrict__ verts, const unsigned long long* __restrict__ vkeys,
                                                              const unsigned* __restrict__ normals, unsigned* __restrict__ nverts,
                                                              unsigned long long* __restrict__ nkeys, unsigned* __restrict__ nnormals) {
  __shared__ unsigned s_w[4];
  const unsigned long long s = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const unsigned old = s < n_slots ? out[s] : 0u;
  const bool owner = s < n_slots && first[old] == (unsigned)s;
  const unsigned rank = block_rank(owner, s_w);
  if (owner) {
    const unsigned v = blk_base[blockIdx.x] + rank;
    vnum[old] = v;
#pragma unroll
    for (unsigned k = 0; k < 3u; k++) {
      nverts[3ull * v + k] = verts[3ull * old + k];
      if (normals) nnormals[3ull * v + k] = normals[3ull * old + k];
    }
    nkeys[v] = vkeys[old];
  }
}

// ---- dual contouring's indexed mesh (gsdf_hip_mesh_dualcontour_indexed): extract's shape, a kept CUBE where extract has an old vertex --
// out[s] = the cube of slot s (kernels_dc_indexed.h: dci_rank_kernel). first[cube] = the smallest slot that names it (memset 0xff
// before); topo_owner_kernel counts the owners; then owners -> vertex numbers in slot order, the position = the cube's placed vertex
// (fv, bit for bit, as integers), the key = the cube's lattice coordinates, kind 5; remap_kernel writes the faces.
// Every out[s] is below the cubes' capacity: dci_rank_kernel tests the four indices of a quad before it writes them, and the host
// does not come here unless every slot was written (its *bad is 0). So neither this kernel, nor topo_owner_kernel, nor
// cube_number_kernel tests them again.
__global__ void __launch_bounds__(BLOCK) cube_first_kernel(const unsigned* __restrict__ out, unsigned long long n_slots, unsigned* __restrict__ first) {
  const unsigned long long s = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  if (s < n_slots) atomicMin(first + out[s], (unsigned)s);
}

__global__ void __launch_bounds__(BLOCK) cube_number_kernel(const unsigned* __restrict__ out, unsigned long long n_slots, const unsigned* __restrict__ first,
                                                            const unsigned* __restrict__ blk_base, unsigned* __restrict__ vnum, const unsigned* __restrict__ fv,
                                                            const Cube* __restrict__ cubes, unsigned* __restrict__ nverts, unsigned long long* __restrict__ nkeys) {
  __shared__ unsigned s_w[4];
  const unsigned long long s = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const unsigned old = s < n_slots ? out[s] : 0u;
  const bool owner = s < n_slots && first[old] == (unsigned)s;
  const unsigned rank = block_rank(owner, s_w);
  if (owner) {
    const unsigned v = blk_base[blockIdx.x] + rank;
    vnum[old] = v;
#pragma unroll
    for (unsigned k = 0; k < 3u; k++) nverts[3ull * v + k] = fv[3ull * old + k];
    const Cube c = cubes[old];
    nkeys[v] = (unsigned long long)c.x | ((unsigned long long)c.y << 20) | ((unsigned long long)c.z << 40) | (5ull << 60);
  }
}
