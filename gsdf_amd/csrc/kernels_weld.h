// kernels_weld.h -- indexed meshes: the marching-cubes vertices of a records mesh welded by lattice edge, and the binary PLY of
// the result (include/gsdf_hip.h: "indexed meshes" states the contract; abi_indexed.hip launches these). Also what the weld shares
// with the report (kernels_topo.h): the open-addressing table, a workgroup's flag count / rank, the scan across blocks, the remap.
//
// The soup of gsdf_hip_mesh_march (march_dense_kernel) is a function of the packed records: chunk c of DENSE_CHUNK records starts
// at triangle sum(chunk_tri[< c]), a record's triangles follow those of the records before it in its chunk, in table order, each
// with its corners reversed. So every slot's key can be written without looking at a float coordinate:
//   weld_chunk_scan_kernel   exclusive prefix of the chunks' triangle counts (one workgroup)
//   weld_keys_kernel         one record per lane -> the keys of its slots
//   weld_insert_kernel       key -> its cell of the table (table_claim), 32-bit atomicMin on the cell's slot
//   weld_owner_kernel        slot -> the smallest slot with its key (table_find); owners counted per block of 256 slots
//   block_scan_kernel        exclusive prefix of the blocks' owner counts (one workgroup): the carry across blocks
//   weld_number_kernel       the owner's rank in its block (block_rank) + the block's carry: owner -> vertex number; gathers the
//                            owner's position out of the soup, and its key
//   remap_kernel             idx[s] = number of slot s's owner
// The table's content after weld_insert_kernel does not depend on the order of arrival: a cell's key is set once, its slot is a
// minimum. Which CELL a key lands in does depend on it, and nothing reads that.
#pragma once
#include "kernels_common.h"

#define WELD_EMPTY_KEY 0xffffffffffffffffull
#define WELD_MAX_PROBES 4096u  // a probe sequence this long means a table far too full: the pass gives up and the host grows it

#define TABLE_NONE 0xffffffffffffffffull  // no cell (a cell index is below 2^32)

struct TableCounters {
  unsigned long long overflow;  // a key found no cell within WELD_MAX_PROBES
  unsigned long long probes;    // cells inspected by the inserting pass
  unsigned long long distinct;  // keys that claimed a cell
};

__device__ __forceinline__ unsigned weld_hash(unsigned long long k) {
  k ^= k >> 33;
  k *= 0xff51afd7ed558ccdull;
  k ^= k >> 33;
  k *= 0xc4ceb9fe1a85ec53ull;
  k ^= k >> 33;
  return (unsigned)k;
}

// ---- the open-addressing table: tab_key[mask + 1], every cell WELD_EMPTY_KEY before the pass (a memset of 0xff) ----------------
// The cell of `key`, claimed by a 64-bit compare-and-swap on the empty key if no thread had it yet (*is_new += 1 then); linear
// probing, *probes += the cells inspected. TABLE_NONE after WELD_MAX_PROBES cells: the host grows the table and runs the pass again.
__device__ __forceinline__ unsigned long long table_claim(unsigned long long* tab_key, unsigned mask, unsigned long long key, unsigned* probes,
                                                          unsigned* is_new) {
  unsigned h = weld_hash(key) & mask;
  for (unsigned n = 0; n < WELD_MAX_PROBES && n <= mask; n++) {
    (*probes)++;
    unsigned long long seen = tab_key[h];
    if (seen == WELD_EMPTY_KEY) {
      seen = atomicCAS(&tab_key[h], WELD_EMPTY_KEY, key);
      if (seen == WELD_EMPTY_KEY) { (*is_new)++; seen = key; }
    }
    if (seen == key) return h;
    h = (h + 1u) & mask;
  }
  return TABLE_NONE;
}
// Read-only: the cell that holds `key`, TABLE_NONE if the table does not (the probe met an empty cell, or every cell).
__device__ __forceinline__ unsigned long long table_find(const unsigned long long* tab_key, unsigned mask, unsigned long long key) {
  unsigned h = weld_hash(key) & mask;
  for (unsigned n = 0; n <= mask; n++) {
    const unsigned long long seen = tab_key[h];
    if (seen == key) return h;
    if (seen == WELD_EMPTY_KEY) break;
    h = (h + 1u) & mask;
  }
  return TABLE_NONE;
}
// An inserting pass's statistics, one atomic per wave and counter. Every lane of the wave calls it (it shuffles).
__device__ __forceinline__ void table_stats(unsigned probes, unsigned is_new, bool lost, TableCounters* ctr) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) { probes += __shfl_down(probes, off, 64); is_new += __shfl_down(is_new, off, 64); }
  const bool any_lost = __ballot(lost) != 0ull;
  if ((threadIdx.x & 63u) == 0u) {
    if (probes) atomicAdd(&ctr->probes, (unsigned long long)probes);
    if (is_new) atomicAdd(&ctr->distinct, (unsigned long long)is_new);
    if (any_lost) atomicMax(&ctr->overflow, 1ull);
  }
}

// ---- flags of one workgroup: how many are set (valid in thread 0 after the call) / the rank of this thread's among them ---------
// s_w: 4 words of LDS. Every thread of the workgroup calls them (they synchronise).
__device__ __forceinline__ unsigned block_count(bool flag, unsigned* s_w) {
  const unsigned cnt = (unsigned)__builtin_popcountll(__ballot(flag));
  if ((threadIdx.x & 63u) == 0u) s_w[threadIdx.x >> 6] = cnt;
  __syncthreads();
  return s_w[0] + s_w[1] + s_w[2] + s_w[3];
}
__device__ __forceinline__ unsigned block_rank(bool flag, unsigned* s_w) {
  const unsigned long long m = __ballot(flag);
  const unsigned wave = threadIdx.x >> 6;
  const unsigned before = __builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));  // exclusive, inside the wave
  if ((threadIdx.x & 63u) == 0u) s_w[wave] = (unsigned)__builtin_popcountll(m);
  __syncthreads();
  return (wave > 0 ? s_w[0] : 0u) + (wave > 1 ? s_w[1] : 0u) + (wave > 2 ? s_w[2] : 0u) + before;
}

// |v| < 1e-12f as mcInterpolate asks it (marchcubes.go:84-90: abs(0 - v) < 1e-12), on the bits: false for a NaN in every build
__device__ __forceinline__ bool weld_snaps(uint32_t bits) { return (bits & 0x7fffffffu) < __float_as_uint(1e-12f); }

// The key of the vertex marching cubes puts on edge `ed` (march_edge_word) of the leaf (lx, ly, lz) with corner distances d[8].
__device__ __forceinline__ unsigned long long weld_key(uint32_t ed, const uint32_t* d, unsigned lx, unsigned ly, unsigned lz) {
  const unsigned pa = (ed >> 8) & 7u, axis = (ed >> 6) & 3u, pb = pa ^ (1u << axis);
  const bool k1 = weld_snaps(d[ed & 7u]), k2 = weld_snaps(d[(ed >> 3) & 7u]);
  unsigned off = pa & pb, kind = axis;  // the edge's lower end
  if (k1 != k2) { off = k1 ? pa : pb; kind = 3u; }
  const unsigned long long ix = lx + (off & 1u), iy = ly + ((off >> 1) & 1u), iz = lz + ((off >> 2) & 1u);
  return ix | (iy << 20) | (iz << 40) | ((unsigned long long)kind << 60);
}

// chunk_tri[n_chunks] (the payload's tail) -> chunk_base[n_chunks], exclusive, in triangles. One workgroup of 1024 threads.
__global__ void __launch_bounds__(1024) weld_chunk_scan_kernel(const uint32_t* __restrict__ chunk_tri, unsigned long long n_chunks,
                                                               uint32_t* __restrict__ chunk_base) {
  __shared__ unsigned long long s_w[16];
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const unsigned long long per = (n_chunks + 1023ull) / 1024ull;
  unsigned long long e0 = (unsigned long long)tid * per, e1 = e0 + per;
  if (e0 > n_chunks) e0 = n_chunks;
  if (e1 > n_chunks) e1 = n_chunks;
  unsigned long long mine = 0;
  for (unsigned long long e = e0; e < e1; e++) mine += chunk_tri[e];
  unsigned long long incl = mine;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const unsigned lo = __shfl_up((unsigned)incl, off, 64), hi = __shfl_up((unsigned)(incl >> 32), off, 64);
    if (lane >= (unsigned)off) incl += ((unsigned long long)hi << 32) | lo;
  }
  if (lane == 63u) s_w[wave] = incl;
  __syncthreads();
  unsigned long long before = 0;
  for (unsigned w = 0; w < wave; w++) before += s_w[w];
  unsigned long long acc = before + incl - mine;
  for (unsigned long long e = e0; e < e1; e++) {
    chunk_base[e] = (uint32_t)acc;  // (3 F < 2^32 was checked on the host)
    acc += chunk_tri[e];
  }
}

// One record per lane, one chunk per workgroup pass.
__global__ void __launch_bounds__(BLOCK) weld_keys_kernel(const uint8_t* __restrict__ payload, unsigned long long n_recs,
                                                          const uint32_t* __restrict__ chunk_base, unsigned long long n_slots,
                                                          unsigned long long* __restrict__ keys) {
  __shared__ unsigned s_w[4];
  struct __attribute__((packed, aligned(8))) Rec { uint32_t w[REC_WORDS]; };
  const unsigned lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const unsigned long long n_chunks = (n_recs + DENSE_CHUNK - 1ull) / DENSE_CHUNK;
  for (unsigned long long c = blockIdx.x; c < n_chunks; c += gridDim.x) {  // block-uniform
    const unsigned long long q = c * DENSE_CHUNK + threadIdx.x;
    uint32_t rw[REC_WORDS];
#pragma unroll
    for (int k = 0; k < REC_WORDS; k++) rw[k] = 0u;
    if (q < n_recs) {
      const Rec v = *(const Rec*)(payload + q * 40ull);
#pragma unroll
      for (int k = 0; k < REC_WORDS; k++) rw[k] = v.w[k];
    }
    const unsigned index = (rw[9] >> 16) & 255u;
    const unsigned nt = q < n_recs ? (unsigned)GSDF_MC_NTRI[index] : 0u;
    const unsigned incl = wave_incl_scan_u32(nt);
    __syncthreads();  // the previous pass's readers are done with s_w
    if (lane == 63u) s_w[wave] = incl;
    __syncthreads();
    const unsigned first = (wave > 0 ? s_w[0] : 0u) + (wave > 1 ? s_w[1] : 0u) + (wave > 2 ? s_w[2] : 0u) + (incl - nt);
    const unsigned long long s0 = 3ull * ((unsigned long long)chunk_base[c] + first);
    const unsigned lx = rw[8] & 0xffffu, ly = rw[8] >> 16, lz = rw[9] & 0xffffu;
    for (unsigned k = 0; k < nt; k++) {
#pragma unroll
      for (unsigned j = 0; j < 3u; j++) {
        const int e = GSDF_MC_TRI[index][3u * k + (2u - j)];  // reversed winding (marchcubes.go:64-68), as the marching kernels
        const unsigned long long s = s0 + 3ull * k + j;
        if (s < n_slots) keys[s] = weld_key(march_edge_word((unsigned)e & 15u), rw, lx, ly, lz);  // (s >= n_slots: damaged counts)
      }
    }
  }
}

// tab_slot[cells] = 0xffffffff before the pass (the table's memset of 0xff covers it); mask = cells - 1.
__global__ void __launch_bounds__(BLOCK) weld_insert_kernel(const unsigned long long* __restrict__ keys, unsigned long long n_slots,
                                                            unsigned long long* __restrict__ tab_key, unsigned* __restrict__ tab_slot,
                                                            unsigned mask, TableCounters* __restrict__ ctr) {
  unsigned my_probes = 0, my_new = 0;
  bool lost = false;
  const unsigned long long step = (unsigned long long)gridDim.x * BLOCK;
  for (unsigned long long s = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; s < n_slots; s += step) {
    const unsigned long long cell = table_claim(tab_key, mask, keys[s], &my_probes, &my_new);
    if (cell != TABLE_NONE) atomicMin(&tab_slot[cell], (unsigned)s);
    else lost = true;
  }
  table_stats(my_probes, my_new, lost, ctr);
}

// idx[s] = the smallest slot with slot s's key; blk_cnt[b] = owners (idx[s] == s) among slots [256 b, 256 b + 256).
__global__ void __launch_bounds__(BLOCK) weld_owner_kernel(const unsigned long long* __restrict__ keys, unsigned long long n_slots,
                                                           const unsigned long long* __restrict__ tab_key, const unsigned* __restrict__ tab_slot,
                                                           unsigned mask, unsigned* __restrict__ idx, unsigned* __restrict__ blk_cnt) {
  __shared__ unsigned s_w[4];
  const unsigned long long s = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  bool owner = false;
  if (s < n_slots) {
    const unsigned long long cell = table_find(tab_key, mask, keys[s]);  // every key is in the table
    const unsigned own = cell != TABLE_NONE ? tab_slot[cell] : (unsigned)s;
    idx[s] = own;
    owner = own == (unsigned)s;
  }
  const unsigned total = block_count(owner, s_w);
  if (threadIdx.x == 0) blk_cnt[blockIdx.x] = total;
}

// blk_cnt[n_blocks] -> blk_base[n_blocks], exclusive; their sum -> *total. One workgroup of 1024 threads.
__global__ void __launch_bounds__(1024) block_scan_kernel(const unsigned* __restrict__ blk_cnt, unsigned n_blocks, unsigned* __restrict__ blk_base,
                                                          unsigned long long* __restrict__ total) {
  __shared__ unsigned s_w[16];
  const unsigned tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  const unsigned per = (n_blocks + 1023u) / 1024u;
  unsigned e0 = tid * per, e1 = e0 + per;
  if (e0 > n_blocks) e0 = n_blocks;
  if (e1 > n_blocks) e1 = n_blocks;
  unsigned mine = 0;
  for (unsigned e = e0; e < e1; e++) mine += blk_cnt[e];
  const unsigned incl = wave_incl_scan_u32(mine);
  if (lane == 63u) s_w[wave] = incl;
  __syncthreads();
  unsigned before = 0, sum = 0;
  for (unsigned w = 0; w < 16u; w++) {
    if (w < wave) before += s_w[w];
    sum += s_w[w];
  }
  unsigned acc = before + incl - mine;
  for (unsigned e = e0; e < e1; e++) {
    blk_base[e] = acc;
    acc += blk_cnt[e];
  }
  if (tid == 0) *total = sum;
}

// Owners -> vertex numbers, in slot order; the owner's position (soup: 3 floats per slot) and key go to the vertex arrays.
__global__ void __launch_bounds__(BLOCK) weld_number_kernel(const unsigned* __restrict__ idx, unsigned long long n_slots, const unsigned* __restrict__ blk_base,
                                                            const float* __restrict__ soup, const unsigned long long* __restrict__ keys,
                                                            unsigned* __restrict__ vnum, float* __restrict__ verts, unsigned long long* __restrict__ vkeys) {
  __shared__ unsigned s_w[4];
  const unsigned long long s = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const bool owner = s < n_slots && idx[s] == (unsigned)s;
  const unsigned rank = block_rank(owner, s_w);
  if (owner) {
    const unsigned v = blk_base[blockIdx.x] + rank;
    vnum[s] = v;
    const float* src = soup + 3ull * s;
    float* dst = verts + 3ull * v;
    dst[0] = src[0]; dst[1] = src[1]; dst[2] = src[2];
    vkeys[v] = keys[s];
  }
}

// idx[s] = vnum[idx[s]]: slots that name an owner / an old vertex -> slots that name its new number
__global__ void __launch_bounds__(BLOCK) remap_kernel(unsigned* __restrict__ idx, unsigned long long n_slots, const unsigned* __restrict__ vnum) {
  const unsigned long long s = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  if (s < n_slots) idx[s] = vnum[idx[s]];
}

// ---- binary PLY ----------------------------------------------------------------------------------------------------------------
// The header's length is a multiple of 4 (its comment line is padded), so the body is a stream of dwords.
// Vertex records: x y z (nx ny nz). out: the first dword behind the header.
__global__ void __launch_bounds__(BLOCK) ply_verts_kernel(const float* __restrict__ verts, const float* __restrict__ normals, unsigned long long n_verts,
                                                          uint32_t* __restrict__ out) {
  const unsigned stride = normals ? 6u : 3u;
  const unsigned long long n = n_verts * stride, step = (unsigned long long)gridDim.x * BLOCK;
  for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += step) {
    const unsigned long long v = i / stride;
    const unsigned c = (unsigned)(i - v * stride);
    out[i] = __float_as_uint(c < 3u ? verts[3ull * v + c] : normals[3ull * v + (c - 3u)]);
  }
}
// Face records of 13 bytes: 3, then three int32. A lane per output dword (the last one may run past the file's end, inside the
// buffer: the bytes behind the last face are written as 0).
__global__ void __launch_bounds__(BLOCK) ply_faces_kernel(const unsigned* __restrict__ idx, unsigned long long n_tris, uint32_t* __restrict__ out) {
  const unsigned long long nbytes = n_tris * 13ull, n = (nbytes + 3ull) / 4ull, step = (unsigned long long)gridDim.x * BLOCK;
  for (unsigned long long i = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x; i < n; i += step) {
    uint32_t w = 0;
#pragma unroll
    for (unsigned k = 0; k < 4u; k++) {
      const unsigned long long b = 4ull * i + k;
      if (b >= nbytes) break;
      const unsigned long long f = b / 13ull;
      const unsigned o = (unsigned)(b - f * 13ull);
      const uint32_t byte = o == 0u ? 3u : ((idx[3ull * f + (o - 1u) / 4u] >> (8u * ((o - 1u) & 3u))) & 255u);
      w |= byte << (8u * k);
    }
    out[i] = w;
  }
}
