// abi_indexed.hip -- C ABI (include/gsdf_hip.h), indexed meshes: the gsdf_indexed handle, the weld of a records mesh, counts /
// stats / reads, normals, the binary PLY, the report (edge classes, shells, measures) with the extraction of shells, and the
// projection of the vertices onto a program's field (its kernel is abi_eval.hip's: project_dev), and the numbering of dual
// contouring's quads into a handle (indexed_from_cube_slots: abi_mesh.hip orders them and owns the evaluating stages).
// Kernels: kernels_weld.h (weld, PLY, and the table / scan / remap every pass shares), kernels_topo.h (report, extract),
// kernels_mass.h (mass properties), kernels_simplify.h (simplify), kernels_simplify_adaptive.h (adaptive simplify), kernels_clean.h (clean). No
// interpreter kernel is compiled here: of the meshers this unit needs mesh_march_dense alone, and abi_mesh.hip owns that.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <new>
#include <type_traits>
#include <vector>

#include "kernels_common.h"
#include "kernels_weld.h"
#include "kernels_topo.h"
#define KERNELS_MASS_MESH
#include "kernels_mass.h"
#include "mass_host.h"
#include "kernels_simplify.h"
#include "kernels_simplify_adaptive.h"
#include "kernels_clean.h"
#include "abi_program.h"

namespace {
// a device buffer from the triangle pool (sized in 36-byte units), handed back when it goes out of scope
struct PoolBuf {
  int device = 0;
  float* p = nullptr;
  uint64_t cap = 0;
  PoolBuf() = default;
  PoolBuf(const PoolBuf&) = delete;
  PoolBuf& operator=(const PoolBuf&) = delete;
  ~PoolBuf() { give(); }
  void give() { pool_give(device, p, cap); p = nullptr; cap = 0; }
  bool take(int dev, size_t bytes) {
    give();
    device = dev;
    const uint64_t units = (bytes + 35) / 36 + 1;
    p = pool_take(dev, units, &cap);
    if (!p) {
      if (hipMalloc((void**)&p, units * 36) != hipSuccess) { (void)hipGetLastError(); p = nullptr; return false; }
      cap = units;
    }
    return true;
  }
  template <typename T> T* as() const { return (T*)p; }
};
struct EventPair {
  hipEvent_t a = nullptr, b = nullptr;
  ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
  bool make() { return hipEventCreate(&a) == hipSuccess && hipEventCreate(&b) == hipSuccess; }
  double ms() const { float t = 0; return hipEventElapsedTime(&t, a, b) == hipSuccess ? (double)t : 0.0; }
};
}  // namespace

struct gsdf_indexed {
  int device = 0;
  int num_cu = 256;
  hipStream_t stream = nullptr;
  uint64_t n_verts = 0, n_tris = 0;
  PoolBuf verts, idx, vkeys, normals;
  bool has_normals = false;
  double ms_device = 0;
  gsdf_indexed_stats st{};
  void* h_ply = nullptr;
  size_t h_ply_cap = 0, ply_len = 0;
  bool ply_valid = false;
  // gsdf_hip_indexed_report's result, computed once: the report, the shell table, the shell numbers of vertices and faces (device)
  bool topo_valid = false;
  gsdf_indexed_report rep{};
  std::vector<gsdf_shell> shells;
  PoolBuf shell_of_vertex, shell_of_face;
  // ... and the shells' integers behind its volume and centroid (volume, moment x / y / z), which gsdf_hip_indexed_mass carries on
  struct ShellInts { __int128 v[4]; };
  std::vector<ShellInts> shell_ints;
  // gsdf_hip_indexed_mass's result, computed once: the mesh's record, the shells' records, the device time of the pass
  bool mass_valid = false;
  gsdf_mass mass_total{};
  std::vector<gsdf_mass> mass_shells;
  double mass_ms = 0;
  // gsdf_hip_indexed_project's per-vertex record of the handle it made: d_before, d_after (V floats each), status (V bytes)
  bool has_fit = false;
  PoolBuf fit_before, fit_after, fit_status;
};

extern "C" void gsdf_hip_indexed_destroy(gsdf_indexed* ix) {
  if (!ix) return;
  (void)hipSetDevice(ix->device);
  if (ix->stream) { (void)hipStreamSynchronize(ix->stream); (void)hipStreamDestroy(ix->stream); }
  hpool_give(ix->h_ply, ix->h_ply_cap);
  delete ix;
}

namespace {
// A handle in the making: destroyed on every way out of its entry point except the one that release()s it to the caller.
struct IndexedDelete { void operator()(gsdf_indexed* ix) const { gsdf_hip_indexed_destroy(ix); } };
using IndexedPtr = std::unique_ptr<gsdf_indexed, IndexedDelete>;

// an empty handle on the calling thread's device, with its own stream
int indexed_new(int device, int num_cu, IndexedPtr* out) {
  IndexedPtr ix(new (std::nothrow) gsdf_indexed());
  if (!ix) return fail(GSDF_ERR_BAD_ARGUMENT, "out of memory");
  ix->device = device;
  ix->num_cu = num_cu;
  if (hipStreamCreateWithFlags(&ix->stream, hipStreamNonBlocking) != hipSuccess) {
    (void)hipGetLastError();
    ix->stream = nullptr;
    return fail(GSDF_ERR_HIP, "hipStreamCreate failed");
  }
  *out = std::move(ix);
  return GSDF_OK;
}

// (kernel parameters convert implicitly: a T* buffer goes to a const T* parameter as it is)
#define LAUNCH(KERNEL, GRID, THREADS, STREAM, ...)                                       \
  do {                                                                                   \
    hipLaunchKernelGGL(KERNEL, dim3(GRID), dim3(THREADS), 0, STREAM, __VA_ARGS__);       \
    HIP_TRY(hipGetLastError());                                                          \
  } while (0)

unsigned blocks_of(uint64_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

// blk_cnt[n_blocks] -> blk_base[n_blocks], exclusive, and their sum on the host: one round trip. d_total: 8 bytes of scratch.
int scan_blocks(hipStream_t s, const PoolBuf& blk_cnt, unsigned n_blocks, const PoolBuf& blk_base, const PoolBuf& d_total, uint64_t* total) {
  LAUNCH(block_scan_kernel, 1, 1024, s, blk_cnt.as<unsigned>(), n_blocks, blk_base.as<unsigned>(), d_total.as<unsigned long long>());
  unsigned long long h = 0;
  HIP_TRY(hipMemcpyAsync(&h, d_total.p, sizeof h, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *total = h;
  return GSDF_OK;
}

// An inserting pass over an open-addressing table (kernels_weld.h: table_claim) at load <= 0.5: a pass that ends fuller than that, or
// that gave up on a key, is repeated with twice the cells -- no key is ever dropped. The first size is the power of two >= `want`
// cells, or >= the value of floor_env where that is set: the tests' way into the growth path. pass(cells) memsets the table and the
// counters and launches the pass on s; d_head is where that pass's Head is on the device: its TableCounters, or a record that
// begins with them and goes on with whatever else the host wants to know after the same round trip.
template <typename Head>
struct TableRunOf {
  uint64_t cells = 0;
  int attempts = 0;
  Head head{};
};
using TableRun = TableRunOf<TableCounters>;
template <typename Head, typename Pass>
int table_build(const char* what, const char* floor_env, uint64_t want, size_t cell_bytes, int dev, hipStream_t s, PoolBuf& table, const void* d_head,
                Pass pass, TableRunOf<Head>* run) {
  want = env_u64(floor_env, want);  // (developer knob: a floor for the table, so that tests reach the regrowth)
  for (uint64_t cells = 1024;; cells <<= 1) {
    if (cells < want) continue;
    if (cells > ((uint64_t)1 << 32)) return fail(GSDF_ERR_CAPACITY, std::string(what) + ": hash table capacity exceeded");
    if (!table.take(dev, cells * cell_bytes)) return fail(GSDF_ERR_HIP, std::string(what) + ": no device memory for the workspace");
    run->attempts++;
    if (int rc = pass(cells)) return rc;
    HIP_TRY(hipMemcpyAsync(&run->head, d_head, sizeof run->head, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    static_assert(std::is_standard_layout<Head>::value && sizeof(Head) >= sizeof(TableCounters), "a head record begins with its TableCounters");
    TableCounters tc;
    std::memcpy(&tc, &run->head, sizeof tc);
    if (!tc.overflow && tc.distinct * 2 <= cells) {
      run->cells = cells;
      return GSDF_OK;
    }
  }
}
}  // namespace

// ---- the weld (kernels_weld.h) -------------------------------------------------------------------------------------------------
extern "C" int gsdf_hip_mesh_weld(const gsdf_mesh* m, gsdf_indexed** out) {
  if (!m || !out) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *out = nullptr;
  const bool marched = m->payload != GSDF_PAYLOAD_RECORDS;
  const uint8_t* d_recs = marched ? m->d_wrecs : m->d_recs;
  const uint64_t n_recs = marched ? m->n_wrecs : m->n_recs;
  if (!m->weldable || (!d_recs && m->st.n_tris))
    return fail(GSDF_ERR_BAD_ARGUMENT, "weld needs a mesh of the octree mesher made with payload = GSDF_PAYLOAD_RECORDS and shard_count == 1 (marched in place or "
                                       "not): triangle-payload, flat, dual-contouring, minecraft, gathered and sharded meshes carry no lattice coordinates");
  if (m->inflight.load() > 0) return fail(GSDF_ERR_BAD_ARGUMENT, "the mesh is being gathered: wait for the gather first");
  const uint64_t F = m->st.n_tris;
  if (F == 0) return fail(GSDF_ERR_EMPTY_BUFFERS, "empty triangle slice");
  if (3 * F >= ((uint64_t)1 << 32)) return fail(GSDF_ERR_CAPACITY, "weld: 3 x triangles must stay below 2^32 (32-bit vertex numbers)");
  HIP_TRY(hipSetDevice(m->device));
  const int dev = m->device;
  PoolBuf soup_tmp, keys, vnum, chunk_base, blk_cnt, blk_base, ctr, total, table;  // (before the handle: it goes first, and waits for its stream)
  IndexedPtr ix;
  if (int rc = indexed_new(dev, m->num_cu, &ix)) return rc;
  hipStream_t s = ix->stream;
  const uint64_t S = 3 * F;  // soup slots
  const uint64_t n_chunks = (n_recs + DENSE_CHUNK - 1) / DENSE_CHUNK;
  const unsigned n_blocks = blocks_of(S);
  const char* nomem = "weld: no device memory for the workspace";
  // the soup: the mesh's own triangles if it was marched, else a marching pass over its records into scratch
  const float* soup = m->d_tris;
  if (!marched) {
    if (!soup_tmp.take(dev, (size_t)F * 36 + dense_parts_bytes() + 36)) return fail(GSDF_ERR_HIP, nomem);
    const gsdf_dense_part part{0, n_recs, 0};
    if (int rc = mesh_march_dense(d_recs, &part, 1, dense_parts_at(soup_tmp.p, F), m->st.origin[0], m->st.origin[1], m->st.origin[2], m->st.res, soup_tmp.p,
                                  m->num_cu, s))
      return rc;
    soup = soup_tmp.p;
  }
  if (!keys.take(dev, S * 8) || !ix->idx.take(dev, S * 4) || !vnum.take(dev, S * 4) || !chunk_base.take(dev, n_chunks * 4 + 4) ||
      !blk_cnt.take(dev, (size_t)n_blocks * 4) || !blk_base.take(dev, (size_t)n_blocks * 4) || !ctr.take(dev, sizeof(TableCounters)) || !total.take(dev, 8))
    return fail(GSDF_ERR_HIP, nomem);
  EventPair ev_k, ev_i, ev_n;
  if (!ev_k.make() || !ev_i.make() || !ev_n.make()) return fail(GSDF_ERR_HIP, "hipEventCreate failed");
  // 1. keys
  HIP_TRY(hipEventRecord(ev_k.a, s));
  LAUNCH(weld_chunk_scan_kernel, 1, 1024, s, (const uint32_t*)(d_recs + n_recs * 40ull), (unsigned long long)n_chunks, chunk_base.as<uint32_t>());
  LAUNCH(weld_keys_kernel, grid_for(n_chunks * BLOCK, m->num_cu, 16), BLOCK, s, d_recs, (unsigned long long)n_recs, chunk_base.as<uint32_t>(),
         (unsigned long long)S, keys.as<unsigned long long>());
  HIP_TRY(hipEventRecord(ev_k.b, s));
  // 2. the table: 12 bytes per cell (the keys, then the slots), cells from F (V is about F / 2)
  TableRun run;
  HIP_TRY(hipEventRecord(ev_i.a, s));
  if (int rc = table_build("weld", "GSDF_HIP_WELD_CELLS_MIN", F, 12, dev, s, table, ctr.p, [&](uint64_t cells) -> int {
        HIP_TRY(hipMemsetAsync(table.p, 0xff, cells * 12, s));
        HIP_TRY(hipMemsetAsync(ctr.p, 0, sizeof(TableCounters), s));
        LAUNCH(weld_insert_kernel, grid_for(S, m->num_cu, 16), BLOCK, s, keys.as<unsigned long long>(), (unsigned long long)S, table.as<unsigned long long>(),
               (unsigned*)(table.as<unsigned long long>() + cells), (unsigned)(cells - 1), ctr.as<TableCounters>());
        return GSDF_OK;
      }, &run))
    return rc;
  HIP_TRY(hipEventRecord(ev_i.b, s));
  const uint64_t cells = run.cells;
  // 3. owners, numbers, positions, indices
  HIP_TRY(hipEventRecord(ev_n.a, s));
  LAUNCH(weld_owner_kernel, n_blocks, BLOCK, s, keys.as<unsigned long long>(), (unsigned long long)S, table.as<unsigned long long>(),
         (unsigned*)(table.as<unsigned long long>() + cells), (unsigned)(cells - 1), ix->idx.as<unsigned>(), blk_cnt.as<unsigned>());
  uint64_t V = 0;
  if (int rc = scan_blocks(s, blk_cnt, n_blocks, blk_base, total, &V)) return rc;
  if (V == 0 || V > S || V != run.head.distinct) return fail(GSDF_ERR_HIP, "weld: internal error (owners and distinct keys disagree)");
  if (!ix->verts.take(dev, V * 12) || !ix->vkeys.take(dev, V * 8)) return fail(GSDF_ERR_HIP, nomem);
  LAUNCH(weld_number_kernel, n_blocks, BLOCK, s, ix->idx.as<unsigned>(), (unsigned long long)S, blk_base.as<unsigned>(), soup, keys.as<unsigned long long>(),
         vnum.as<unsigned>(), ix->verts.p, ix->vkeys.as<unsigned long long>());
  LAUNCH(remap_kernel, n_blocks, BLOCK, s, ix->idx.as<unsigned>(), (unsigned long long)S, vnum.as<unsigned>());
  HIP_TRY(hipEventRecord(ev_n.b, s));
  HIP_TRY(hipStreamSynchronize(s));
  ix->n_verts = V;
  ix->n_tris = F;
  ix->st.ms_keys = ev_k.ms();
  ix->st.ms_insert = ev_i.ms();
  ix->st.ms_number = ev_n.ms();
  ix->st.probes = run.head.probes;
  ix->st.table_cells = cells;
  ix->st.attempts = run.attempts;
  ix->ms_device = ix->st.ms_keys + ix->st.ms_insert + ix->st.ms_number;
  *out = ix.release();
  return GSDF_OK;
}

// ---- dual contouring's indexed mesh: the numbering (abi_mesh.hip orders the quads; kernels_topo.h: cube_first_kernel) -------------
int launch_block_scan(const unsigned* d_cnt, unsigned n, unsigned* d_base, unsigned long long* d_total, hipStream_t s) {
  LAUNCH(block_scan_kernel, 1, 1024, s, d_cnt, n, d_base, d_total);
  return GSDF_OK;
}

namespace {
struct CubeSlotsWs { PoolBuf first, vnum, blk_cnt, blk_base, total; };  // (the caller's: it outlives the work on s on every way out)
int cube_slots_number(gsdf_indexed* ix, CubeSlotsWs& w, hipStream_t s, uint64_t S, uint64_t cube_cap, const float* d_fv, const Cube* d_cubes) {
  const int dev = ix->device;
  const unsigned n_blocks = blocks_of(S);
  const char* nomem = "dual contouring, indexed: no device memory for the workspace";
  PoolBuf &first = w.first, &vnum = w.vnum, &blk_cnt = w.blk_cnt, &blk_base = w.blk_base, &total = w.total;
  if (!first.take(dev, cube_cap * 4) || !vnum.take(dev, cube_cap * 4) || !blk_cnt.take(dev, (size_t)n_blocks * 4) || !blk_base.take(dev, (size_t)n_blocks * 4) ||
      !total.take(dev, 8))
    return fail(GSDF_ERR_HIP, nomem);
  EventPair ev;
  if (!ev.make()) return fail(GSDF_ERR_HIP, "hipEventCreate failed");
  HIP_TRY(hipEventRecord(ev.a, s));
  HIP_TRY(hipMemsetAsync(first.p, 0xff, cube_cap * 4, s));
  LAUNCH(cube_first_kernel, n_blocks, BLOCK, s, ix->idx.as<unsigned>(), (unsigned long long)S, first.as<unsigned>());
  LAUNCH(topo_owner_kernel, n_blocks, BLOCK, s, ix->idx.as<unsigned>(), (unsigned long long)S, first.as<unsigned>(), blk_cnt.as<unsigned>());
  uint64_t V = 0;
  if (int rc = scan_blocks(s, blk_cnt, n_blocks, blk_base, total, &V)) return rc;
  if (V == 0 || V > S || V > cube_cap) return fail(GSDF_ERR_HIP, "dual contouring, indexed: internal error (owners)");
  if (!ix->verts.take(dev, V * 12) || !ix->vkeys.take(dev, V * 8)) return fail(GSDF_ERR_HIP, nomem);
  LAUNCH(cube_number_kernel, n_blocks, BLOCK, s, ix->idx.as<unsigned>(), (unsigned long long)S, first.as<unsigned>(), blk_base.as<unsigned>(), vnum.as<unsigned>(),
         (const unsigned*)d_fv, d_cubes, ix->verts.as<unsigned>(), ix->vkeys.as<unsigned long long>());
  LAUNCH(remap_kernel, n_blocks, BLOCK, s, ix->idx.as<unsigned>(), (unsigned long long)S, vnum.as<unsigned>());
  HIP_TRY(hipEventRecord(ev.b, s));
  HIP_TRY(hipStreamSynchronize(s));
  ix->n_verts = V;
  ix->n_tris = S / 3;
  ix->st.ms_number = ev.ms();
  return GSDF_OK;
}
}  // namespace

int indexed_from_cube_slots(int device, int num_cu, hipStream_t s, float* d_slot_cube, uint64_t slot_cap36, uint64_t S, uint64_t cube_cap, const float* d_fv,
                            const void* d_cubes, const hipEvent_t key_ev[4], gsdf_indexed** out) {
  *out = nullptr;
  IndexedPtr ix;
  if (int rc = indexed_new(device, num_cu, &ix)) {
    (void)hipStreamSynchronize(s);  // (the ordering pass may still be writing the slots)
    pool_give(device, d_slot_cube, slot_cap36);
    return rc;
  }
  ix->idx.device = device; ix->idx.p = d_slot_cube; ix->idx.cap = slot_cap36;
  CubeSlotsWs w;
  if (int rc = cube_slots_number(ix.get(), w, s, S, cube_cap, d_fv, (const Cube*)d_cubes)) {
    (void)hipStreamSynchronize(s);  // the buffers go back to the pool: nothing may be running on them
    return rc;
  }
  float ta = 0, tb = 0;  // (s has been waited for)
  if (hipEventElapsedTime(&ta, key_ev[0], key_ev[1]) != hipSuccess || hipEventElapsedTime(&tb, key_ev[2], key_ev[3]) != hipSuccess) { (void)hipGetLastError(); ta = tb = 0; }
  ix->st.ms_keys = (double)ta + (double)tb;  // (no hash table: ms_insert, probes, table_cells, attempts stay 0)
  ix->ms_device = ix->st.ms_keys + ix->st.ms_number;
  *out = ix.release();
  return GSDF_OK;
}

extern "C" int gsdf_hip_indexed_counts(const gsdf_indexed* ix, uint64_t* n_verts, uint64_t* n_tris, double* ms_device) {
  if (!ix) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (n_verts) *n_verts = ix->n_verts;
  if (n_tris) *n_tris = ix->n_tris;
  if (ms_device) *ms_device = ix->ms_device;
  return GSDF_OK;
}

extern "C" int gsdf_hip_indexed_stats_get(const gsdf_indexed* ix, gsdf_indexed_stats* st) {
  if (!ix || !st) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *st = ix->st;
  st->has_normals = ix->has_normals ? 1 : 0;
  return GSDF_OK;
}

extern "C" int gsdf_hip_indexed_read(const gsdf_indexed* ix, float* verts, uint32_t* idx, uint64_t* keys) {
  if (!ix) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(ix->device));
  if (verts) HIP_TRY(hipMemcpy(verts, ix->verts.p, ix->n_verts * 12, hipMemcpyDeviceToHost));
  if (idx) HIP_TRY(hipMemcpy(idx, ix->idx.p, ix->n_tris * 12, hipMemcpyDeviceToHost));
  if (keys) HIP_TRY(hipMemcpy(keys, ix->vkeys.p, ix->n_verts * 8, hipMemcpyDeviceToHost));
  return GSDF_OK;
}

extern "C" int gsdf_hip_indexed_normals(gsdf_indexed* ix, gsdf_program* p, float step) {
  if (!ix || !p) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (p->device != ix->device) return fail(GSDF_ERR_BAD_ARGUMENT, "the program and the indexed mesh live on different devices");
  HIP_TRY(hipSetDevice(ix->device));
  if (!ix->normals.p && !ix->normals.take(ix->device, ix->n_verts * 12)) return fail(GSDF_ERR_HIP, "no device memory for the normals");
  ix->has_normals = false;
  ix->ply_valid = false;
  if (int rc = normals3_dev(p, ix->verts.p, ix->normals.p, (size_t)ix->n_verts, step)) return rc;
  ix->has_normals = true;
  return GSDF_OK;
}

extern "C" int gsdf_hip_indexed_read_normals(const gsdf_indexed* ix, float* normals) {
  if (!ix || !normals) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (!ix->has_normals) return fail(GSDF_ERR_BAD_ARGUMENT, "no normals yet: gsdf_hip_indexed_normals first");
  HIP_TRY(hipSetDevice(ix->device));
  HIP_TRY(hipMemcpy(normals, ix->normals.p, ix->n_verts * 12, hipMemcpyDeviceToHost));
  return GSDF_OK;
}

// ---- binary PLY ----------------------------------------------------------------------------------------------------------------
// The PLY header (gsdf_hip.h; gsdf_amd/ply.py writes the same bytes): its comment line is padded to a length that is a multiple of 4.
static std::string ply_header(uint64_t V, uint64_t F, bool normals) {
  std::string a = "ply\nformat binary_little_endian 1.0\ncomment gsdf";
  std::string b = "\nelement vertex " + std::to_string(V) + "\nproperty float x\nproperty float y\nproperty float z\n";
  if (normals) b += "property float nx\nproperty float ny\nproperty float nz\n";
  b += "element face " + std::to_string(F) + "\nproperty list uchar int vertex_indices\nend_header\n";
  a.append((4 - (a.size() + b.size()) % 4) % 4, ' ');
  return a + b;
}

extern "C" int gsdf_hip_indexed_host_ply(gsdf_indexed* ix, const uint8_t** ply, size_t* len) {
  if (!ix || !ply || !len) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *ply = nullptr; *len = 0;
  HIP_TRY(hipSetDevice(ix->device));
  if (!ix->ply_valid) {
    const std::string hdr = ply_header(ix->n_verts, ix->n_tris, ix->has_normals);
    const size_t vbytes = (size_t)ix->n_verts * (ix->has_normals ? 24 : 12), fbytes = (size_t)ix->n_tris * 13;
    const size_t bytes = hdr.size() + vbytes + fbytes;
    if (int rc = host_buf(&ix->h_ply, &ix->h_ply_cap, bytes + 4)) return rc;
    PoolBuf d_out;  // device scratch from the triangle pool (the last face dword may reach past the file's end)
    if (!d_out.take(ix->device, bytes + 4)) return fail(GSDF_ERR_HIP, "hipMalloc of the PLY scratch failed");
    EventPair ev;
    if (!ev.make()) return fail(GSDF_ERR_HIP, "hipEventCreate failed");
    std::memcpy(ix->h_ply, hdr.data(), hdr.size());  // pinned: a valid source for the async header upload
    hipStream_t s = ix->stream;
    uint8_t* o = (uint8_t*)d_out.p;
    hipError_t e = hipEventRecord(ev.a, s);
    if (e == hipSuccess) e = hipMemcpyAsync(o, ix->h_ply, hdr.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(ply_verts_kernel, dim3(grid_for(vbytes / 4, ix->num_cu, 8)), dim3(BLOCK), 0, s, ix->verts.p, ix->has_normals ? ix->normals.p : nullptr,
                         (unsigned long long)ix->n_verts, (uint32_t*)(o + hdr.size()));
      e = hipGetLastError();
    }
    if (e == hipSuccess) {
      hipLaunchKernelGGL(ply_faces_kernel, dim3(grid_for((fbytes + 3) / 4, ix->num_cu, 8)), dim3(BLOCK), 0, s, ix->idx.as<unsigned>(),
                         (unsigned long long)ix->n_tris, (uint32_t*)(o + hdr.size() + vbytes));
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(ix->h_ply, o, bytes, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipEventRecord(ev.b, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    else (void)hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(GSDF_ERR_HIP, std::string("PLY build/transfer: ") + hipGetErrorString(e));
    ix->st.ms_ply = ev.ms();
    ix->ply_len = bytes;
    ix->ply_valid = true;
  }
  *ply = (const uint8_t*)ix->h_ply;
  *len = ix->ply_len;
  return GSDF_OK;
}

extern "C" int gsdf_hip_indexed_ply(gsdf_indexed* ix, uint8_t* dst, size_t cap, size_t* len) {
  if (!ix || !len) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *len = ply_header(ix->n_verts, ix->n_tris, ix->has_normals).size() + (size_t)ix->n_verts * (ix->has_normals ? 24 : 12) + (size_t)ix->n_tris * 13;
  if (!dst || cap < *len) return fail(GSDF_ERR_SHORT_BUFFER, "short buffer");
  const uint8_t* h = nullptr;
  size_t n = 0;
  if (int rc = gsdf_hip_indexed_host_ply(ix, &h, &n)) return rc;
  big_memcpy(dst, h, n);
  return GSDF_OK;
}

// ---- report and extract (kernels_topo.h) -----------------------------------------------------------------------------------------
namespace {
float topo_unordered(unsigned o) {
  const uint32_t bits = (o & 0x80000000u) ? (o ^ 0x80000000u) : ~o;
  float f;
  std::memcpy(&f, &bits, 4);
  return f;
}
// low-word sum and (signed) rest sum of the quantised terms -> the integer they stand for
__int128 topo_int(const unsigned long long* s) { return (__int128)(long long)s[1] * ((__int128)1 << 32) + (__int128)s[0]; }
// that integer as float64 (one rounding) times 2^-shift (exact)
double topo_value(__int128 t, int shift) { return std::ldexp((double)t, -shift); }
double topo_quotient(double m, double v) {
  if (v == 0.0) {
    const uint64_t q = 0x7ff8000000000000ull;
    double d;
    std::memcpy(&d, &q, 8);
    return d;
  }
  return m / v;
}
}  // namespace

extern "C" int gsdf_hip_indexed_create(const float* verts, uint64_t n_verts, const uint32_t* idx, uint64_t n_tris, const uint64_t* keys, gsdf_indexed** out) {
  if (!out) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *out = nullptr;
  if (n_verts == 0 || n_tris == 0) return fail(GSDF_ERR_EMPTY_BUFFERS, "empty buffers");
  if (!verts || !idx) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (3 * n_tris >= ((uint64_t)1 << 32) || n_verts >= ((uint64_t)1 << 32))
    return fail(GSDF_ERR_CAPACITY, "indexed mesh: vertices and 3 x triangles must stay below 2^32 (32-bit vertex numbers)");
  for (uint64_t s = 0; s < 3 * n_tris; s++)
    if (idx[s] >= n_verts)
      return fail(GSDF_ERR_BAD_ARGUMENT, "indexed mesh: face " + std::to_string(s / 3) + " names vertex index " + std::to_string(idx[s]) + ", the mesh has " +
                                             std::to_string(n_verts) + " vertices");
  int device = 0;
  HIP_TRY(hipGetDevice(&device));
  const int num_cu = grid_cus(device);
  IndexedPtr ix;
  if (int rc = indexed_new(device, num_cu, &ix)) return rc;
  if (!ix->verts.take(device, n_verts * 12) || !ix->idx.take(device, n_tris * 12) || !ix->vkeys.take(device, n_verts * 8))
    return fail(GSDF_ERR_HIP, "indexed mesh: no device memory");
  hipError_t e = hipMemcpy(ix->verts.p, verts, n_verts * 12, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(ix->idx.p, idx, n_tris * 12, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = keys ? hipMemcpy(ix->vkeys.p, keys, n_verts * 8, hipMemcpyHostToDevice) : hipMemset(ix->vkeys.p, 0, n_verts * 8);
  if (e != hipSuccess) return fail(GSDF_ERR_HIP, std::string("indexed mesh upload: ") + hipGetErrorString(e));
  ix->n_verts = n_verts;
  ix->n_tris = n_tris;
  *out = ix.release();
  return GSDF_OK;
}

// The report, the shell table and the shell numbers, once per handle.
static int topo_ensure(gsdf_indexed* ix) {
  if (ix->topo_valid) return GSDF_OK;
  HIP_TRY(hipSetDevice(ix->device));
  const int dev = ix->device;
  hipStream_t s = ix->stream;
  const uint64_t V = ix->n_verts, F = ix->n_tris;
  const unsigned nb_v = blocks_of(V), nb_f = blocks_of(F);
  const char* nomem = "report: no device memory for the workspace";
  PoolBuf ctr, parent, used, root_of, shell_num, blk_cnt, blk_base, table, acc;
  if (!ctr.take(dev, sizeof(TopoCounters)) || !parent.take(dev, V * 4) || !used.take(dev, V * 4) || !root_of.take(dev, V * 4) || !shell_num.take(dev, V * 4) ||
      !blk_cnt.take(dev, (size_t)nb_v * 4) || !blk_base.take(dev, (size_t)nb_v * 4) || !ix->shell_of_vertex.take(dev, V * 4) ||
      !ix->shell_of_face.take(dev, F * 4))
    return fail(GSDF_ERR_HIP, nomem);
  TopoCounters* d_ctr = ctr.as<TopoCounters>();
  EventPair ev_e, ev_s, ev_m;
  if (!ev_e.make() || !ev_s.make() || !ev_m.make()) return fail(GSDF_ERR_HIP, "hipEventCreate failed");
  // 1. the edge table: 16 bytes per cell (the keys, then the two direction counters), cells from 3 F (about 3 F / 2 pairs). Then
  // the exponent.
  TableRun run;
  HIP_TRY(hipEventRecord(ev_e.a, s));
  if (int rc = table_build("report", "GSDF_HIP_TOPO_CELLS_MIN", 3 * F, 16, dev, s, table, &d_ctr->tab, [&](uint64_t cells) -> int {
        HIP_TRY(hipMemsetAsync(table.p, 0xff, cells * 8, s));
        HIP_TRY(hipMemsetAsync((uint8_t*)table.p + cells * 8, 0, cells * 8, s));
        HIP_TRY(hipMemsetAsync(d_ctr, 0, sizeof(TopoCounters), s));
        LAUNCH(topo_edge_insert_kernel, nb_f, BLOCK, s, ix->idx.as<unsigned>(), (unsigned long long)F, table.as<unsigned long long>(),
               (unsigned*)(table.as<unsigned long long>() + cells), (unsigned)(cells - 1), d_ctr);
        return GSDF_OK;
      }, &run))
    return rc;
  const uint64_t cells = run.cells;
  LAUNCH(topo_maxbits_kernel, grid_for(3 * V, ix->num_cu, 8), BLOCK, s, ix->verts.p, (unsigned long long)(3 * V), &d_ctr->maxbits);
  HIP_TRY(hipEventRecord(ev_e.b, s));
  // 2. shells
  HIP_TRY(hipEventRecord(ev_s.a, s));
  LAUNCH(topo_parent_init_kernel, nb_v, BLOCK, s, parent.as<unsigned>(), used.as<unsigned>(), (unsigned long long)V);
  LAUNCH(topo_union_kernel, nb_f, BLOCK, s, ix->idx.as<unsigned>(), (unsigned long long)F, parent.as<unsigned>(), used.as<unsigned>());
  LAUNCH(topo_root_kernel, nb_v, BLOCK, s, parent.as<unsigned>(), used.as<unsigned>(), (unsigned long long)V, root_of.as<unsigned>(), blk_cnt.as<unsigned>(), d_ctr);
  LAUNCH(block_scan_kernel, 1, 1024, s, blk_cnt.as<unsigned>(), nb_v, blk_base.as<unsigned>(), &d_ctr->n_shells);
  TopoCounters hc{};
  HIP_TRY(hipMemcpyAsync(&hc, d_ctr, sizeof hc, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const uint64_t n_shells = hc.n_shells;
  if (n_shells > V) return fail(GSDF_ERR_HIP, "report: internal error (more shells than vertices)");
  if (!acc.take(dev, (n_shells + 1) * sizeof(TopoShellAcc))) return fail(GSDF_ERR_HIP, nomem);
  TopoShellAcc* d_acc = acc.as<TopoShellAcc>();
  HIP_TRY(hipMemsetAsync(d_acc, 0, (n_shells + 1) * sizeof(TopoShellAcc), s));
  LAUNCH(topo_number_kernel, nb_v, BLOCK, s, root_of.as<unsigned>(), used.as<unsigned>(), (unsigned long long)V, blk_base.as<unsigned>(), shell_num.as<unsigned>(), d_acc);
  LAUNCH(topo_vertex_shell_kernel, nb_v, BLOCK, s, root_of.as<unsigned>(), used.as<unsigned>(), (unsigned long long)V, shell_num.as<unsigned>(),
         ix->shell_of_vertex.as<unsigned>(), d_acc);
  HIP_TRY(hipEventRecord(ev_s.b, s));
  // 3. measures and pair classes
  const int biased = (int)(hc.maxbits >> 23);
  const int e = (biased > 1 ? biased : 1) - 126;
  const int sh_area = 59 - 2 * e, sh_vol = 62 - 3 * e, sh_mom = 62 - 4 * e;
  HIP_TRY(hipEventRecord(ev_m.a, s));
  LAUNCH(topo_measure_kernel, nb_f, BLOCK, s, ix->verts.p, ix->idx.as<unsigned>(), (unsigned long long)F, ix->shell_of_vertex.as<unsigned>(),
         ix->shell_of_face.as<unsigned>(), d_acc, std::ldexp(1.0, sh_area), std::ldexp(1.0, sh_vol), std::ldexp(1.0, sh_mom));
  LAUNCH(topo_classify_kernel, blocks_of(cells), BLOCK, s, table.as<unsigned long long>(), (unsigned*)(table.as<unsigned long long>() + cells),
         (unsigned long long)cells, ix->shell_of_vertex.as<unsigned>(), d_acc);
  HIP_TRY(hipEventRecord(ev_m.b, s));
  std::vector<TopoShellAcc> ha(n_shells);
  if (n_shells) HIP_TRY(hipMemcpyAsync(ha.data(), d_acc, n_shells * sizeof(TopoShellAcc), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  // the shells' records; the mesh's sums are the sums of the shells' integers
  gsdf_indexed_report r{};
  std::vector<gsdf_shell> shells(n_shells);
  std::vector<gsdf_indexed::ShellInts> ints(n_shells);
  __int128 tot[5] = {0, 0, 0, 0, 0};
  unsigned bb[6] = {TOPO_BB_MIN_INIT, TOPO_BB_MIN_INIT, TOPO_BB_MIN_INIT, TOPO_BB_MAX_INIT, TOPO_BB_MAX_INIT, TOPO_BB_MAX_INIT};
  const int shift[5] = {sh_area, sh_vol, sh_mom, sh_mom, sh_mom};
  uint64_t tris = 0, edges_by_shell = 0;
  for (uint64_t k = 0; k < n_shells; k++) {
    const TopoShellAcc& a = ha[k];
    gsdf_shell& o = shells[k];
    o.n_verts = a.n_verts; o.n_tris = a.n_tris; o.nonfinite = a.nonfinite;
    o.edges = a.edges; o.boundary_edges = a.boundary; o.nonmanifold_edges = a.nonmanifold; o.misoriented_edges = a.misoriented;
    o.euler = (int64_t)a.n_verts - (int64_t)a.edges + (int64_t)a.n_tris;
    double val[5];
    for (int q = 0; q < 5; q++) {
      const __int128 t = topo_int(a.sum + 2 * q);
      tot[q] += t;
      val[q] = topo_value(t, shift[q]);
      if (q > 0) ints[k].v[q - 1] = t;
    }
    o.area = val[0]; o.volume = val[1];
    for (int q = 0; q < 3; q++) o.centroid[q] = topo_quotient(val[2 + q], val[1]);
    for (int q = 0; q < 6; q++) o.bbox[q] = topo_unordered(a.bb[q]);
    for (int q = 0; q < 3; q++) { bb[q] = std::min(bb[q], a.bb[q]); bb[3 + q] = std::max(bb[3 + q], a.bb[3 + q]); }
    o.label = a.label;
    r.nonfinite += a.nonfinite; r.boundary_edges += a.boundary; r.nonmanifold_edges += a.nonmanifold; r.misoriented_edges += a.misoriented;
    tris += a.n_tris; edges_by_shell += a.edges;
  }
  if (tris != F - hc.degenerate || edges_by_shell != hc.tab.distinct) return fail(GSDF_ERR_HIP, "report: internal error (the shells' counts do not add up)");
  r.n_verts = V; r.n_tris = F; r.degenerate = hc.degenerate; r.used_verts = hc.used_verts; r.edges = hc.tab.distinct; r.n_shells = n_shells;
  r.euler = (int64_t)r.used_verts - (int64_t)r.edges + (int64_t)(F - r.degenerate);
  r.area = topo_value(tot[0], shift[0]);
  r.volume = topo_value(tot[1], shift[1]);
  for (int q = 0; q < 3; q++) r.centroid[q] = topo_quotient(topo_value(tot[2 + q], shift[2 + q]), r.volume);
  for (int q = 0; q < 6; q++) r.bbox[q] = topo_unordered(bb[q]);
  r.closed_oriented = (r.degenerate == 0 && r.boundary_edges == 0 && r.nonmanifold_edges == 0 && r.misoriented_edges == 0) ? 1 : 0;
  r.exponent = e;
  r.ms_edges = ev_e.ms(); r.ms_shells = ev_s.ms(); r.ms_measure = ev_m.ms();
  r.probes = hc.tab.probes; r.table_cells = cells; r.attempts = run.attempts;
  ix->rep = r;
  ix->shells.swap(shells);
  ix->shell_ints.swap(ints);
  ix->topo_valid = true;
  return GSDF_OK;
}

extern "C" int gsdf_hip_indexed_report(gsdf_indexed* ix, gsdf_indexed_report* rep) {
  if (!ix || !rep) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (int rc = topo_ensure(ix)) return rc;
  *rep = ix->rep;
  return GSDF_OK;
}

extern "C" int gsdf_hip_indexed_shells(gsdf_indexed* ix, gsdf_shell* dst, uint64_t cap, uint64_t* n) {
  if (!ix || !n) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (int rc = topo_ensure(ix)) return rc;
  *n = ix->shells.size();
  if (!dst) return GSDF_OK;
  if (cap < *n) return fail(GSDF_ERR_SHORT_BUFFER, "short buffer");
  if (*n) std::memcpy(dst, ix->shells.data(), *n * sizeof(gsdf_shell));
  return GSDF_OK;
}

extern "C" int gsdf_hip_indexed_read_shell_of(gsdf_indexed* ix, uint32_t* shell_of_vertex, uint32_t* shell_of_face) {
  if (!ix) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (int rc = topo_ensure(ix)) return rc;
  HIP_TRY(hipSetDevice(ix->device));
  if (shell_of_vertex) HIP_TRY(hipMemcpy(shell_of_vertex, ix->shell_of_vertex.p, ix->n_verts * 4, hipMemcpyDeviceToHost));
  if (shell_of_face) HIP_TRY(hipMemcpy(shell_of_face, ix->shell_of_face.p, ix->n_tris * 4, hipMemcpyDeviceToHost));
  return GSDF_OK;
}

// ---- mass properties (kernels_mass.h, mass_host.h; gsdf_hip.h: "indexed meshes: mass properties") ---------------------------------
namespace {
thread_local double g_mass_ms = 0;
}
extern "C" double gsdf_hip_indexed_mass_ms(void) { return g_mass_ms; }

// The second moments of the shells, once per handle, behind the report (whose exponent, shell numbering and first-degree integers
// it takes over).
static int mass_ensure(gsdf_indexed* ix) {
  if (ix->mass_valid) return GSDF_OK;
  if (int rc = topo_ensure(ix)) return rc;
  HIP_TRY(hipSetDevice(ix->device));
  const int dev = ix->device;
  hipStream_t s = ix->stream;
  const uint64_t F = ix->n_tris, n_shells = ix->shells.size();
  const int e = ix->rep.exponent;
  PoolBuf acc;
  if (!acc.take(dev, (n_shells + 1) * sizeof(MassShellAcc))) return fail(GSDF_ERR_HIP, "mass: no device memory for the workspace");
  MassShellAcc* d_acc = acc.as<MassShellAcc>();
  EventPair ev;
  if (!ev.make()) return fail(GSDF_ERR_HIP, "hipEventCreate failed");
  std::vector<MassShellAcc> ha(n_shells);
  HIP_TRY(hipEventRecord(ev.a, s));
  HIP_TRY(hipMemsetAsync(d_acc, 0, (n_shells + 1) * sizeof(MassShellAcc), s));
  LAUNCH(mass_second_kernel, blocks_of(F), BLOCK, s, ix->verts.p, ix->idx.as<unsigned>(), (unsigned long long)F, ix->shell_of_face.as<unsigned>(), d_acc,
         std::ldexp(1.0, 62 - 5 * e));
  HIP_TRY(hipEventRecord(ev.b, s));
  if (n_shells) HIP_TRY(hipMemcpyAsync(ha.data(), d_acc, n_shells * sizeof(MassShellAcc), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  // the shells' records; the mesh's integers are the sums of the shells'
  std::vector<gsdf_mass> shells(n_shells);
  __int128 tot[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (uint64_t k = 0; k < n_shells; k++) {
    __int128 sums[10];
    for (int q = 0; q < 4; q++) sums[q] = ix->shell_ints[k].v[q];
    for (int q = 0; q < 6; q++) sums[4 + q] = mass::whole(ha[k].sum[2 * q], ha[k].sum[2 * q + 1]);
    for (int q = 0; q < 10; q++) tot[q] += sums[q];
    mass::fill_mass(&shells[k], sums, e, ix->shells[k].label);
  }
  mass::fill_mass(&ix->mass_total, tot, e, 0xffffffffu);
  ix->mass_shells.swap(shells);
  ix->mass_ms = ev.ms();
  ix->mass_valid = true;
  return GSDF_OK;
}

extern "C" int gsdf_hip_indexed_mass(gsdf_indexed* ix, gsdf_mass* total, gsdf_mass* shells, uint64_t cap, uint64_t* n) {
  g_mass_ms = 0;
  if (!ix) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (!total && !shells && !n) return fail(GSDF_ERR_BAD_ARGUMENT, "mass: nothing asked for (total, shells and n are all null)");
  if (shells && !n) return fail(GSDF_ERR_BAD_ARGUMENT, "mass: shells needs n (a short buffer is reported through it)");
  if (int rc = mass_ensure(ix)) return rc;
  g_mass_ms = ix->mass_ms;
  if (total) *total = ix->mass_total;
  if (n) *n = ix->mass_shells.size();
  if (!shells) return GSDF_OK;
  if (cap < *n) return fail(GSDF_ERR_SHORT_BUFFER, "short buffer");
  if (*n) std::memcpy(shells, ix->mass_shells.data(), *n * sizeof(gsdf_mass));
  return GSDF_OK;
}

extern "C" int gsdf_hip_indexed_extract(gsdf_indexed* ix, const uint8_t* keep_shell, int drop_degenerate, gsdf_indexed** out) {
  if (!ix || !out) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *out = nullptr;
  if (int rc = topo_ensure(ix)) return rc;
  HIP_TRY(hipSetDevice(ix->device));
  const int dev = ix->device;
  hipStream_t s = ix->stream;
  const uint64_t V = ix->n_verts, F = ix->n_tris, n_shells = ix->shells.size();
  const unsigned nb_f = blocks_of(F);
  const char* nomem = "extract: no device memory for the workspace";
  PoolBuf d_keep, keep, blk_cnt, blk_base, total, first, vnum;
  if (!keep.take(dev, F) || !blk_cnt.take(dev, (size_t)blocks_of(3 * F) * 4) || !blk_base.take(dev, (size_t)blocks_of(3 * F) * 4) || !total.take(dev, 8) ||
      !first.take(dev, V * 4) || !vnum.take(dev, V * 4))
    return fail(GSDF_ERR_HIP, nomem);
  if (keep_shell && n_shells) {
    if (!d_keep.take(dev, n_shells)) return fail(GSDF_ERR_HIP, nomem);
    HIP_TRY(hipMemcpyAsync(d_keep.p, keep_shell, n_shells, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));  // (the caller's bytes are pageable: they were read by now)
  }
  EventPair ev;
  if (!ev.make()) return fail(GSDF_ERR_HIP, "hipEventCreate failed");
  HIP_TRY(hipEventRecord(ev.a, s));
  // kept faces, in order
  LAUNCH(topo_keep_kernel, nb_f, BLOCK, s, ix->shell_of_face.as<unsigned>(), (unsigned long long)F, keep_shell ? d_keep.as<unsigned char>() : nullptr,
         (!drop_degenerate && !keep_shell) ? 1 : 0, keep.as<unsigned char>(), blk_cnt.as<unsigned>());
  uint64_t F2 = 0;
  if (int rc = scan_blocks(s, blk_cnt, nb_f, blk_base, total, &F2)) return rc;
  if (F2 == 0) return fail(GSDF_ERR_EMPTY_BUFFERS, "extract: nothing kept");
  if (F2 > F) return fail(GSDF_ERR_HIP, "extract: internal error (more faces kept than there are)");
  IndexedPtr nx;
  if (int rc = indexed_new(dev, ix->num_cu, &nx)) return rc;
  const uint64_t S2 = 3 * F2;
  const unsigned nb_s = blocks_of(S2);
  if (!nx->idx.take(dev, S2 * 4)) return fail(GSDF_ERR_HIP, nomem);
  HIP_TRY(hipMemsetAsync(first.p, 0xff, V * 4, s));
  LAUNCH(topo_compact_kernel, nb_f, BLOCK, s, ix->idx.as<unsigned>(), keep.as<unsigned char>(), (unsigned long long)F, blk_base.as<unsigned>(), nx->idx.as<unsigned>(),
         first.as<unsigned>());
  // vertices by their smallest kept slot
  LAUNCH(topo_owner_kernel, nb_s, BLOCK, s, nx->idx.as<unsigned>(), (unsigned long long)S2, first.as<unsigned>(), blk_cnt.as<unsigned>());
  uint64_t V2 = 0;
  if (int rc = scan_blocks(s, blk_cnt, nb_s, blk_base, total, &V2)) return rc;
  if (V2 == 0 || V2 > V) return fail(GSDF_ERR_HIP, "extract: internal error (kept vertices)");
  if (!nx->verts.take(dev, V2 * 12) || !nx->vkeys.take(dev, V2 * 8) || (ix->has_normals && !nx->normals.take(dev, V2 * 12))) return fail(GSDF_ERR_HIP, nomem);
  LAUNCH(topo_renumber_kernel, nb_s, BLOCK, s, nx->idx.as<unsigned>(), (unsigned long long)S2, first.as<unsigned>(), blk_base.as<unsigned>(), vnum.as<unsigned>(),
         ix->verts.as<unsigned>(), ix->vkeys.as<unsigned long long>(), ix->has_normals ? ix->normals.as<unsigned>() : nullptr, nx->verts.as<unsigned>(),
         nx->vkeys.as<unsigned long long>(), ix->has_normals ? nx->normals.as<unsigned>() : nullptr);
  LAUNCH(remap_kernel, nb_s, BLOCK, s, nx->idx.as<unsigned>(), (unsigned long long)S2, vnum.as<unsigned>());
  HIP_TRY(hipEventRecord(ev.b, s));
  HIP_TRY(hipStreamSynchronize(s));
  nx->n_verts = V2;
  nx->n_tris = F2;
  nx->has_normals = ix->has_normals;
  nx->ms_device = ev.ms();
  *out = nx.release();
  return GSDF_OK;
}

// ---- simplify (kernels_simplify.h) -----------------------------------------------------------------------------------------------
extern "C" int gsdf_hip_indexed_simplify(gsdf_indexed* ix, const gsdf_simplify_opts* o, gsdf_indexed** out, gsdf_simplify_stats* st) {
  if (out) *out = nullptr;
  if (!o) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (!(o->cell > 0.0f) || !std::isfinite(o->cell)) return fail(GSDF_ERR_BAD_ARGUMENT, "simplify: the cell edge must be positive and finite");
  if (!std::isfinite(o->origin[0]) || !std::isfinite(o->origin[1]) || !std::isfinite(o->origin[2]))
    return fail(GSDF_ERR_BAD_ARGUMENT, "simplify: the origin must be finite");
  if (o->flags != 0) return fail(GSDF_ERR_BAD_ARGUMENT, "simplify: unknown flags " + std::to_string(o->flags));
  if (!ix || (!out && !st)) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(ix->device));
  const int dev = ix->device;
  hipStream_t s = ix->stream;
  const bool dry = out == nullptr;
  const uint64_t V = ix->n_verts, F = ix->n_tris;
  const unsigned nb_v = blocks_of(V), nb_f = blocks_of(F);
  const char* nomem = "simplify: no device memory for the workspace";
  PoolBuf ctr, used, vcell, table, keep, fcell, blk_cnt, blk_base, total, cpos, first, vnum;
  if (!ctr.take(dev, sizeof(SimplifyCounters)) || !used.take(dev, V * 4) || !vcell.take(dev, V * 4)) return fail(GSDF_ERR_HIP, nomem);
  SimplifyCounters* d_ctr = ctr.as<SimplifyCounters>();
  EventPair ev_cells, ev_f;
  if (!ev_cells.make() || !ev_f.make()) return fail(GSDF_ERR_HIP, "hipEventCreate failed");
  // 1. used vertices, the exponent, and the cluster table: per cell the key (8 bytes), the label (4), the record (32), the flag (4);
  // cells from 2 V: the number of used vertices is known on the device only at this point, V bounds it (and so the clusters) from
  // above, and asking for 2 V instead of 2 x used saves the round trip that would fetch it
  HIP_TRY(hipEventRecord(ev_cells.a, s));
  HIP_TRY(hipMemsetAsync(d_ctr, 0, sizeof(SimplifyCounters), s));
  HIP_TRY(hipMemsetAsync(used.p, 0, V * 4, s));
  LAUNCH(simplify_mark_kernel, nb_f, BLOCK, s, ix->idx.as<unsigned>(), (unsigned long long)F, used.as<unsigned>(), &d_ctr->head);
  LAUNCH(topo_maxbits_kernel, grid_for(3 * V, ix->num_cu, 8), BLOCK, s, ix->verts.p, (unsigned long long)(3 * V), &d_ctr->head.maxbits);
  TableRunOf<SimplifyHead> run;
  auto tab_key = [&](uint64_t cells) { (void)cells; return table.as<unsigned long long>(); };
  auto tab_label = [&](uint64_t cells) { return (unsigned*)((uint8_t*)table.p + cells * 8); };
  auto tab_acc = [&](uint64_t cells) { return (SimplifyCell*)((uint8_t*)table.p + cells * 12); };
  auto tab_flag = [&](uint64_t cells) { return (unsigned*)((uint8_t*)table.p + cells * 44); };
  if (int rc = table_build("simplify", "GSDF_HIP_SIMPLIFY_CELLS_MIN", 2 * V, 48, dev, s, table, &d_ctr->head, [&](uint64_t cells) -> int {
        HIP_TRY(hipMemsetAsync(table.p, 0xff, cells * 12, s));
        HIP_TRY(hipMemsetAsync((uint8_t*)table.p + cells * 12, 0, cells * 36, s));
        HIP_TRY(hipMemsetAsync(&d_ctr->head, 0, SIMPLIFY_HEAD_RESET_BYTES, s));
        LAUNCH(simplify_insert_kernel, grid_for(V, ix->num_cu, 16), BLOCK, s, ix->verts.p, used.as<unsigned>(), (unsigned long long)V, (double)o->origin[0],
               (double)o->origin[1], (double)o->origin[2], (double)o->cell, tab_key(cells), tab_label(cells), (unsigned)(cells - 1), vcell.as<unsigned>(),
               &d_ctr->head);
        return GSDF_OK;
      }, &run))
    return rc;
  const SimplifyHead& hd = run.head;
  if (hd.nonfinite)
    return fail(GSDF_ERR_BAD_ARGUMENT, "simplify: " + std::to_string(hd.nonfinite) + " used vertices have a NaN or infinite coordinate");
  if (hd.out_of_range)
    return fail(GSDF_ERR_RESOLUTION, "simplify: the cell is too small for this mesh: vertex " + std::to_string(0xffffffffull - hd.first_bad) + " (and " +
                                         std::to_string(hd.out_of_range - 1) + " more) lies 2^19 cells or more from the origin");
  const uint64_t cells = run.cells;
  if (cells > ((uint64_t)1 << 31)) return fail(GSDF_ERR_CAPACITY, "simplify: hash table capacity exceeded");  // (a cell number is 32 bits, all ones = none)
  const int biased = (int)(hd.maxbits >> 23);
  const int e = (biased > 1 ? biased : 1) - 126;
  LAUNCH(simplify_sum_kernel, nb_v, BLOCK, s, ix->verts.p, vcell.as<unsigned>(), (unsigned long long)V, std::ldexp(1.0, 30 - e), tab_acc(cells));
  HIP_TRY(hipEventRecord(ev_cells.b, s));
  // 2. faces; the cells' positions. (The new handle's stream is made before the events: it is host work.)
  IndexedPtr nx;
  if (!dry)
    if (int rc = indexed_new(dev, ix->num_cu, &nx)) return rc;
  if (!blk_cnt.take(dev, (size_t)blocks_of(3 * F) * 4) || !blk_base.take(dev, (size_t)blocks_of(3 * F) * 4) ||
      (!dry && (!keep.take(dev, F) || !fcell.take(dev, 3 * F * 4) || !total.take(dev, 8) || !cpos.take(dev, cells * 12) || !first.take(dev, cells * 4) ||
                !vnum.take(dev, cells * 4))))
    return fail(GSDF_ERR_HIP, nomem);
  HIP_TRY(hipEventRecord(ev_f.a, s));
  LAUNCH(simplify_faces_kernel, nb_f, BLOCK, s, ix->idx.as<unsigned>(), (unsigned long long)F, vcell.as<unsigned>(), tab_flag(cells),
         dry ? nullptr : keep.as<unsigned char>(), dry ? nullptr : fcell.as<unsigned>(), blk_cnt.as<unsigned>());
  LAUNCH(block_scan_kernel, 1, 1024, s, blk_cnt.as<unsigned>(), nb_f, blk_base.as<unsigned>(), &d_ctr->tail.kept);
  LAUNCH(simplify_place_kernel, grid_for(cells, ix->num_cu, 8), BLOCK, s, tab_key(cells), tab_label(cells), tab_acc(cells), tab_flag(cells),
         (unsigned long long)cells, ix->verts.p, std::ldexp(1.0, e - 30), dry ? nullptr : cpos.p, &d_ctr->tail);
  SimplifyTail tl{};
  HIP_TRY(hipMemcpyAsync(&tl, &d_ctr->tail, sizeof tl, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const uint64_t F2 = tl.kept;
  if (hd.degenerate + F2 > F) return fail(GSDF_ERR_HIP, "simplify: internal error (the face counts do not add up)");
  uint64_t V2 = 0;
  if (!dry) {
    if (F2 == 0) return fail(GSDF_ERR_EMPTY_BUFFERS, "simplify: nothing kept (every face collapsed: the cell is too large for this mesh)");
    const uint64_t S2 = 3 * F2;
    const unsigned nb_s = blocks_of(S2);
    if (!nx->idx.take(dev, S2 * 4)) return fail(GSDF_ERR_HIP, nomem);
    // extract's kernels, the table's cell standing for the old vertex: kept faces in order, clusters by their smallest kept slot
    HIP_TRY(hipMemsetAsync(first.p, 0xff, cells * 4, s));
    LAUNCH(topo_compact_kernel, nb_f, BLOCK, s, fcell.as<unsigned>(), keep.as<unsigned char>(), (unsigned long long)F, blk_base.as<unsigned>(),
           nx->idx.as<unsigned>(), first.as<unsigned>());
    LAUNCH(topo_owner_kernel, nb_s, BLOCK, s, nx->idx.as<unsigned>(), (unsigned long long)S2, first.as<unsigned>(), blk_cnt.as<unsigned>());
    if (int rc = scan_blocks(s, blk_cnt, nb_s, blk_base, total, &V2)) return rc;
    if (V2 != tl.named) return fail(GSDF_ERR_HIP, "simplify: internal error (kept clusters)");
    if (!nx->verts.take(dev, V2 * 12) || !nx->vkeys.take(dev, V2 * 8)) return fail(GSDF_ERR_HIP, nomem);
    LAUNCH(topo_renumber_kernel, nb_s, BLOCK, s, nx->idx.as<unsigned>(), (unsigned long long)S2, first.as<unsigned>(), blk_base.as<unsigned>(), vnum.as<unsigned>(),
           cpos.as<unsigned>(), tab_key(cells), (const unsigned*)nullptr, nx->verts.as<unsigned>(), nx->vkeys.as<unsigned long long>(), (unsigned*)nullptr);
    LAUNCH(remap_kernel, nb_s, BLOCK, s, nx->idx.as<unsigned>(), (unsigned long long)S2, vnum.as<unsigned>());
  }
  HIP_TRY(hipEventRecord(ev_f.b, s));
  HIP_TRY(hipStreamSynchronize(s));
  const uint64_t n_collapsed = F - hd.degenerate - F2;
  gsdf_simplify_stats r{};
  r.n_verts_in = V; r.n_tris_in = F; r.used_verts_in = hd.used; r.degenerate_in = hd.degenerate; r.cells = hd.tab.distinct; r.collapsed = n_collapsed;
  r.n_verts = tl.named; r.n_tris = F2; r.largest_cell = tl.largest; r.exponent = e;
  r.ms_cells = ev_cells.ms(); r.ms_faces = ev_f.ms();
  r.probes = hd.tab.probes; r.table_cells = cells; r.attempts = run.attempts;
  if (st) *st = r;
  if (!dry) {
    nx->n_verts = V2;
    nx->n_tris = F2;
    nx->ms_device = r.ms_cells + r.ms_faces;
    *out = nx.release();
  }
  return GSDF_OK;
}

// ---- adaptive simplify (kernels_simplify_adaptive.h) ---------------------------------------------------------------------------------
extern "C" int gsdf_hip_indexed_simplify_adaptive(gsdf_indexed* ix, const gsdf_adaptive_opts* o, gsdf_indexed** out, gsdf_adaptive_stats* st) {
  if (out) *out = nullptr;
  if (!o) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (!(o->cell > 0.0f) || !std::isfinite(o->cell)) return fail(GSDF_ERR_BAD_ARGUMENT, "adaptive simplify: the cell edge must be positive and finite");
  if (!std::isfinite(o->origin[0]) || !std::isfinite(o->origin[1]) || !std::isfinite(o->origin[2]))
    return fail(GSDF_ERR_BAD_ARGUMENT, "adaptive simplify: the origin must be finite");
  if (!(o->tol >= 0.0f) || !std::isfinite(o->tol)) return fail(GSDF_ERR_BAD_ARGUMENT, "adaptive simplify: tol must be finite and not negative");
  if (o->levels < 1 || o->levels > ADAPTIVE_MAX_LEVELS) return fail(GSDF_ERR_BAD_ARGUMENT, "adaptive simplify: levels must be 1 .. 16");
  if (o->flags != 0) return fail(GSDF_ERR_BAD_ARGUMENT, "adaptive simplify: unknown flags " + std::to_string(o->flags));
  if (!ix || (!out && !st)) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(ix->device));
  const int dev = ix->device;
  hipStream_t s = ix->stream;
  const bool dry = out == nullptr;
  const uint64_t V = ix->n_verts, F = ix->n_tris;
  const unsigned levels = o->levels;
  const double tol = (double)o->tol;
  const unsigned nb_v = blocks_of(V), nb_f = blocks_of(F);
  const char* nomem = "adaptive simplify: no device memory for the workspace";
  PoolBuf ctr, used, vcell, vchoice, table, cpos, flag, keep, fcell, blk_cnt, blk_base, total, ukeys, first, vnum;
  if (!ctr.take(dev, sizeof(AdaptiveCounters)) || !used.take(dev, V * 4) || !vcell.take(dev, (size_t)levels * V * 4) || !vchoice.take(dev, V * 4))
    return fail(GSDF_ERR_HIP, nomem);
  AdaptiveCounters* d_ctr = ctr.as<AdaptiveCounters>();
  EventPair ev_cells, ev_e, ev_f;
  if (!ev_cells.make() || !ev_e.make() || !ev_f.make()) return fail(GSDF_ERR_HIP, "hipEventCreate failed");
  // 1. used vertices, the exponent, and ONE table for the cells of all levels: per cell the key (8 bytes), the label (4), the record
  // (32), the error (8). A surface has about a quarter of a level's cells at the next one, so 3 V cells ask for a load below 0.5
  // in nearly every case; where they do not, the table grows as every table here does.
  HIP_TRY(hipEventRecord(ev_cells.a, s));
  HIP_TRY(hipMemsetAsync(d_ctr, 0, sizeof(AdaptiveCounters), s));
  HIP_TRY(hipMemsetAsync(used.p, 0, V * 4, s));
  LAUNCH(simplify_mark_kernel, nb_f, BLOCK, s, ix->idx.as<unsigned>(), (unsigned long long)F, used.as<unsigned>(), &d_ctr->head);
  LAUNCH(topo_maxbits_kernel, grid_for(3 * V, ix->num_cu, 8), BLOCK, s, ix->verts.p, (unsigned long long)(3 * V), &d_ctr->head.maxbits);
  TableRunOf<SimplifyHead> run;
  auto tab_key = [&](uint64_t cells) { (void)cells; return table.as<unsigned long long>(); };
  auto tab_label = [&](uint64_t cells) { return (unsigned*)((uint8_t*)table.p + cells * 8); };
  auto tab_acc = [&](uint64_t cells) { return (SimplifyCell*)((uint8_t*)table.p + cells * 12); };
  auto tab_err = [&](uint64_t cells) { return (unsigned long long*)((uint8_t*)table.p + cells * 44); };
  if (int rc = table_build("adaptive simplify", "GSDF_HIP_SIMPLIFY_CELLS_MIN", (levels > 1 ? 3 : 2) * V, 52, dev, s, table, &d_ctr->head, [&](uint64_t cells) -> int {
        HIP_TRY(hipMemsetAsync(table.p, 0xff, cells * 12, s));
        HIP_TRY(hipMemsetAsync((uint8_t*)table.p + cells * 12, 0, cells * 40, s));
        HIP_TRY(hipMemsetAsync(&d_ctr->head, 0, SIMPLIFY_HEAD_RESET_BYTES, s));
        LAUNCH(adaptive_insert_kernel, grid_for(V, ix->num_cu, 16), BLOCK, s, ix->verts.p, used.as<unsigned>(), (unsigned long long)V, (double)o->origin[0],
               (double)o->origin[1], (double)o->origin[2], (double)o->cell, levels, tab_key(cells), tab_label(cells), (unsigned)(cells - 1),
               vcell.as<unsigned>(), &d_ctr->head);
        return GSDF_OK;
      }, &run))
    return rc;
  const SimplifyHead& hd = run.head;
  if (hd.nonfinite)
    return fail(GSDF_ERR_BAD_ARGUMENT, "adaptive simplify: " + std::to_string(hd.nonfinite) + " used vertices have a NaN or infinite coordinate");
  if (hd.out_of_range)
    return fail(GSDF_ERR_RESOLUTION, "adaptive simplify: the cell is too small for this mesh: vertex " + std::to_string(0xffffffffull - hd.first_bad) + " (and " +
                                         std::to_string(hd.out_of_range - 1) + " more) lies 2^17 cells or more from the origin");
  const uint64_t cells = run.cells;
  const uint64_t ids = cells + V;  // cluster numbers: a table cell, or cells + v for a vertex that stays alone
  if (cells > ((uint64_t)1 << 31) || ids >= 0xffffffffull) return fail(GSDF_ERR_CAPACITY, "adaptive simplify: hash table capacity exceeded");
  const int biased = (int)(hd.maxbits >> 23);
  const int e = (biased > 1 ? biased : 1) - 126;
  if (!cpos.take(dev, ids * 12) || !flag.take(dev, ids * 4)) return fail(GSDF_ERR_HIP, nomem);
  LAUNCH(adaptive_sum_kernel, nb_v, BLOCK, s, ix->verts.p, vcell.as<unsigned>(), (unsigned long long)V, levels, std::ldexp(1.0, 30 - e), tab_acc(cells));
  LAUNCH(adaptive_place_kernel, grid_for(cells, ix->num_cu, 8), BLOCK, s, tab_key(cells), tab_label(cells), tab_acc(cells), (unsigned long long)cells, ix->verts.p,
         std::ldexp(1.0, e - 30), cpos.p);
  HIP_TRY(hipEventRecord(ev_cells.b, s));
  // 2. the cells' errors, and every vertex's choice
  HIP_TRY(hipEventRecord(ev_e.a, s));
  LAUNCH(adaptive_error_kernel, nb_f, BLOCK, s, ix->verts.p, ix->idx.as<unsigned>(), (unsigned long long)F, vcell.as<unsigned>(), (unsigned long long)V, levels,
         cpos.p, tab_err(cells), tol);
  LAUNCH(adaptive_choose_kernel, nb_v, BLOCK, s, vcell.as<unsigned>(), (unsigned long long)V, levels, tab_label(cells), tab_acc(cells), tab_err(cells), tol,
         (unsigned)cells, vchoice.as<unsigned>(), &d_ctr->tail);
  HIP_TRY(hipEventRecord(ev_e.b, s));
  // 3. faces, as the uniform simplifier's with the choice where it has the cell. (The new handle's stream is made before the events.)
  IndexedPtr nx;
  if (!dry)
    if (int rc = indexed_new(dev, ix->num_cu, &nx)) return rc;
  if (!blk_cnt.take(dev, (size_t)blocks_of(3 * F) * 4) || !blk_base.take(dev, (size_t)blocks_of(3 * F) * 4) ||
      (!dry && (!keep.take(dev, F) || !fcell.take(dev, 3 * F * 4) || !total.take(dev, 8) || !ukeys.take(dev, ids * 8) || !first.take(dev, ids * 4) ||
                !vnum.take(dev, ids * 4))))
    return fail(GSDF_ERR_HIP, nomem);
  HIP_TRY(hipEventRecord(ev_f.a, s));
  HIP_TRY(hipMemsetAsync(flag.p, 0, ids * 4, s));
  LAUNCH(simplify_faces_kernel, nb_f, BLOCK, s, ix->idx.as<unsigned>(), (unsigned long long)F, vchoice.as<unsigned>(), flag.as<unsigned>(),
         dry ? nullptr : keep.as<unsigned char>(), dry ? nullptr : fcell.as<unsigned>(), blk_cnt.as<unsigned>());
  LAUNCH(block_scan_kernel, 1, 1024, s, blk_cnt.as<unsigned>(), nb_f, blk_base.as<unsigned>(), &d_ctr->tail.kept);
  LAUNCH(adaptive_named_kernel, grid_for(ids, ix->num_cu, 8), BLOCK, s, flag.as<unsigned>(), (unsigned long long)ids, &d_ctr->tail);
  AdaptiveTail tl{};
  HIP_TRY(hipMemcpyAsync(&tl, &d_ctr->tail, sizeof tl, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const uint64_t F2 = tl.kept;
  if (hd.degenerate + F2 > F) return fail(GSDF_ERR_HIP, "adaptive simplify: internal error (the face counts do not add up)");
  uint64_t V2 = 0;
  if (!dry) {
    if (F2 == 0) return fail(GSDF_ERR_EMPTY_BUFFERS, "adaptive simplify: nothing kept (every face collapsed: cell, tol and levels are too large for this mesh)");
    const uint64_t S2 = 3 * F2;
    const unsigned nb_s = blocks_of(S2);
    if (!nx->idx.take(dev, S2 * 4)) return fail(GSDF_ERR_HIP, nomem);
    // positions and keys by cluster number: the cells', then the input's own for the vertices that stay alone
    HIP_TRY(hipMemcpyAsync(cpos.p + 3 * cells, ix->verts.p, V * 12, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(ukeys.p, tab_key(cells), cells * 8, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(ukeys.as<unsigned long long>() + cells, ix->vkeys.p, V * 8, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemsetAsync(first.p, 0xff, ids * 4, s));
    LAUNCH(topo_compact_kernel, nb_f, BLOCK, s, fcell.as<unsigned>(), keep.as<unsigned char>(), (unsigned long long)F, blk_base.as<unsigned>(),
           nx->idx.as<unsigned>(), first.as<unsigned>());
    LAUNCH(topo_owner_kernel, nb_s, BLOCK, s, nx->idx.as<unsigned>(), (unsigned long long)S2, first.as<unsigned>(), blk_cnt.as<unsigned>());
    if (int rc = scan_blocks(s, blk_cnt, nb_s, blk_base, total, &V2)) return rc;
    if (V2 != tl.named) return fail(GSDF_ERR_HIP, "adaptive simplify: internal error (kept clusters)");
    if (!nx->verts.take(dev, V2 * 12) || !nx->vkeys.take(dev, V2 * 8)) return fail(GSDF_ERR_HIP, nomem);
    LAUNCH(topo_renumber_kernel, nb_s, BLOCK, s, nx->idx.as<unsigned>(), (unsigned long long)S2, first.as<unsigned>(), blk_base.as<unsigned>(), vnum.as<unsigned>(),
           cpos.as<unsigned>(), ukeys.as<unsigned long long>(), (const unsigned*)nullptr, nx->verts.as<unsigned>(), nx->vkeys.as<unsigned long long>(),
           (unsigned*)nullptr);
    LAUNCH(remap_kernel, nb_s, BLOCK, s, nx->idx.as<unsigned>(), (unsigned long long)S2, vnum.as<unsigned>());
  }
  HIP_TRY(hipEventRecord(ev_f.b, s));
  HIP_TRY(hipStreamSynchronize(s));
  gsdf_adaptive_stats r{};
  r.n_verts_in = V; r.n_tris_in = F; r.used_verts_in = hd.used; r.degenerate_in = hd.degenerate; r.cells = hd.tab.distinct;
  for (int l = 0; l < ADAPTIVE_MAX_LEVELS; l++) r.chosen[l] = tl.chosen[l];
  r.singles = tl.singles; r.collapsed = F - hd.degenerate - F2;
  r.n_verts = tl.named; r.n_tris = F2; r.largest_cluster = tl.largest;
  std::memcpy(&r.max_err, &tl.max_err, 8);
  r.exponent = e;
  r.ms_cells = ev_cells.ms(); r.ms_error = ev_e.ms(); r.ms_faces = ev_f.ms();
  r.probes = hd.tab.probes; r.table_cells = cells; r.attempts = run.attempts;
  if (st) *st = r;
  if (!dry) {
    nx->n_verts = V2;
    nx->n_tris = F2;
    nx->ms_device = r.ms_cells + r.ms_error + r.ms_faces;
    *out = nx.release();
  }
  return GSDF_OK;
}

// ---- clean (kernels_clean.h) -----------------------------------------------------------------------------------------------------------
extern "C" int gsdf_hip_indexed_clean(gsdf_indexed* ix, const gsdf_clean_opts* o, gsdf_indexed** out, gsdf_clean_stats* st) {
  if (out) *out = nullptr;
  if (!o) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (o->flags == 0) return fail(GSDF_ERR_BAD_ARGUMENT, "clean: no flags: nothing to do");
  if (o->flags & ~(GSDF_CLEAN_MERGE_POSITIONS | GSDF_CLEAN_FACES)) return fail(GSDF_ERR_BAD_ARGUMENT, "clean: unknown flags " + std::to_string(o->flags));
  if (o->reserved[0] != 0 || o->reserved[1] != 0 || o->reserved[2] != 0) return fail(GSDF_ERR_BAD_ARGUMENT, "clean: the reserved words must be 0");
  if (!ix || (!out && !st)) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  HIP_TRY(hipSetDevice(ix->device));
  const int dev = ix->device;
  hipStream_t s = ix->stream;
  const bool dry = out == nullptr, merge = (o->flags & GSDF_CLEAN_MERGE_POSITIONS) != 0, faces = (o->flags & GSDF_CLEAN_FACES) != 0;
  const uint64_t V = ix->n_verts, F = ix->n_tris, S = 3 * F;
  const unsigned nb_f = blocks_of(F), nb_s = blocks_of(S);
  const char* nomem = "clean: no device memory for the workspace";
  const char* floor_env = "GSDF_HIP_CLEAN_CELLS_MIN";
  PoolBuf ctr, vtab, vcls, midx, ftab, fcell, named, keep, blk_cnt, blk_base, total, first, vnum;
  if (!ctr.take(dev, sizeof(CleanCounters)) || !named.take(dev, V * 4) || !blk_cnt.take(dev, (size_t)nb_s * 4) || !blk_base.take(dev, (size_t)nb_s * 4))
    return fail(GSDF_ERR_HIP, nomem);
  CleanCounters* d_ctr = ctr.as<CleanCounters>();
  EventPair ev_m, ev_f, ev_r;
  if (!ev_m.make() || !ev_f.make() || !ev_r.make()) return fail(GSDF_ERR_HIP, "hipEventCreate failed");
  HIP_TRY(hipMemsetAsync(d_ctr, 0, sizeof(CleanCounters), s));
  // 1. the vertex table: 4 bytes per cell (the representative), cells from 2 V (at most V classes); every vertex's class; the faces
  // over classes, in a copy (the handle's own faces stay as they are)
  const unsigned* d_idx = ix->idx.as<unsigned>();
  TableRun vrun, frun;
  HIP_TRY(hipEventRecord(ev_m.a, s));
  if (merge) {
    if (!vcls.take(dev, V * 4) || !midx.take(dev, S * 4)) return fail(GSDF_ERR_HIP, nomem);
    if (int rc = table_build("clean", floor_env, 2 * V, 4, dev, s, vtab, &d_ctr->vtab, [&](uint64_t cells) -> int {
          HIP_TRY(hipMemsetAsync(vtab.p, 0xff, cells * 4, s));
          HIP_TRY(hipMemsetAsync(&d_ctr->vtab, 0, sizeof(TableCounters), s));
          LAUNCH(clean_vert_insert_kernel, grid_for(V, ix->num_cu, 16), BLOCK, s, ix->verts.as<unsigned>(), (unsigned long long)V, vtab.as<unsigned>(),
                 (unsigned)(cells - 1), vcls.as<unsigned>(), &d_ctr->vtab);
          return GSDF_OK;
        }, &vrun))
      return rc;
    if (vrun.cells > ((uint64_t)1 << 31)) return fail(GSDF_ERR_CAPACITY, "clean: hash table capacity exceeded");  // (a cell number is 32 bits, all ones = none)
    LAUNCH(clean_vert_class_kernel, grid_for(V, ix->num_cu, 16), BLOCK, s, vtab.as<unsigned>(), (unsigned long long)V, vcls.as<unsigned>(), d_ctr);
    HIP_TRY(hipMemcpyAsync(midx.p, ix->idx.p, S * 4, hipMemcpyDeviceToDevice, s));
    LAUNCH(remap_kernel, nb_s, BLOCK, s, midx.as<unsigned>(), (unsigned long long)S, vcls.as<unsigned>());
    d_idx = midx.as<unsigned>();
  }
  HIP_TRY(hipEventRecord(ev_m.b, s));
  // 2. the face table: per cell the representative (4 bytes), the two orientations' smallest faces (8) and counts (8); cells from
  // 2 F (at most F sets). Then the rule. (The new handle's stream is made before the events: it is host work.)
  IndexedPtr nx;
  if (!dry)
    if (int rc = indexed_new(dev, ix->num_cu, &nx)) return rc;
  if (!dry && (!keep.take(dev, F) || !total.take(dev, 8) || !first.take(dev, V * 4) || !vnum.take(dev, V * 4))) return fail(GSDF_ERR_HIP, nomem);
  auto tab_min = [&](uint64_t cells) { return (unsigned*)((uint8_t*)ftab.p + cells * 4); };
  auto tab_cnt = [&](uint64_t cells) { return (unsigned*)((uint8_t*)ftab.p + cells * 12); };
  HIP_TRY(hipEventRecord(ev_f.a, s));
  if (faces) {
    if (!fcell.take(dev, F * 4)) return fail(GSDF_ERR_HIP, nomem);
    if (int rc = table_build("clean", floor_env, 2 * F, 20, dev, s, ftab, &d_ctr->ftab, [&](uint64_t cells) -> int {
          HIP_TRY(hipMemsetAsync(ftab.p, 0xff, cells * 12, s));
          HIP_TRY(hipMemsetAsync(tab_cnt(cells), 0, cells * 8, s));
          HIP_TRY(hipMemsetAsync(&d_ctr->ftab, 0, sizeof(TableCounters), s));
          LAUNCH(clean_face_insert_kernel, nb_f, BLOCK, s, d_idx, (unsigned long long)F, ftab.as<unsigned>(), tab_min(cells), tab_cnt(cells), (unsigned)(cells - 1),
                 fcell.as<unsigned>(), &d_ctr->ftab);
          return GSDF_OK;
        }, &frun))
      return rc;
    if (frun.cells > ((uint64_t)1 << 31)) return fail(GSDF_ERR_CAPACITY, "clean: hash table capacity exceeded");
  }
  HIP_TRY(hipMemsetAsync(named.p, 0, V * 4, s));
  LAUNCH(clean_decide_kernel, nb_f, BLOCK, s, d_idx, (unsigned long long)F, faces ? ftab.as<unsigned>() : nullptr, faces ? tab_min(frun.cells) : nullptr,
         faces ? tab_cnt(frun.cells) : nullptr, faces ? fcell.as<unsigned>() : nullptr, named.as<unsigned>(), dry ? nullptr : keep.as<unsigned char>(),
         blk_cnt.as<unsigned>(), d_ctr);
  LAUNCH(block_scan_kernel, 1, 1024, s, blk_cnt.as<unsigned>(), nb_f, blk_base.as<unsigned>(), &d_ctr->kept);
  LAUNCH(clean_named_kernel, grid_for(V, ix->num_cu, 8), BLOCK, s, named.as<unsigned>(), (unsigned long long)V, d_ctr);
  HIP_TRY(hipEventRecord(ev_f.b, s));
  CleanCounters hc{};
  HIP_TRY(hipMemcpyAsync(&hc, d_ctr, sizeof hc, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const uint64_t F2 = hc.kept;
  if (hc.degenerate + hc.duplicate + hc.opposite + F2 != F || (faces && hc.face_sets != hc.ftab.distinct) || (merge && hc.merged >= V))
    return fail(GSDF_ERR_HIP, "clean: internal error (the counts do not add up)");
  // 3. extract's kernels over the classes: kept faces in order, classes by their smallest kept slot, the smallest member's data
  uint64_t V2 = 0;
  if (!dry) {
    if (F2 == 0) return fail(GSDF_ERR_EMPTY_BUFFERS, "clean: nothing kept (every face is degenerate or cancels against an opposite one)");
    const uint64_t S2 = 3 * F2;
    const unsigned nb_s2 = blocks_of(S2);
    if (!nx->idx.take(dev, S2 * 4)) return fail(GSDF_ERR_HIP, nomem);
    HIP_TRY(hipEventRecord(ev_r.a, s));
    HIP_TRY(hipMemsetAsync(first.p, 0xff, V * 4, s));
    LAUNCH(topo_compact_kernel, nb_f, BLOCK, s, d_idx, keep.as<unsigned char>(), (unsigned long long)F, blk_base.as<unsigned>(), nx->idx.as<unsigned>(),
           first.as<unsigned>());
    LAUNCH(topo_owner_kernel, nb_s2, BLOCK, s, nx->idx.as<unsigned>(), (unsigned long long)S2, first.as<unsigned>(), blk_cnt.as<unsigned>());
    if (int rc = scan_blocks(s, blk_cnt, nb_s2, blk_base, total, &V2)) return rc;
    if (V2 != hc.named) return fail(GSDF_ERR_HIP, "clean: internal error (kept vertices)");
    if (!nx->verts.take(dev, V2 * 12) || !nx->vkeys.take(dev, V2 * 8) || (ix->has_normals && !nx->normals.take(dev, V2 * 12))) return fail(GSDF_ERR_HIP, nomem);
    LAUNCH(topo_renumber_kernel, nb_s2, BLOCK, s, nx->idx.as<unsigned>(), (unsigned long long)S2, first.as<unsigned>(), blk_base.as<unsigned>(), vnum.as<unsigned>(),
           ix->verts.as<unsigned>(), ix->vkeys.as<unsigned long long>(), ix->has_normals ? ix->normals.as<unsigned>() : nullptr, nx->verts.as<unsigned>(),
           nx->vkeys.as<unsigned long long>(), ix->has_normals ? nx->normals.as<unsigned>() : nullptr);
    LAUNCH(remap_kernel, nb_s2, BLOCK, s, nx->idx.as<unsigned>(), (unsigned long long)S2, vnum.as<unsigned>());
    HIP_TRY(hipEventRecord(ev_r.b, s));
    HIP_TRY(hipStreamSynchronize(s));
  }
  gsdf_clean_stats r{};
  r.n_verts_in = V; r.n_tris_in = F; r.merged_verts = hc.merged; r.degenerate = hc.degenerate; r.face_sets = hc.face_sets; r.cancelled_sets = hc.cancelled_sets;
  r.duplicate_faces = hc.duplicate; r.opposite_faces = hc.opposite; r.largest_set = hc.largest; r.n_verts = hc.named; r.n_tris = F2;
  r.ms_merge = ev_m.ms(); r.ms_faces = ev_f.ms(); r.ms_result = dry ? 0.0 : ev_r.ms();
  r.vert_probes = merge ? vrun.head.probes : 0; r.vert_table_cells = vrun.cells; r.vert_attempts = vrun.attempts;
  r.face_probes = faces ? frun.head.probes : 0; r.face_table_cells = frun.cells; r.face_attempts = frun.attempts;
  if (st) *st = r;
  if (!dry) {
    nx->n_verts = V2;
    nx->n_tris = F2;
    nx->has_normals = ix->has_normals;
    nx->ms_device = r.ms_merge + r.ms_faces + r.ms_result;
    *out = nx.release();
  }
  return GSDF_OK;
}

// ---- project onto the field (kernels_project.h; the launch is abi_eval.hip's project_dev) -----------------------------------------
extern "C" int gsdf_hip_indexed_project(gsdf_indexed* ix, gsdf_program* p, const gsdf_project_opts* o, gsdf_indexed** out, gsdf_project_stats* st) {
  if (out) *out = nullptr;
  if (!o) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (!std::isfinite(o->step) || !(o->step > 0.0f)) return fail(GSDF_ERR_BAD_ARGUMENT, "project: the step must be positive and finite");
  if (!std::isfinite(o->tol) || !(o->tol >= 0.0f)) return fail(GSDF_ERR_BAD_ARGUMENT, "project: tol must be finite and not negative");
  if (!std::isfinite(o->max_move) || !(o->max_move >= 0.0f)) return fail(GSDF_ERR_BAD_ARGUMENT, "project: max_move must be finite and not negative");
  if (o->max_iters < 0 || o->max_iters > 64) return fail(GSDF_ERR_BAD_ARGUMENT, "project: max_iters must be 0 .. 64");
  if (o->flags != 0) return fail(GSDF_ERR_BAD_ARGUMENT, "project: unknown flags " + std::to_string(o->flags));
  if (!ix || !p || (!out && !st)) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (p->prog.is2d) return fail(GSDF_ERR_DIMENSION, "project: the program is 2D");
  if (p->device != ix->device) return fail(GSDF_ERR_BAD_ARGUMENT, "the program and the indexed mesh live on different devices");
  HIP_TRY(hipSetDevice(ix->device));
  const int dev = ix->device;
  const uint64_t V = ix->n_verts, F = ix->n_tris;
  gsdf_project_stats r{};
  if (!out) {  // the dry run: the stats alone
    if (int rc = project_dev(p, ix->verts.p, (size_t)V, o, nullptr, nullptr, nullptr, nullptr, &r)) return rc;
    *st = r;
    return GSDF_OK;
  }
  IndexedPtr nx;
  if (int rc = indexed_new(dev, ix->num_cu, &nx)) return rc;
  if (!nx->verts.take(dev, V * 12) || !nx->idx.take(dev, F * 12) || !nx->vkeys.take(dev, V * 8) || !nx->fit_before.take(dev, V * 4) ||
      !nx->fit_after.take(dev, V * 4) || !nx->fit_status.take(dev, V))
    return fail(GSDF_ERR_HIP, "project: no device memory for the result");
  HIP_TRY(hipMemcpyAsync(nx->idx.p, ix->idx.p, F * 12, hipMemcpyDeviceToDevice, nx->stream));
  HIP_TRY(hipMemcpyAsync(nx->vkeys.p, ix->vkeys.p, V * 8, hipMemcpyDeviceToDevice, nx->stream));
  if (int rc = project_dev(p, ix->verts.p, (size_t)V, o, nx->verts.p, nx->fit_before.p, nx->fit_after.p, nx->fit_status.as<uint8_t>(), &r)) return rc;
  HIP_TRY(hipStreamSynchronize(nx->stream));
  nx->n_verts = V;
  nx->n_tris = F;
  nx->has_fit = true;
  nx->ms_device = r.ms_device;
  if (st) *st = r;
  *out = nx.release();
  return GSDF_OK;
}

// ---- wall thickness (kernels_ray.h; the launch is abi_eval.hip's ray_dev on the device-resident vertices) ---------------------------
extern "C" int gsdf_hip_indexed_thickness(gsdf_indexed* ix, gsdf_program* p, const gsdf_thickness_opts* o, float* thickness_out, uint8_t* status_out, gsdf_ray_stats* st) {
  if (!o) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (int rc = ray_opts_refused(&o->ray, "thickness")) return rc;
  if (!std::isfinite(o->step) || !(o->step > 0.0f)) return fail(GSDF_ERR_BAD_ARGUMENT, "thickness: the step must be positive and finite");
  if (o->reserved[0] != 0 || o->reserved[1] != 0) return fail(GSDF_ERR_BAD_ARGUMENT, "thickness: the reserved words must be 0");
  if (!ix || !p || (!thickness_out && !status_out && !st)) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (p->prog.is2d) return fail(GSDF_ERR_DIMENSION, "thickness: the program is 2D");
  if (p->device != ix->device) return fail(GSDF_ERR_BAD_ARGUMENT, "the program and the indexed mesh live on different devices");
  HIP_TRY(hipSetDevice(ix->device));
  const uint64_t V = ix->n_verts;
  DevPtr<float> d_t;
  DevPtr<uint8_t> d_s;
  if (thickness_out) HIP_TRY(hipMalloc((void**)&d_t.p, V * 4));
  if (status_out) HIP_TRY(hipMalloc((void**)&d_s.p, V));
  gsdf_ray_stats r{};
  if (int rc = ray_dev(p, ix->verts.p, (size_t)V, &o->ray, o->step, o->thin, d_t.p, nullptr, d_s.p, nullptr, &r)) return rc;
  if (thickness_out) HIP_TRY(hipMemcpy(thickness_out, d_t.p, V * 4, hipMemcpyDeviceToHost));
  if (status_out) HIP_TRY(hipMemcpy(status_out, d_s.p, V, hipMemcpyDeviceToHost));
  if (st) *st = r;
  return GSDF_OK;
}

extern "C" int gsdf_hip_indexed_read_fit(const gsdf_indexed* ix, float* dist_before, float* dist_after, uint8_t* status) {
  if (!ix) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (!ix->has_fit) return fail(GSDF_ERR_BAD_ARGUMENT, "no fit: the handle was not made by gsdf_hip_indexed_project");
  HIP_TRY(hipSetDevice(ix->device));
  if (dist_before) HIP_TRY(hipMemcpy(dist_before, ix->fit_before.p, ix->n_verts * 4, hipMemcpyDeviceToHost));
  if (dist_after) HIP_TRY(hipMemcpy(dist_after, ix->fit_after.p, ix->n_verts * 4, hipMemcpyDeviceToHost));
  if (status) HIP_TRY(hipMemcpy(status, ix->fit_status.p, ix->n_verts, hipMemcpyDeviceToHost));
  return GSDF_OK;
}
