// abi_host.h -- what the translation units of the C ABI share on the host side: error plumbing, the mesh handle, the buffer
// pools. No device code (abi_comm.cpp, abi_evalhost.cpp and abi_host.cpp are plain C++).
//   abi_host.cpp  error text, triangle / pinned-buffer pools, result copies
//   abi_eval.hip  programs, self-test hooks, gleval.SDF3 / SDF2 Evaluate, normals, projection, rays, image / view / picture renderers
//   abi_evalhost.cpp  the evaluator side without a GPU: lowering for inspection, orbit camera, picture size, colour conversions,
//                 block cache (over the public ABI of a program)
//   abi_spec.hip  per-tree (specialised) kernels of a program: first build, background build and adoption, the groups built on
//                 first use (spec_ensure), the report of what a handle launches. Host code only: it owns no kernel
//   abi_mesh.hip  octree / flat / dual-contouring meshers and the mesh accessors
//   abi_indexed.hip  indexed meshes: the gsdf_indexed handle, weld, PLY, report and extract
//   abi_contour.hip  2-D outlines and z-slices traced into ordered closed loops; the loops uploaded, simplified, measured, hatched,
//                 skin-classified and offset. One Job (stream, events, final wait) per call, one Tracer for every traced call
//   abi_mass.cpp  principal axes of an inertia tensor (host only; without a HIP header, so that a plain C++ program can link it)
//   abi_comm.cpp  multi-GPU: communicator (RCCL or the in-process loopback transport), gather plan, gatherv
// (the list the library is built from: UNITS in __graft_entry__.py)
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <string>

#pragma GCC visibility push(default)
#include "../../include/gsdf_hip.h"
#pragma GCC visibility pop

// ---------------------------------------------------------------------------------------------
// error plumbing
// ---------------------------------------------------------------------------------------------
int fail(int code, const std::string& msg);  // sets the calling thread's gsdf_hip_last_error text, returns code
#define HIP_TRY(expr)                                                                                   \
  do {                                                                                                  \
    hipError_t _e = (expr);                                                                             \
    if (_e != hipSuccess) return fail(GSDF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)
// the same inside a function that has a `bail(code)` to release what it holds on the way out
#define HIP_TRYM(expr)                                                                                        \
  do {                                                                                                        \
    hipError_t _e = (expr);                                                                                   \
    if (_e != hipSuccess) return bail(fail(GSDF_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e))); \
  } while (0)

// Environment knobs (tuning, developer A/B switches): a site that reads its knob once keeps the value in a `static const`.
inline int env_int(const char* name, int dflt) { const char* e = getenv(name); return e ? atoi(e) : dflt; }
inline uint64_t env_u64(const char* name, uint64_t dflt) { const char* e = getenv(name); return e ? (uint64_t)strtoull(e, nullptr, 10) : dflt; }
inline bool env_flag(const char* name) { const char* e = getenv(name); return e && atoi(e) != 0; }      // off unless set to non-zero
inline bool env_flag_on(const char* name) { const char* e = getenv(name); return !e || atoi(e) != 0; }  // on unless set to 0
inline bool env_set(const char* name) { return getenv(name) != nullptr; }

// The CU count a handle sizes its capped grids from (grid_for, num_cu * workgroups per CU): the device's, or GSDF_HIP_GRID_CUS where
// that is 1 .. the device's (read whenever a handle learns its count; handles made from a handle inherit). A developer knob:
// with few CUs every grid-stride loop takes several trips at sizes a test can afford. *real_out: the device's own count.
inline int grid_cus(int device, int* real_out = nullptr) {
  int real = 256;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0) real = prop.multiProcessorCount;
  if (real_out) *real_out = real;
  const int n = env_int("GSDF_HIP_GRID_CUS", 0);
  return n >= 1 && n < real ? n : real;
}

inline bool finite_all(const float* v, int n) {
  for (int i = 0; i < n; i++) if (!std::isfinite(v[i])) return false;
  return true;
}

struct gsdf_mesh {
  int device = 0;
  float* d_tris = nullptr;
  uint64_t cap = 0;
  gsdf_mesh_stats st{};
  hipStream_t stream = nullptr;   // the stream the mesher ran on (the program's or the caller's); the mesher has synchronised it
  hipStream_t rstream = nullptr;  // the mesh's OWN stream for later reads / STL builds: a mesh may outlive its program handle
  bool host_out = false;  // d_tris is pinned, device-mapped HOST memory (gsdf_mesh_opts.host_output): the kernels write across PCIe
  // pinned host copies handed out by gsdf_hip_mesh_host_tris / gsdf_hip_mesh_host_stl (owned by the mesh)
  void* h_tris = nullptr;
  size_t h_tris_cap = 0;
  void* h_stl = nullptr;
  size_t h_stl_cap = 0;
  // GSDF_PAYLOAD_RECORDS: the packed cut-leaf records (kernels_octree.h: dense_payload_bytes) instead of triangles, until
  // gsdf_hip_mesh_march / a gather turns them into triangles. d_recs comes from the triangle pool (capacity in 36-byte units).
  int payload = 0;
  uint8_t* d_recs = nullptr;
  uint64_t recs_cap36 = 0;
  uint64_t n_recs = 0;
  // A records mesh of the whole model (octree mesher, shard_count == 1) can be welded (gsdf_hip_mesh_weld), before or after
  // gsdf_hip_mesh_march: the march then parks the records here instead of releasing them, until the mesh is destroyed.
  bool weldable = false;
  uint8_t* d_wrecs = nullptr;
  uint64_t wrecs_cap36 = 0;
  uint64_t n_wrecs = 0;
  int num_cu = 256;
  // device time per stage, where a mesher records it (dual contouring: five stages; gsdf_hip_mesh_stage_ms)
  int n_stages = 0;
  double stage_ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  const char* stage_name[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  // A gather in flight reads this mesh's buffers on the communicator's stream (gsdf_hip_mesh_gatherv_start .. _wait): a
  // destroy in between is deferred to the gather's end instead of handing the buffers to the next mesh under it.
  // ONE count of references: the owner's (dropped by gsdf_hip_mesh_destroy) + one per gather in flight (dropped by
  // mesh_inflight_done); whoever drops the last one frees the mesh -- destroy and a gather's end may run on different threads, and
  // two separate flags let both of them free it.
  std::atomic<int> refs{1};
  std::atomic<int> inflight{0};  // gathers in flight (what gsdf_hip_mesh_march asks about); the lifetime is decided by refs
};
void mesh_inflight_done(gsdf_mesh* m);  // abi_mesh.hip: one gather fewer; destroys a mesh whose owner already let go

// Packed records of several ranks side by side in one device buffer (abi_mesh.hip; layout: kernels_octree.h DensePart).
struct gsdf_dense_part { uint64_t off, n_recs, tri0; };
constexpr int kDenseMaxParts = 64;
inline uint64_t dense_bytes(uint64_t n_recs) { return n_recs * 40ull + ((((n_recs + 255ull) / 256ull) * 4ull + 7ull) & ~7ull); }
// Marching cubes over them into d_tris (room for the parts' triangles: the last part's tri0 + its own), on stream s.
// d_parts: device scratch of at least dense_parts_bytes() that stays valid until the work on s has run.
size_t dense_parts_bytes();
void* dense_parts_at(float* d_tris, uint64_t n_tris);  // where the table goes behind n_tris triangles (8-byte aligned)
int mesh_march_dense(const uint8_t* d_buf, const gsdf_dense_part* parts, int nparts, void* d_parts, float ox, float oy, float oz, float res,
                     float* d_tris, int num_cu, hipStream_t s);

// The other direction (abi_indexed.hip, for gsdf_hip_mesh_dualcontour_indexed in abi_mesh.hip): dual contouring's quads in lattice
// order -> a finished gsdf_indexed handle. d_slot_cube: S = 3 F slots, each the index (< cube_cap: the CALLER has made sure) of the kept cube whose placed
// vertex d_fv[3 cube ..] that corner is; a buffer from the triangle pool of slot_cap36 36-byte units that the handle TAKES OVER as
// its index array (on an error it goes back to the pool). d_cubes: the kept cubes (device `Cube`, kernels_common.h), the vertices'
// keys. Runs on s and waits for it: d_fv and d_cubes may be overwritten afterwards. key_ev: two pairs of events
// recorded on s around the caller's ordering pass, whose device time becomes the handle's gsdf_indexed_stats.ms_keys.
int indexed_from_cube_slots(int device, int num_cu, hipStream_t s, float* d_slot_cube, uint64_t slot_cap36, uint64_t S, uint64_t cube_cap, const float* d_fv,
                            const void* d_cubes, const hipEvent_t key_ev[4], gsdf_indexed** out);
// kernels_weld.h's block_scan_kernel on s: cnt[n] -> base[n], exclusive; *d_total = their sum. (The kernel is abi_indexed.hip's.)
int launch_block_scan(const unsigned* d_cnt, unsigned n, unsigned* d_base, unsigned long long* d_total, hipStream_t s);

// Triangle buffers and pinned host buffers are recycled through small per-process pools (abi_host.cpp).
float* pool_take(int device, uint64_t need, uint64_t* cap_out);
void pool_give(int device, float* p, uint64_t cap);
// the ipc test transport: a transport of that kind exists / is gone; the allocation at `base` has been exported to a peer process
void pool_exporter_opened();
void pool_exporter_closed();
void pool_note_exported(void* base);
void* hpool_take(size_t need, size_t* cap_out);
void hpool_give(void* p, size_t cap);
void big_memcpy(void* dst, const void* src, size_t n);
int host_buf(void** buf, size_t* cap, size_t need);
hipStream_t mesh_stream(gsdf_mesh* m);
void release_tris(gsdf_mesh* m);
