// abi_program.h -- the program handle and the launch helpers of the translation units that own kernels (abi_eval.hip,
// abi_mesh.hip, abi_indexed.hip, abi_contour.hip) and of abi_spec.hip, which builds the handle's per-tree kernels. Include after
// kernels_common.h: the handle's LDS arithmetic uses its constants (BLOCK, ...).
// What the handle owns frees itself (Arena, Owned, EventSet, Stream, SpecKernels below): gsdf_hip_program_destroy is `delete`.
#pragma once
#include <condition_variable>
#include <mutex>
#include <thread>
#include <vector>

#include "abi_host.h"
#include "compile.h"
#include "launch_args.h"
#include "specialize.h"

// ---- owners of device resources: each frees what it holds, none can be copied, all are no-ops on null ---------------------------
struct NoCopy {
  NoCopy() = default;
  NoCopy(const NoCopy&) = delete;
  NoCopy& operator=(const NoCopy&) = delete;
};
// grow-only device memory, reused by every call on the handle
struct Arena : NoCopy {
  void* p = nullptr;
  size_t cap = 0;
  ~Arena() { release(); }
  hipError_t ensure(size_t bytes) {
    if (bytes <= cap) return hipSuccess;
    release();
    size_t want = bytes + bytes / 4 + 4096;
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};
// one allocation of exactly the size asked for: device memory (hipFree) or pinned host memory (hipHostFree)
template <typename T, hipError_t (*Free)(void*)>
struct Owned : NoCopy {
  T* p = nullptr;
  ~Owned() { reset(); }
  void reset() { if (p) (void)Free((void*)p); p = nullptr; }
};
template <typename T> using DevPtr = Owned<T, hipFree>;
template <typename T> using PinnedPtr = Owned<T, hipHostFree>;
template <int N>
struct EventSet : NoCopy {
  hipEvent_t e[N] = {};
  ~EventSet() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
  hipError_t ensure() {  // created at first use, kept
    for (hipEvent_t& x : e)
      if (!x) { hipError_t r = hipEventCreate(&x); if (r != hipSuccess) return r; }
    return hipSuccess;
  }
  hipEvent_t operator[](int i) const { return e[i]; }
};
struct Stream : NoCopy {
  hipStream_t s = nullptr;
  ~Stream() { if (s) (void)hipStreamDestroy(s); }
  hipError_t ensure() { return s ? hipSuccess : hipStreamCreateWithFlags(&s, hipStreamNonBlocking); }
};

// ---- kernel variants as data ----------------------------------------------------------------------------------------------------
// Which instantiation a launch site runs, and what it is called: the name expression the run-time compiler is handed
// (spec_name: "leaf_eval_kernel<4, 3, true, true, false, false>") and the short form gsdf_hip_program_kernels reports
// (short_name: "leaf_eval_kernel<4,3>"). Stored profiles and the tests compare both strings.
struct SweepVariant {  // eval_kernel<DIM, K, W> (dim = 2 | 3); flat_grid_kernel<K, W>, dc_origin_kernel<K, W> (dim = 0)
  int k, w;
  std::string spec_name(const char* base, int dim = 0) const { return std::string(base) + "<" + (dim ? std::to_string(dim) + ", " : "") + std::to_string(k) + ", " + std::to_string(w) + ">"; }
  std::string short_name(const char* base, int dim = 0) const { return std::string(base) + "<" + (dim ? std::to_string(dim) + "," : "") + std::to_string(k) + "," + std::to_string(w) + ">"; }
};
struct LeafVariant {  // leaf_eval_kernel<K, W, UCUBE, NTLDS, BOTH, DZ> (kernels_octree.h)
  int k, w;
  bool ucube, ntlds, both, dz;
  std::string spec_name() const {
    auto b = [](bool x) { return x ? ", true" : ", false"; };
    return "leaf_eval_kernel<" + std::to_string(k) + ", " + std::to_string(w) + b(ucube) + b(ntlds) + b(both) + b(dz) + ">";
  }
  std::string short_name() const {
    return "leaf_eval_kernel<" + std::to_string(k) + "," + std::to_string(w) + (both ? ",both" : "") + (dz ? ",rows" : "") + ">";
  }
};
struct LeafPick { LeafVariant v; hipFunction_t f; };  // f: the handle's per-tree build of v; null: the ahead-of-time kernel of v

// ---- everything a per-tree ("specialised") build of a handle has produced (abi_spec.hip) -----------------------------------------
// The groups of kernels a specialised handle builds the first time an entry point needs them (spec_ensure): the evaluating kernels of
// dual contouring, normals, the flat lattice pass and the 2-D image; distinct z rows (share_corners = 2; kernels_octree.h: DZ);
// eval_kernel<D, 1, 4> for host-mapped calls; distinct lattice points (share_corners = 1: leaf_dense_kernel); the UI's view
// (kernels_view.h); the projection of mesh vertices (kernels_project.h); the 2-D picture, one kernel per conversion kind (kernels_image.h);
// rays and wall thickness (kernels_ray.h).
enum SpecGroup { SPEC_AUX, SPEC_ROWS, SPEC_EVAL_K1, SPEC_DENSE, SPEC_VIEW, SPEC_PROJECT, SPEC_PICTURE, SPEC_RAY, SPEC_GROUPS };
struct SpecBuilt {  // what was built, for which template arguments, by what
  std::vector<hipModule_t> mods;  // the first group's module, then every later one (a kernel rebuilt for another W, the groups above)
  int eval_k = 0, eval_w = 0, leaf_k = 0, leaf_w = 0, rows_w = 0, dense_w = 0;
  bool leaf_both = false, rows_both = false;  // both column passes in one body (kernels_octree.h: BOTH)
  std::string compiler, key;  // hipcc | hiprtc | cache; key of the first group's build (specialize.cpp: build_key)
  double compile_s = 0;
};
struct SpecFns {  // null: the ahead-of-time (interpreter) kernel runs
  hipFunction_t f_eval = nullptr, f_eval_k1 = nullptr, f_prune = nullptr, f_prune_spec = nullptr, f_leaf = nullptr, f_leaf_dz = nullptr, f_leaf_dense = nullptr;
  hipFunction_t f_dc_block_test = nullptr, f_dc_origin = nullptr, f_dc_edges = nullptr, f_dc_normals = nullptr, f_normals = nullptr, f_image = nullptr, f_flat_grid = nullptr;
  hipFunction_t f_view = nullptr, f_view_plain = nullptr, f_project = nullptr, f_imgc[4] = {nullptr, nullptr, nullptr, nullptr};
  hipFunction_t f_ray = nullptr, f_ray_thick = nullptr;
};
struct SpecKernels : SpecBuilt, SpecFns, NoCopy {
  std::atomic<unsigned> todo{0};  // bit g: group g is still to be tried. 0 on a handle that is not specialised: spec_ensure's lock-free exit
  ~SpecKernels() { for (hipModule_t m : mods) (void)hipModuleUnload(m); }
  bool specialised() const { return !mods.empty(); }
  // Everything `from` built becomes this one's, whatever members the structs above have: the configuration before the functions (a
  // reader that sees a function sees what it was built for), the groups to build last. What this one held goes away with `from`,
  // except the seconds it spent compiling.
  void take(SpecKernels& from) {
    std::swap(static_cast<SpecBuilt&>(*this), static_cast<SpecBuilt&>(from));
    compile_s += from.compile_s;
    std::atomic_thread_fence(std::memory_order_release);
    static_cast<SpecFns&>(*this) = from;
    todo.store(from.todo.load(), std::memory_order_release);
  }
};

struct gsdf_program {
  gsdf_dev::Program prog;
  int device = 0;
  Stream stream;  // (declared ahead of everything that ran on it: destroyed last)
  // Workspace of one octree mesh in flight, grow-only, reused by every gsdf_hip_mesh_octree call that gets the slot. Slot 0 runs on
  // the handle's stream, slots 1 and 2 on streams of their own (created on first use): gsdf_hip_mesh_octree_start.
  // Three chains: measured at npt-flange resdiv 1600 with one, two, three, four and six meshes in flight (tools/gpu_pipe_depth.py,
  // round 6): 0.452, 0.365-0.369, 0.340, 0.374, 0.358 ms per mesh -- a third chain fills what two leave idle around the evaluating
  // kernel (the five dependent launches of the centre tests, the marching kernel's latency-bound passes), a fourth only adds contention.
  struct OctreeWs {
    Stream own;
    Arena q0, q1;     // the two cube queues the descent alternates between
    Arena ctr;        // MeshCounters, then the group sums of the two-kernel leaf phase (one clear covers both)
    Arena spec_pass;  // the speculative top: pass bytes, statistics rows, brick masks
    Arena rec, hdr;   // cut-leaf records and block headers of the two-kernel leaf phase
    Arena grp;        // payload = records: scanned group sums
    EventSet<5> ev;   // chain start, descent done, leaf phase done, evaluating kernel done, counters on the host
    bool job_busy = false;
    hipStream_t job_stream = nullptr;
  };
  static constexpr int kJobs = 3;
  OctreeWs ws[kJobs];  // dual contouring and the flat renderer use ws[0].q0, .ctr and .ev too (they refuse to run beside an octree mesh)
  bool mesh_in_flight() const { for (const OctreeWs& w : ws) if (w.job_busy) return true; return false; }
  DevPtr<uint32_t> d_code;
  std::atomic<uint64_t> evals{0};  // (atomic: host-buffer calls of several threads and a mesher may count at the same time)
  // staging for the host-buffer API
  DevPtr<void> d_pos;
  DevPtr<float> d_dist;
  size_t cap_pos_bytes = 0, cap_dist = 0;
  // Staging slots of the host-buffer API: pinned, device-mapped position / distance buffers with a stream each, so that
  // several host threads (glrender.FlatRenderer evaluates from numParallel goroutines, flatrenderer.go:120-129) -- or one
  // caller pipelining gsdf_hip_eval3_submit / gsdf_hip_eval_wait -- have calls in flight at the same time.
  struct Slot : NoCopy {
    Stream s;
    PinnedPtr<void> h_pos;
    PinnedPtr<float> h_dist;
    bool busy = false, waiting = false;
    unsigned gen = 0;  // bumped at every acquisition; a ticket is slot | gen << 8, so a stale or repeated wait is refused instead of releasing somebody else's call
    float* user_dist = nullptr;
    size_t n = 0;
    bool zero_copy = false;
    PinnedPtr<unsigned> h_flag;
    unsigned* d_flag = nullptr;
    unsigned flag_val = 0;
    bool flagged = false;
  };
  // h_flag / d_flag: a word of pinned, device-mapped memory the stream writes flag_val into behind the kernel (completion by
  // polling: a blocking call of 4 096 points is 26 us through hipStreamSynchronize, of which the kernel is a few)
  static constexpr int kSlots = 4;
  Slot slot[kSlots];
  std::mutex slot_mu;
  std::condition_variable slot_cv;
  std::atomic<uint64_t> evals_host{0};
  int num_cu = 256;
  // dual contouring workspace (index grid: 4 B per lattice cell)
  Arena dc_tile, dc_grid, dc_dist, dc_fv, dc_nrm, dc_edge, dc_erun, dc_flag;
  Arena dc_ix, dc_ix_sort;  // its indexed quad stage (kernels_dc_indexed.h)
  EventSet<4> dc_ev;        // its stage marks: origin sweep, edges, normals, placement done
  Arena flat_grid;          // FlatRenderer distances
  Arena flat_bits;          // sign and near-surface bit planes of the flat renderer's lattice (flat_grid_kernel -> flat_cut_scan_kernel)
  Arena flat_list;          // the cut cubes (-> flat_march_list_kernel)
  PinnedPtr<void> h_ctr;  // pinned host copy of the device counters (a pageable destination makes the D2H copy a staged, blocking one)
  uint64_t last_tris = 0;  // triangle count of the previous mesh on this handle: sizes the next output buffer
  uint64_t last_recs = 0;  // cut leaves of the previous mesh with payload = records: sizes the next payload buffer
  uint64_t rec_blocks = 0;  // 64-leaf blocks the cut-leaf record arena is sized for (0: first mesh, start with kRecBlocks0)
  uint64_t last_dc_cubes = 0;  // kept cubes of the previous dual contouring pass: sizes the next queues
  // run-time specialised kernels for this program (gsdf_hip_program_specialize): per-tree modules, else the interpreter's kernels.
  // Written under spec_async_mu by adoption and by spec_ensure; the host-buffer calls, which may run on several threads, read their
  // kernels under it too (abi_eval.hip: eval_dev). Every other reader relies on the one-caller-at-a-time rule of gsdf_hip.h.
  SpecKernels spec;
  size_t lds_dense() const { return (size_t)(prog.nslots * 4 > 8 ? prog.nslots * 4 : 8) * BLOCK * sizeof(float) + 256 + 4 * 512 * sizeof(float) + 4 * 24 * sizeof(float) + 16; }
  // A kernel's counters on the device and the two events around its launch: made at the first launch of the kind, kept for the
  // next (abi_eval.hip: counted_launch). One per kind: the projection (project_dev); rays and wall thickness (ray_dev).
  struct CountedLaunch { DevPtr<void> ctr; EventSet<2> ev; };
  CountedLaunch proj, ray;
  // Specialisation in the background (gsdf_hip_program_specialize_async): a thread builds and loads the kernels on a shadow handle
  // (this program, this device, nothing else) while the interpreter kernels serve; the entry points adopt the result at their
  // next call (abi_spec.hip: spec_adopt). 0 idle | 1 building | 2 built, to be adopted | 3 failed (spec_async_err)
  std::atomic<int> spec_async{0};
  std::thread spec_thread;
  gsdf_program* spec_shadow = nullptr;
  std::mutex spec_async_mu;
  std::string spec_async_err;
  // A build under way finishes first (its thread writes into this handle), then the shadow handle goes; the members free
  // themselves in reverse order of declaration: modules (spec), events, device and pinned memory, the streams last.
  ~gsdf_program() {
    if (spec_thread.joinable()) spec_thread.join();
    delete spec_shadow;
  }
  // leaf kernel batching: K = 4 while 3 workgroups still fit the CU's LDS (<= 11 slots); 12..15 slots run K = 2 at 4
  // waves/SIMD instead of K = 4 at 2 (knurled-cylinder: 23.3 vs 23.8 ms). A 4th wave per SIMD is worth more than the
  // ~30 VGPRs it costs (flange 3.28 -> 2.95 ms), but only if 4 workgroups fit the CU's 160 KB of LDS.
  struct LeafConfig { int k, w; size_t lds; bool ntlds; };
  LeafConfig leaf_config() const {
    static const int forced_w = env_int("GSDF_HIP_LEAF_WAVES", 0);  // tuning knob
    const int ns = prog.nslots > 0 ? prog.nslots : 1;
    const int lk = (batch_k() == 4 && ns > 11) ? 2 : batch_k();
    // The evaluating kernel needs the interpreter's columns only (8 rows at least: a brick's distances) + the 256-byte
    // triangles-per-case table, unless it is exactly that table which would cost the fourth workgroup per CU (40 rows = 40 KB): the
    // kernel then reads the counts from the table in global memory.
    const size_t rows_e = (size_t)(ns * lk > 8 ? ns * lk : 8) * BLOCK * sizeof(float);
    const bool ntlds = !(4 * rows_e <= kLdsPerCu && 4 * (rows_e + 256) > kLdsPerCu);
    const size_t lds = rows_e + (ntlds ? 256 : 0);
    int w = forced_w ? forced_w : (4 * lds <= kLdsPerCu ? 4 : 3);
    if (lk == 4) { if (w != 2 && w != 4 && !(w == 5 && 5 * lds <= kLdsPerCu)) w = 3; }
    else if (lk == 2) { if (w != 4) w = 3; }
    else w = 4;
    return {lk, w, lds, ntlds};
  }
  // Ahead-of-time (interpreter) leaf kernels exist only at occupancies the compiler reaches WITHOUT scratch
  // (tests/test_kernel_resources.py reads the shipped code object): at 4 workgroups per CU (128 VGPRs) the K = 4 and
  // K = 2 interpreter builds spill, and a spilling build is not trusted (see fn_scratch_bytes).
  static int leaf_aot_waves(int k, int w) { return k == 4 ? (w == 2 ? 2 : 3) : (k == 2 ? 3 : 4); }
  // What the leaf phase of a mesh launches whose last level of cubes is lq (3 for meshes of three levels or more: a wave pass is one
  // level-3 cube -- column bricks, scalar prefetched cube load -- its case-count table in LDS unless that costs a workgroup per CU;
  // else a few leaves: occupancy is no concern, table in LDS). rows: share_corners = 2 asks for the distinct z rows of a brick once
  // each (kernels_octree.h: DZ); a specialised handle without a scratch-free build of that form evaluates every row through its
  // specialised kernel (v.dz comes back false). The per-tree kernel is the same launch whichever W it was built for.
  LeafPick leaf_pick(int lq, bool rows = false) const {
    const LeafConfig c = leaf_config();
    const bool own = spec.f_leaf && spec.leaf_k == c.k;
    const int aw = leaf_aot_waves(c.k, c.w);
    if (rows && spec.f_leaf_dz) return {{4, spec.rows_w, true, c.ntlds, spec.rows_both, true}, spec.f_leaf_dz};
    if (rows && !own) return {{4, aw, true, c.ntlds, false, true}, nullptr};
    if (own && lq == 3) return {{c.k, spec.leaf_w, true, c.ntlds, spec.leaf_both, false}, spec.f_leaf};
    return {{c.k, aw, lq == 3, lq == 3 ? c.ntlds : true, false, false}, nullptr};
  }
  size_t lds_bytes(int k = 1) const { return (size_t)(prog.nslots > 0 ? prog.nslots : 1) * k * BLOCK * sizeof(float); }
  // The largest trees (gsdf_hip.h: "Largest trees"). A workgroup may ask for a CU's whole LDS and no more; an entry point whose
  // kernels would ask for more refuses the tree on the host, before its first launch: lds_refused(what, dynamic + static bytes of
  // its most demanding launch, the slot limit that follows from them) is GSDF_OK or GSDF_ERR_BAD_TREE with the limit in the message.
  static constexpr size_t kLdsPerCu = (size_t)160 * 1024;
  int lds_refused(const char* what, size_t need, const std::string& limit) const {
    if (need <= kLdsPerCu) return GSDF_OK;
    return fail(GSDF_ERR_BAD_TREE, std::string("tree too large for ") + what + ": " + std::to_string(prog.nslots) + " slots (interval stack " +
                std::to_string(prog.lip_depth) + ") need " + std::to_string(need) + " bytes of LDS per workgroup, a CU has " + std::to_string(kLdsPerCu) +
                " (limit: " + limit + ")");
  }
  // normals_kernel, project_kernel, ray_kernel<true>, dc_normals_kernel: two points per lane, no static LDS
  int normals_refused(const char* what) const { return lds_refused(what, lds_bytes(2), std::to_string(GSDF_HIP_MAX_SLOTS_NORMALS) + " slots"); }
  static_assert((size_t)GSDF_HIP_MAX_SLOTS_NORMALS * 2 * BLOCK * sizeof(float) <= kLdsPerCu && (size_t)(GSDF_HIP_MAX_SLOTS_NORMALS + 1) * 2 * BLOCK * sizeof(float) > kLdsPerCu,
                "gsdf_hip.h: GSDF_HIP_MAX_SLOTS_NORMALS is the largest slot count whose two points per lane fit a CU's LDS");
  // what gsdf_hip_program_create adds to one point per lane. Kept as it was for ABI stability (GSDF_HIP_MAX_SLOTS_CREATE is a public,
  // tested limit): a brick's eight rows, and the 4096 + 128 * 36 + 64 bytes of triangle table, LDS triangle stage and scan words
  // that a leaf kernel which also emitted the triangles once added; no kernel asks for more
  static constexpr size_t kCreateExtra = 8 * BLOCK * 4 + 4096 + 128 * 36 + 64;
  static_assert((size_t)GSDF_HIP_MAX_SLOTS_CREATE * BLOCK * sizeof(float) + kCreateExtra <= kLdsPerCu && (size_t)(GSDF_HIP_MAX_SLOTS_CREATE + 1) * BLOCK * sizeof(float) + kCreateExtra > kLdsPerCu,
                "gsdf_hip.h: GSDF_HIP_MAX_SLOTS_CREATE is the largest slot count gsdf_hip_program_create accepts");
  // dual contouring's origin sweep: the ahead-of-time builds are <4,3>, <2,3>, <1,4> (the others need scratch). One rule for the
  // launch (abi_mesh.hip: dc_mesh) and for the name gsdf_hip_program_kernels reports.
  static SweepVariant dc_origin_variant(int k) { return {k, k == 1 ? 4 : 3}; }
  // Workgroups per CU the lattice/eval sweeps are compiled for (their W template argument): 4 when the LDS allows it.
  int sweep_waves(int k) const {
    static const int forced = env_int("GSDF_HIP_SWEEP_WAVES", 0);  // tuning / debugging knob
    if (k != 1 && (forced == 3 || forced == 4)) return forced;
    return (k == 1 || 4 * (lds_bytes(k) + 64) <= kLdsPerCu) ? 4 : 3;
  }
  SweepVariant sweep_variant(int k) const { return {k, sweep_waves(k)}; }
  // Points carried per lane: as many as keep >= 2 workgroups per CU resident (160 KB LDS per CU).
  int batch_k() const {
    static const int forced = env_int("GSDF_HIP_BATCH_K", 0);  // tuning knob
    if (forced == 1 || forced == 2 || forced == 4) return forced;
    return prog.nslots <= 12 ? 4 : (prog.nslots <= 28 ? 2 : 1);
  }
};

// One launch path for the kernels that exist twice: `aot`, the ahead-of-time (interpreter) kernel, gives the parameter types
// P...; `f` is the handle's per-tree build with the same parameters, launched instead when there is one. Every argument is
// converted to the kernel's own parameter type, whatever the type of the expression at the call (launch_args.h). aot may be a
// null pointer of the right type where no ahead-of-time build of the variant exists: without f that is an error, not a launch.
inline hipError_t launch_fn(hipFunction_t f, unsigned grid, unsigned block, size_t lds, hipStream_t s, void** args) {
  return hipModuleLaunchKernel(f, grid, 1, 1, block, 1, 1, (unsigned)lds, s, args, nullptr);
}
template <typename... P, typename... A>
inline hipError_t launch_kernel(void (*aot)(P...), hipFunction_t f, unsigned grid, unsigned block, size_t lds, hipStream_t s, const A&... a) {
  static_assert(launch_args::accepts<void(P...), const A&...>::value, "kernel launch: argument count or types do not fit the kernel's signature");
  if (f) {
    launch_args::Marshalled<void(P...)> m(a...);
    return launch_fn(f, grid, block, lds, s, m.args());
  }
  if (!aot) return hipErrorInvalidDeviceFunction;
  hipLaunchKernelGGL(aot, dim3(grid), dim3(block), lds, s, static_cast<P>(a)...);
  return hipGetLastError();
}

inline unsigned grid_for(uint64_t n, int num_cu, int blocks_per_cu) {
  uint64_t b = (n + BLOCK - 1) / BLOCK;
  uint64_t mx = (uint64_t)num_cu * (uint64_t)blocks_per_cu;
  if (b > mx) b = mx;
  if (b < 1) b = 1;
  return (unsigned)b;
}

// A background build (gsdf_hip_program_specialize_async) that has finished is taken over here: called at the top of the entry
// points that launch evaluating kernels. One relaxed load when there is nothing to adopt. abi_spec.hip.
void spec_adopt_slow(gsdf_program* p);
inline void spec_adopt(gsdf_program* p) { if (p->spec_async.load(std::memory_order_acquire) == 2) spec_adopt_slow(p); }
// The kernels of group g for a specialised handle, built the first time an entry point asks (abi_spec.hip). One atomic load and no
// lock where there is nothing to build: the handle is not specialised, or the group has been tried.
void spec_ensure(gsdf_program* p, SpecGroup g);
// gleval.NormalsCentralDiff on device-resident points (abi_eval.hip; what gsdf_hip_normals3 launches): blocking.
int normals3_dev(gsdf_program* p, const float* d_pos, float* d_nrm, size_t n, float step);
// The projection of device-resident points onto the field (abi_eval.hip; what gsdf_hip_indexed_project launches; gsdf_hip.h states
// the arithmetic): d_pos 12-byte xyz on the program's device; d_out_pos (3 n floats), d_before, d_after (n floats), d_status (n bytes)
// each optional; st->n_verts .. steps_max and ms_device are filled. Blocking. The options are the caller's to check.
int project_dev(gsdf_program* p, const float* d_pos, size_t n, const gsdf_project_opts* o, float* d_out_pos, float* d_before, float* d_after,
                uint8_t* d_status, gsdf_project_stats* st);
// Rays through the field (abi_eval.hip; what gsdf_hip_raycast3 and gsdf_hip_indexed_thickness launch; gsdf_hip.h states the
// arithmetic). d_in on the program's device: n rays of 24 bytes, or, with step > 0, n vertices of 12 bytes whose rays the kernel
// builds along the inward normal (h = step / 2; d_t then receives the thickness). d_t, d_d (n floats), d_status (n bytes), d_steps
// (n uint16) each optional; *st is filled. Blocking. The options are the caller's to check.
int ray_dev(gsdf_program* p, const float* d_in, size_t n, const gsdf_ray_opts* o, float step, float thin, float* d_t, float* d_d, uint8_t* d_status,
            uint16_t* d_steps, gsdf_ray_stats* st);
// gsdf_ray_opts as gsdf_hip.h allows them: GSDF_OK, or GSDF_ERR_BAD_ARGUMENT with `what` in front of the text
int ray_opts_refused(const gsdf_ray_opts* o, const char* what);

namespace {
// ms3.Box.ScaleCentered(1.01) = NewCenteredBox(Center(), MulElem(scale, Size())) [external]; float32, unfused.
inline void scale_centered(const float bb[6], float s, float mn[3], float mx[3]) {
  for (int a = 0; a < 3; a++) {
    const float c = 0.5f * (bb[a] + bb[a + 3]);
    const float size = bb[a + 3] - bb[a];
    float sz = fmaxf(s, 0.f) * size;
    const float half = 0.5f * fmaxf(sz, 0.f);
    mn[a] = c - half;
    mx[a] = c + half;
  }
}
struct DevBuf {
  void* p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
};
}  // namespace
