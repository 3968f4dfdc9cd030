// abi_contour.hip -- C ABI (include/gsdf_hip.h, section "contours"): the outline of a 2-D part and the z-slices of a 3-D part as
// ordered closed loops, traced on the device. The gsdf_contour handle, gsdf_hip_contour2 / gsdf_hip_slice3, counts / read / stats.
// Kernels: kernels_contour.h. The distances come from the program's own Evaluate (gsdf_hip_eval2_dev / gsdf_hip_eval3_dev:
// interpreter or per-tree kernels, whichever the handle has); no interpreter kernel is compiled here.
// Behind the tracer (section "contours: simplify and measures", kernels_contour_simplify.h): gsdf_hip_contour_create uploads loops,
// gsdf_hip_contour_simplify drops vertices within a tolerance of dyadic chords, gsdf_hip_contour_measures sums areas and lengths,
// gsdf_hip_contour_sections (kernels_mass.h) first and second moments of area, gsdf_hip_contour_hatch (kernels_hatch.h) the segments
// of parallel lines inside the loops, as a gsdf_hatch handle of its own, gsdf_hip_contour_hatch_skin (kernels_skin.h) those segments cut
// against the layers under and over each layer and classed as inner, bottom or top skin, gsdf_hip_contour_offset /
// gsdf_hip_contour_distance (kernels_offset.h) the loops moved sideways by in-plane distances: the signed distance of a lattice to the
// layer's own edges, traced by the tracer's steps 2 .. 5 (Tracer below, which gsdf_hip_contour2 / gsdf_hip_slice3 run too).
// What the entry points share stands once, ahead of them: Job (a call's stream, events and final wait), contour_new / hatch_new (the
// handles' buffers), the fixed-point helpers (exponent_of, unordered, maxbits_enqueue; mass::whole and mass::value from mass_host.h),
// scan_offsets (counts -> offsets), Tracer (steps 2 .. 5), hatch_open / length_of (the opening and the tail of hatch and skin).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <deque>
#include <limits>
#include <memory>
#include <new>
#include <vector>

#include "kernels_common.h"
#include "kernels_contour.h"
#include "kernels_contour_simplify.h"
#define KERNELS_MASS_LOOPS
#include "kernels_mass.h"
#include "mass_host.h"
#include "kernels_hatch.h"
#include "kernels_skin.h"
#include "kernels_offset.h"
#include "abi_program.h"

struct gsdf_contour {
  int device = 0;
  uint64_t n_loops = 0, n_verts = 0;
  DevPtr<float> xy;
  DevPtr<unsigned> keys, loop_start, loop_layer;  // loop_start: n_loops + 1
  gsdf_contour_stats st{};
};

extern "C" void gsdf_hip_contour_destroy(gsdf_contour* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  delete c;
}

namespace {
struct ContourDelete { void operator()(gsdf_contour* c) const { gsdf_hip_contour_destroy(c); } };
using ContourPtr = std::unique_ptr<gsdf_contour, ContourDelete>;

// (kernel parameters convert implicitly: a T* buffer goes to a const T* parameter as it is. The casts left at the launches below
// reinterpret -- float data read or written as words, w.pos reused as vertex numbers -- or narrow a count that a capacity check bounds.)
#define LAUNCH(KERNEL, GRID, STREAM, ...)                                          \
  do {                                                                             \
    hipLaunchKernelGGL(KERNEL, dim3(GRID), dim3(BLOCK), 0, STREAM, __VA_ARGS__);   \
    HIP_TRY(hipGetLastError());                                                    \
  } while (0)

unsigned blocks_of(uint64_t n) { return (unsigned)((n + BLOCK - 1) / BLOCK); }

template <typename T>
bool dev_alloc(DevPtr<T>& b, uint64_t n) {
  b.reset();
  if (hipMalloc((void**)&b.p, (n ? n : 1) * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); b.p = nullptr; return false; }
  return true;
}

// One call's stream, events and final wait. `stream` is the call's own Stream or the program's, borrowed; the caller declares it
// first, then its workspaces and unfinished handles, then the Job: on every way out the Job goes first and waits for the stream, then
// the buffers go, and an owned stream is destroyed last.
struct Job : NoCopy {
  Stream& stream;
  hipStream_t s = nullptr;
  EventSet<8> ev;
  explicit Job(Stream& st) : stream(st) {}
  ~Job() { if (s) (void)hipStreamSynchronize(s); }
  int open() {
    HIP_TRY(stream.ensure());
    if (ev.ensure() != hipSuccess) return fail(GSDF_ERR_HIP, "hipEventCreate failed");
    s = stream.s;
    return GSDF_OK;
  }
  double ms(int a, int b) const { float t = 0; return hipEventElapsedTime(&t, ev[a], ev[b]) == hipSuccess ? (double)t : 0.0; }
};

// a handle for n_verts vertices in n_loops loops: buffers only, the stats' three counts set
int contour_new(int device, uint64_t n_verts, uint64_t n_loops, uint32_t n_layers, ContourPtr* out) {
  ContourPtr c(new (std::nothrow) gsdf_contour());
  if (!c) return fail(GSDF_ERR_BAD_ARGUMENT, "out of memory");
  c->device = device;
  c->n_verts = n_verts;
  c->n_loops = n_loops;
  c->st.n_verts = n_verts;
  c->st.n_loops = n_loops;
  c->st.n_layers = n_layers;
  if (!dev_alloc(c->xy, 2 * n_verts) || !dev_alloc(c->keys, n_verts) || !dev_alloc(c->loop_start, n_loops + 1) || !dev_alloc(c->loop_layer, n_loops))
    return fail(GSDF_ERR_HIP, "contour: no device memory for the result");
  *out = std::move(c);
  return GSDF_OK;
}

// ---- fixed point: the sums are integers at a power of two that the largest |coordinate| decides (gsdf_hip.h states the arithmetic) ----
// memset and cmeas_maxbits_kernel on s: *d_maxbits = the largest bits of |x|, |y| over the handle's vertices. Queues, does not wait.
int maxbits_enqueue(const gsdf_contour* c, unsigned long long* d_maxbits, hipStream_t s) {
  const uint64_t V = c->n_verts;
  const unsigned nb_max = blocks_of(2 * V) < 1024u ? blocks_of(2 * V) : 1024u;
  HIP_TRY(hipMemsetAsync(d_maxbits, 0, 8, s));
  LAUNCH(cmeas_maxbits_kernel, nb_max, s, c->xy.p, (unsigned long long)(2 * V), d_maxbits);
  return GSDF_OK;
}
// the exponent e of that word: coordinates are below 2^e (0, the word of a handle without vertices: -125)
int exponent_of(unsigned long long maxbits) { return (int)std::max(1u, (unsigned)(maxbits >> 23)) - 126; }
// the float whose order-preserving word (cmeas_kernel's and offset_bbox_kernel's boxes) is o
float unordered(unsigned o) {
  const unsigned b = o ^ ((o >> 31) ? 0x80000000u : 0xffffffffu);
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}
// (integers -> float64: mass::whole puts the two words of a sum together, mass::value rounds it once and scales by a power of two)

// cnt[n], whose per-block sums the kernel that counted left in blk_cnt -> off[n + 1], exclusive; *total = their sum. On s.
int scan_offsets(const unsigned* cnt, uint64_t n, const unsigned* blk_cnt, unsigned* blk_base, unsigned long long* total, unsigned* off, hipStream_t s) {
  const unsigned nb = blocks_of(n);
  if (int rc = launch_block_scan(blk_cnt, nb, blk_base, total, s)) return rc;
  LAUNCH(hatch_scan_kernel, nb, s, cnt, (unsigned)n, blk_base, off);
  return GSDF_OK;
}

// nodes along one axis (gsdf_hip.h, "Lattice"): floor(fl(fl(hi - lo) / res)) + 4; 0 for a count that cannot be a lattice's
uint64_t axis_nodes(float lo, float hi, float res) {
  const float size = hi - lo;
  const float q = size / res;
  if (!(q >= 0.f)) return 4;  // (an empty or inverted box: the ring of outside cells alone)
  if (!(q < 2147483648.f)) return 0;
  return (uint64_t)std::floor(q) + 4;
}

unsigned ceil_log2(uint64_t n) {
  unsigned r = 0;
  while (((uint64_t)1 << r) < n) r++;
  return r;
}

// the loops of one chunk of whole layers, still on the device
struct Part {
  uint64_t n_verts = 0, n_loops = 0;
  DevPtr<float> xy;
  DevPtr<unsigned> keys, loop_start, loop_layer;
};

// what every chunk of a call shares: node-sized buffers for the largest chunk, vertex-sized ones that grow
struct Workspace {
  DevPtr<float> pos, dist, z;
  DevPtr<unsigned> succ, blk_cnt, blk_base, layer_base;
  DevPtr<unsigned long long> totals;  // [0] cut edges, [1] loops, [2] vertices of the loops
  DevPtr<ContourCounters> ctr;
  Arena verts;  // nine arrays of V words
  Arena blk;    // four arrays of blocks_of(V) words
};

// The tracer's steps 2 .. 5 over a call's chunks, and what the call carries from chunk to chunk. The caller plans, allocates, queues
// its field pass into w.dist chunk by chunk (job.ev[0] recorded ahead of it) with chunk() behind each, and finishes. A unit is what
// the caller's chunks are whole numbers of: a layer (contour2 / slice3), an input layer with all its insets (offset).
struct Tracer {
  gsdf_contour_stats& st;
  std::deque<Part> parts;  // (ahead of the workspace: it goes first)
  Workspace w;
  std::vector<unsigned> h_base;
  uint64_t largest_layer = 0;
  ContourLattice lat{};
  uint64_t per_chunk = 0;                     // units per chunk
  uint64_t chunk_nodes = 0, chunk_layers = 0;  // of a full chunk

  // The one lattice of the call and its layers into st. Units per chunk: max_nodes nodes, at least one unit, the chunk's slots
  // (layer * 2 N + key) below 2^32, no more than there are.
  void plan(const ContourLattice& lattice, uint64_t max_nodes, uint64_t layers_per_unit, uint64_t n_units) {
    lat = lattice;
    st.nx = lat.nx;
    st.ny = lat.ny;
    st.n_layers = (uint32_t)(n_units * layers_per_unit);
    const uint64_t unit_nodes = (uint64_t)lat.nx * lat.ny * layers_per_unit;
    per_chunk = std::min({std::max<uint64_t>(max_nodes / unit_nodes, 1), (((uint64_t)1 << 31) - 1) / unit_nodes, n_units});
    chunk_nodes = per_chunk * unit_nodes;
    chunk_layers = per_chunk * layers_per_unit;
  }

  // The buffers of a full chunk, the counters cleared on the job's stream. pos_words: words of w.pos per node (the field pass's
  // positions; the slots' vertex numbers live there afterwards: 8 bytes per node at least). z: n_z planes for w.z, or null.
  int alloc(Job& job, unsigned pos_words, const float* z, uint64_t n_z, const char* nomem) {
    const uint64_t chunk_slots = 2 * chunk_nodes;
    const unsigned slot_blocks = blocks_of(chunk_slots);
    if (!dev_alloc(w.pos, chunk_nodes * pos_words) || !dev_alloc(w.dist, chunk_nodes) || !dev_alloc(w.succ, chunk_slots) || !dev_alloc(w.blk_cnt, slot_blocks) ||
        !dev_alloc(w.blk_base, slot_blocks) || !dev_alloc(w.layer_base, chunk_layers + 1) || !dev_alloc(w.totals, 3) || !dev_alloc(w.ctr, 1) || (n_z && !dev_alloc(w.z, n_z)))
      return fail(GSDF_ERR_HIP, nomem);
    h_base.resize(chunk_layers + 1);
    if (z) HIP_TRY(hipMemcpyAsync(w.z.p, z, (size_t)n_z * 4, hipMemcpyHostToDevice, job.s));
    HIP_TRY(hipMemsetAsync(w.ctr.p, 0, sizeof(ContourCounters), job.s));
    return GSDF_OK;
  }

  // Steps 2 .. 5 of one chunk of Lc whole layers whose distances stand in w.dist: cells -> succ, vertex numbers, leaders and ranks,
  // the loops -> a Part (none for a chunk without a cut edge; with emit false the counts alone). l0: the chunk's first layer. Adds to
  // st's counts and times; waits for the stream.
  int chunk(Job& job, uint64_t Lc, uint64_t l0, bool emit) {
    const char* nomem = "contour: no device memory for the workspace";
    hipStream_t s = job.s;
    const uint64_t N = (uint64_t)lat.nx * lat.ny, E = 2 * N;
    const uint64_t nodes = Lc * N, slots = Lc * E;
    const unsigned nb_slots = blocks_of(slots);
    HIP_TRY(hipEventRecord(job.ev[1], s));
    // 2. cells -> succ over the edge slots; cut edges per block, per layer
    HIP_TRY(hipMemsetAsync(w.succ.p, 0xff, (size_t)slots * 4, s));
    LAUNCH(contour_cells_kernel, blocks_of(nodes), s, lat, w.dist.p, (unsigned long long)nodes, w.succ.p, w.ctr.p);
    LAUNCH(contour_count_kernel, nb_slots, s, w.succ.p, (unsigned long long)slots, w.blk_cnt.p);
    if (int rc = launch_block_scan(w.blk_cnt.p, nb_slots, w.blk_base.p, w.totals.p, s)) return rc;
    LAUNCH(contour_layer_base_kernel, blocks_of(Lc + 1), s, w.succ.p, w.blk_base.p, w.totals.p, (unsigned)E, (unsigned)Lc, w.layer_base.p);
    HIP_TRY(hipEventRecord(job.ev[2], s));
    HIP_TRY(hipMemcpyAsync(h_base.data(), w.layer_base.p, (size_t)(Lc + 1) * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    st.ms_eval += job.ms(0, 1);
    st.ms_trace += job.ms(1, 2);
    const uint64_t V = h_base[Lc];
    uint64_t chunk_largest = 0;
    for (uint64_t l = 0; l < Lc; l++) chunk_largest = std::max<uint64_t>(chunk_largest, h_base[l + 1] - h_base[l]);
    largest_layer = std::max(largest_layer, chunk_largest);
    if (V == 0) return GSDF_OK;
    if (st.n_verts + V >= ((uint64_t)1 << 32)) return fail(GSDF_ERR_CAPACITY, "contour: 2^32 vertices or more");
    // 3. vertex numbers, links, the leaders by pointer jumping, the ranks by list ranking: rounds for the chunk's largest layer
    const unsigned nb_v = blocks_of(V);
    if (w.verts.ensure((size_t)V * 9 * 4) != hipSuccess || w.blk.ensure((size_t)nb_v * 4 * 4) != hipSuccess) return fail(GSDF_ERR_HIP, nomem);
    unsigned* va = (unsigned*)w.verts.p;
    unsigned *slot_of = va, *pred = va + V, *mn[2] = {va + 2 * V, va + 3 * V}, *lk[2] = {va + 4 * V, va + 5 * V}, *rk[2] = {va + 6 * V, va + 7 * V}, *start_of = va + 8 * V;
    unsigned* ba = (unsigned*)w.blk.p;
    unsigned *blk_loops = ba, *blk_len = ba + nb_v, *base_loops = ba + 2 * (size_t)nb_v, *base_len = ba + 3 * (size_t)nb_v;
    unsigned* vnum = (unsigned*)w.pos.p;
    const unsigned rounds = ceil_log2(chunk_largest);
    HIP_TRY(hipEventRecord(job.ev[3], s));
    LAUNCH(contour_number_kernel, nb_slots, s, w.succ.p, (unsigned long long)slots, w.blk_base.p, (unsigned)V, vnum, slot_of, w.ctr.p);
    LAUNCH(contour_link_kernel, nb_v, s, w.succ.p, (unsigned long long)slots, vnum, slot_of, (unsigned)V, pred, mn[0], lk[0], w.ctr.p);
    int cur = 0;
    for (unsigned r = 0; r < rounds; r++, cur ^= 1) LAUNCH(contour_min_kernel, nb_v, s, mn[cur], lk[cur], (unsigned)V, mn[cur ^ 1], lk[cur ^ 1]);
    const unsigned* leader = mn[cur];
    LAUNCH(contour_rank_init_kernel, nb_v, s, leader, pred, (unsigned)V, rk[0], lk[0]);
    int rc_ = 0;
    for (unsigned r = 0; r < rounds; r++, rc_ ^= 1) LAUNCH(contour_rank_kernel, nb_v, s, rk[rc_], lk[rc_], (unsigned)V, rk[rc_ ^ 1], lk[rc_ ^ 1]);
    const unsigned* rank = rk[rc_];
    // 4. leaders -> loops
    LAUNCH(contour_leader_count_kernel, nb_v, s, leader, pred, rank, (unsigned)V, blk_loops, blk_len);
    if (int rc = launch_block_scan(blk_loops, nb_v, base_loops, w.totals.p + 1, s)) return rc;
    if (int rc = launch_block_scan(blk_len, nb_v, base_len, w.totals.p + 2, s)) return rc;
    HIP_TRY(hipEventRecord(job.ev[4], s));
    unsigned long long h_tot[3] = {0, 0, 0};
    ContourCounters h_ctr;
    HIP_TRY(hipMemcpyAsync(h_tot, w.totals.p, sizeof h_tot, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&h_ctr, w.ctr.p, sizeof h_ctr, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    st.ms_trace += job.ms(3, 4);
    const uint64_t nl = h_tot[1];
    if (h_ctr.bad || nl == 0 || nl > V || h_tot[2] != V) return fail(GSDF_ERR_HIP, "contour: internal error (succ is not a permutation of the cut edges)");
    if (emit) {
      // 5. emit
      parts.emplace_back();
      Part& part = parts.back();
      part.n_verts = V;
      part.n_loops = nl;
      if (!dev_alloc(part.xy, 2 * V) || !dev_alloc(part.keys, V) || !dev_alloc(part.loop_start, nl) || !dev_alloc(part.loop_layer, nl)) return fail(GSDF_ERR_HIP, nomem);
      HIP_TRY(hipEventRecord(job.ev[5], s));
      LAUNCH(contour_leader_number_kernel, nb_v, s, leader, pred, rank, slot_of, (unsigned)V, base_loops, base_len, (unsigned)nl, (unsigned)E, (unsigned)l0, (unsigned)st.n_verts,
             start_of, part.loop_start.p, part.loop_layer.p, w.ctr.p);
      LAUNCH(contour_emit_kernel, nb_v, s, lat, w.dist.p, slot_of, leader, rank, start_of, (unsigned)V, (unsigned)E, part.xy.p, part.keys.p, w.ctr.p);
      HIP_TRY(hipEventRecord(job.ev[6], s));
      HIP_TRY(hipStreamSynchronize(s));
      st.ms_trace += job.ms(5, 6);
    }
    st.n_verts += V;
    st.n_loops += nl;
    return GSDF_OK;
  }

  // Behind the last chunk: the counters of the whole call into st; with `out`, a handle with st and the chunks' loops behind one another.
  int finish(Job& job, int device, ContourPtr* out) {
    hipStream_t s = job.s;
    ContourCounters h_ctr;
    HIP_TRY(hipMemcpyAsync(&h_ctr, w.ctr.p, sizeof h_ctr, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h_ctr.bad) return fail(GSDF_ERR_HIP, "contour: internal error (a vertex out of range)");
    st.border_inside = h_ctr.border_inside;
    st.nonfinite_nodes = h_ctr.nonfinite_nodes;
    st.saddle_cells = h_ctr.saddle_cells;
    st.rank_rounds = ceil_log2(largest_layer);
    st.ms_device = st.ms_eval + st.ms_trace;
    if (!out) return GSDF_OK;
    ContourPtr c;
    if (int rc = contour_new(device, st.n_verts, st.n_loops, st.n_layers, &c)) return rc;
    c->st = st;
    uint64_t v0 = 0, q0 = 0;
    for (const Part& part : parts) {
      HIP_TRY(hipMemcpyAsync(c->xy.p + 2 * v0, part.xy.p, (size_t)part.n_verts * 8, hipMemcpyDeviceToDevice, s));
      HIP_TRY(hipMemcpyAsync(c->keys.p + v0, part.keys.p, (size_t)part.n_verts * 4, hipMemcpyDeviceToDevice, s));
      HIP_TRY(hipMemcpyAsync(c->loop_start.p + q0, part.loop_start.p, (size_t)part.n_loops * 4, hipMemcpyDeviceToDevice, s));
      HIP_TRY(hipMemcpyAsync(c->loop_layer.p + q0, part.loop_layer.p, (size_t)part.n_loops * 4, hipMemcpyDeviceToDevice, s));
      v0 += part.n_verts;
      q0 += part.n_loops;
    }
    const unsigned end = (unsigned)c->n_verts;
    HIP_TRY(hipMemcpyAsync(c->loop_start.p + c->n_loops, &end, 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    *out = std::move(c);
    return GSDF_OK;
  }
};

int contour_run(gsdf_program* p, int dim, float res, const float* z, uint32_t n_z, const gsdf_contour_opts* o, gsdf_contour** out) {
  if (!p || !out) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *out = nullptr;
  if (p->prog.is2d != (dim == 2)) return fail(GSDF_ERR_DIMENSION, dim == 2 ? "program is 3D, contour2 called" : "program is 2D, slice3 called");
  if (dim == 3 && (!z || n_z == 0)) return fail(GSDF_ERR_BAD_ARGUMENT, "slice3 needs at least one z");
  const float* bb = p->prog.bb;
  if (!std::isfinite(res) || !(res > 0.f)) return fail(GSDF_ERR_BAD_ARGUMENT, "contour: res must be finite and positive");
  for (int a = 0; a < 6; a++)
    if (a % 3 != 2 && !std::isfinite(bb[a])) return fail(GSDF_ERR_BAD_ARGUMENT, "contour: the program's bounds are not finite");
  const uint64_t nx = axis_nodes(bb[0], bb[3], res), ny = axis_nodes(bb[1], bb[4], res);
  if (nx == 0 || ny == 0 || nx * ny >= ((uint64_t)1 << 31)) return fail(GSDF_ERR_BAD_ARGUMENT, "contour: the lattice needs 2^31 nodes or more at this res");
  const uint64_t N = nx * ny, L = dim == 2 ? 1 : n_z;
  ContourLattice lat{(unsigned)nx, (unsigned)ny, bb[0] - res, bb[1] - res, res};

  HIP_TRY(hipSetDevice(p->device));
  spec_adopt(p);
  gsdf_contour_stats st{};
  Tracer t{st};
  ContourPtr c;
  Job job(p->stream);  // (the program's stream, borrowed)
  if (int rc = job.open()) return rc;
  hipStream_t s = job.s;
  t.plan(lat, o && o->max_nodes ? o->max_nodes : (uint64_t)GSDF_CONTOUR_DEFAULT_MAX_NODES, 1, L);
  if (int rc = t.alloc(job, dim == 2 ? 2 : 3, dim == 3 ? z : nullptr, L, "contour: no device memory for the workspace")) return rc;
  Workspace& w = t.w;
  for (uint64_t l0 = 0; l0 < L; l0 += t.per_chunk) {
    const uint64_t Lc = L - l0 < t.per_chunk ? L - l0 : t.per_chunk;
    const uint64_t nodes = Lc * N;
    // 1. evaluate: positions, then the program's Evaluate over them
    HIP_TRY(hipEventRecord(job.ev[0], s));
    if (dim == 2) LAUNCH(contour_pos_kernel<2>, blocks_of(nodes), s, lat, nullptr, (unsigned long long)nodes, w.pos.p);
    else LAUNCH(contour_pos_kernel<3>, blocks_of(nodes), s, lat, w.z.p + l0, (unsigned long long)nodes, w.pos.p);
    if (int rc = dim == 2 ? gsdf_hip_eval2_dev(p, w.pos.p, 8, w.dist.p, (size_t)nodes, (void*)s) : gsdf_hip_eval3_dev(p, w.pos.p, 12, w.dist.p, (size_t)nodes, (void*)s)) return rc;
    // 2 .. 5. trace
    if (int rc = t.chunk(job, Lc, l0, true)) return rc;
  }
  st.evals = N * L;
  if (int rc = t.finish(job, p->device, &c)) return rc;
  *out = c.release();
  return GSDF_OK;
}
}  // namespace

extern "C" int gsdf_hip_contour2(gsdf_program* p2d, float res, const gsdf_contour_opts* o, gsdf_contour** out) { return contour_run(p2d, 2, res, nullptr, 1, o, out); }
extern "C" int gsdf_hip_slice3(gsdf_program* p3d, float res, const float* z, uint32_t n_z, const gsdf_contour_opts* o, gsdf_contour** out) {
  return contour_run(p3d, 3, res, z, n_z, o, out);
}

extern "C" int gsdf_hip_contour_counts(const gsdf_contour* c, uint32_t* n_layers, uint64_t* n_loops, uint64_t* n_verts) {
  if (!c) return fail(GSDF_ERR_BAD_ARGUMENT, "null contour");
  if (n_layers) *n_layers = c->st.n_layers;
  if (n_loops) *n_loops = c->n_loops;
  if (n_verts) *n_verts = c->n_verts;
  return GSDF_OK;
}

extern "C" int gsdf_hip_contour_read(const gsdf_contour* c, float* xy, uint32_t* keys, uint32_t* loop_start, uint32_t* loop_layer) {
  if (!c) return fail(GSDF_ERR_BAD_ARGUMENT, "null contour");
  HIP_TRY(hipSetDevice(c->device));
  if (xy && c->n_verts) HIP_TRY(hipMemcpy(xy, c->xy.p, (size_t)c->n_verts * 8, hipMemcpyDeviceToHost));
  if (keys && c->n_verts) HIP_TRY(hipMemcpy(keys, c->keys.p, (size_t)c->n_verts * 4, hipMemcpyDeviceToHost));
  if (loop_start) HIP_TRY(hipMemcpy(loop_start, c->loop_start.p, (size_t)(c->n_loops + 1) * 4, hipMemcpyDeviceToHost));
  if (loop_layer && c->n_loops) HIP_TRY(hipMemcpy(loop_layer, c->loop_layer.p, (size_t)c->n_loops * 4, hipMemcpyDeviceToHost));
  return GSDF_OK;
}

extern "C" int gsdf_hip_contour_stats_get(const gsdf_contour* c, gsdf_contour_stats* st) {
  if (!c || !st) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *st = c->st;
  return GSDF_OK;
}

// ---- loops after tracing: upload, simplify, measures (gsdf_hip.h, "contours: simplify and measures") -------------------------------
namespace {
struct SimplifyWs {
  DevPtr<unsigned> loop_of, rej, changed, blk_cnt, blk_base;
  DevPtr<unsigned char> keep;
  DevPtr<unsigned long long> total;
  DevPtr<CsimpCounters> ctr;
};
}  // namespace

extern "C" int gsdf_hip_contour_create(const float* xy, uint64_t n_verts, const uint32_t* loop_start, uint64_t n_loops, const uint32_t* loop_layer, uint32_t n_layers,
                                       const uint32_t* keys, gsdf_contour** out) {
  if (!out) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *out = nullptr;
  if (n_loops == 0 || n_verts == 0) return fail(GSDF_ERR_EMPTY_BUFFERS, "empty buffers");
  if (!xy || !loop_start) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (n_verts >= ((uint64_t)1 << 32)) return fail(GSDF_ERR_CAPACITY, "contour: 2^32 vertices or more");
  if (n_layers == 0) return fail(GSDF_ERR_BAD_ARGUMENT, "contour: n_layers must be at least 1");
  if (loop_start[0] != 0) return fail(GSDF_ERR_BAD_ARGUMENT, "contour: loop 0 starts at vertex " + std::to_string(loop_start[0]) + ", not at 0");
  for (uint64_t q = 0; q < n_loops; q++)
    if ((uint64_t)loop_start[q + 1] < (uint64_t)loop_start[q] + 3)
      return fail(GSDF_ERR_BAD_ARGUMENT, "contour: loop " + std::to_string(q) + " (vertices " + std::to_string(loop_start[q]) + " .. " + std::to_string(loop_start[q + 1]) +
                                             ") has fewer than 3 vertices");
  if (loop_start[n_loops] != n_verts)
    return fail(GSDF_ERR_BAD_ARGUMENT, "contour: loop " + std::to_string(n_loops - 1) + " ends at vertex " + std::to_string(loop_start[n_loops]) + ", the handle has " +
                                           std::to_string(n_verts) + " vertices");
  if (loop_layer)
    for (uint64_t q = 0; q < n_loops; q++) {
      if (loop_layer[q] >= n_layers)
        return fail(GSDF_ERR_BAD_ARGUMENT, "contour: loop " + std::to_string(q) + " names layer " + std::to_string(loop_layer[q]) + ", the handle has " + std::to_string(n_layers) + " layers");
      if (q > 0 && loop_layer[q] < loop_layer[q - 1])
        return fail(GSDF_ERR_BAD_ARGUMENT, "contour: loop " + std::to_string(q) + " is in layer " + std::to_string(loop_layer[q]) + ", behind a loop of layer " + std::to_string(loop_layer[q - 1]));
    }
  for (uint64_t i = 0; i < 2 * n_verts; i++)
    if (!std::isfinite(xy[i])) return fail(GSDF_ERR_BAD_ARGUMENT, "contour: vertex " + std::to_string(i / 2) + " has a NaN or infinite coordinate");
  int device = 0;
  HIP_TRY(hipGetDevice(&device));
  ContourPtr c;
  if (int rc = contour_new(device, n_verts, n_loops, n_layers, &c)) return rc;
  hipError_t e = hipMemcpy(c->xy.p, xy, (size_t)n_verts * 8, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(c->loop_start.p, loop_start, (size_t)(n_loops + 1) * 4, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = keys ? hipMemcpy(c->keys.p, keys, (size_t)n_verts * 4, hipMemcpyHostToDevice) : hipMemset(c->keys.p, 0, (size_t)n_verts * 4);
  if (e == hipSuccess) e = loop_layer ? hipMemcpy(c->loop_layer.p, loop_layer, (size_t)n_loops * 4, hipMemcpyHostToDevice) : hipMemset(c->loop_layer.p, 0, (size_t)n_loops * 4);
  if (e != hipSuccess) return fail(GSDF_ERR_HIP, std::string("contour upload: ") + hipGetErrorString(e));
  *out = c.release();
  return GSDF_OK;
}

extern "C" int gsdf_hip_contour_simplify(const gsdf_contour* c, const gsdf_contour_simplify_opts* o, gsdf_contour** out, gsdf_contour_simplify_stats* st_out) {
  if (out) *out = nullptr;
  if (!c || !o) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (!(o->tol >= 0.f)) return fail(GSDF_ERR_BAD_ARGUMENT, "contour simplify: tol must be a number >= 0");
  if (o->levels > CSIMP_MAX_LEVELS) return fail(GSDF_ERR_BAD_ARGUMENT, "contour simplify: levels must be 1 .. 16 (0: 8)");
  if (o->passes > 8) return fail(GSDF_ERR_BAD_ARGUMENT, "contour simplify: passes must be 1 .. 8 (0: 1)");
  const bool dry = o->dry != 0;
  if (!out && !dry) return fail(GSDF_ERR_BAD_ARGUMENT, "contour simplify: out may be null in a dry run only");
  const unsigned levels = o->levels ? o->levels : 8u, passes = o->passes ? o->passes : 1u;
  const double tol2 = (double)o->tol * (double)o->tol;
  gsdf_contour_simplify_stats st{};
  st.n_verts_in = st.n_verts_out = c->n_verts;
  st.n_loops = c->n_loops;

  HIP_TRY(hipSetDevice(c->device));
  ContourPtr cur;  // the previous pass's result; null: the caller's handle
  if (c->n_verts > 0 && c->n_loops > 0) {
    const uint64_t V0 = c->n_verts, NL = c->n_loops;
    Stream stream;
    SimplifyWs w;
    Job job(stream);
    if (int rc = job.open()) return rc;
    hipStream_t s = job.s;
    const unsigned nb0 = blocks_of(V0);
    if (!dev_alloc(w.loop_of, V0) || !dev_alloc(w.rej, V0) || !dev_alloc(w.changed, NL) || !dev_alloc(w.blk_cnt, nb0) || !dev_alloc(w.blk_base, nb0) || !dev_alloc(w.keep, V0) ||
        !dev_alloc(w.total, 1) || !dev_alloc(w.ctr, 1))
      return fail(GSDF_ERR_HIP, "contour simplify: no device memory for the workspace");
    HIP_TRY(hipMemsetAsync(w.ctr.p, 0, sizeof(CsimpCounters), s));
    for (unsigned pass = 0; pass < passes; pass++) {
      const gsdf_contour* in = cur ? cur.get() : c;
      const uint64_t V = in->n_verts;
      const unsigned nb = blocks_of(V);
      const bool last = pass + 1 == passes;
      HIP_TRY(hipEventRecord(job.ev[0], s));
      HIP_TRY(hipMemsetAsync(w.rej.p, 0, (size_t)V * 4, s));
      HIP_TRY(hipMemsetAsync(w.changed.p, 0, (size_t)NL * 4, s));
      LAUNCH(cloop_of_kernel, nb, s, in->loop_start.p, (unsigned)NL, (unsigned)V, w.loop_of.p);
      LAUNCH(csimp_reject_kernel, nb, s, in->xy.p, in->loop_start.p, w.loop_of.p, (unsigned)V, levels, tol2, w.rej.p);
      LAUNCH(csimp_mark_kernel, nb, s, in->xy.p, in->loop_start.p, w.loop_of.p, (unsigned)V, levels, w.rej.p, w.keep.p, w.changed.p, w.blk_cnt.p, w.ctr.p);
      if (int rc = launch_block_scan(w.blk_cnt.p, nb, w.blk_base.p, w.total.p, s)) return rc;
      HIP_TRY(hipEventRecord(job.ev[1], s));
      unsigned long long h_total = 0;
      HIP_TRY(hipMemcpyAsync(&h_total, w.total.p, 8, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      st.ms_device += job.ms(0, 1);
      if (h_total < 3 * NL || h_total > V) return fail(GSDF_ERR_HIP, "contour simplify: internal error (a loop kept fewer than 3 vertices)");
      st.n_verts_out = h_total;
      if (last && dry) break;
      ContourPtr next;
      if (int rc = contour_new(c->device, h_total, NL, c->st.n_layers, &next)) return rc;
      HIP_TRY(hipEventRecord(job.ev[2], s));
      LAUNCH(csimp_emit_kernel, nb, s, (const unsigned*)in->xy.p, in->keys.p, in->loop_start.p, w.loop_of.p, (unsigned)V, (unsigned)NL, w.keep.p, w.blk_base.p, (unsigned)h_total,
             (unsigned*)next->xy.p, next->keys.p, next->loop_start.p, w.ctr.p);
      HIP_TRY(hipMemcpyAsync(next->loop_layer.p, c->loop_layer.p, (size_t)NL * 4, hipMemcpyDeviceToDevice, s));
      HIP_TRY(hipEventRecord(job.ev[3], s));
      HIP_TRY(hipStreamSynchronize(s));
      st.ms_device += job.ms(2, 3);
      cur = std::move(next);
    }
    CsimpCounters h_ctr;
    HIP_TRY(hipMemcpyAsync(&h_ctr, w.ctr.p, sizeof h_ctr, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (h_ctr.bad) return fail(GSDF_ERR_HIP, "contour simplify: internal error (a vertex out of range)");
    for (unsigned k = 0; k <= CSIMP_MAX_LEVELS; k++) {
      st.spans[k] = h_ctr.spans[k];
      if (h_ctr.spans[k]) st.max_level = k;
    }
    st.loops_changed = h_ctr.loops_changed;
    double q2 = 0;
    std::memcpy(&q2, &h_ctr.max_q2, 8);
    st.max_dev = std::sqrt(q2);
  }
  if (!dry && !cur) {  // a handle without loops: its copy
    if (int rc = contour_new(c->device, c->n_verts, c->n_loops, c->st.n_layers, &cur)) return rc;
    const unsigned zero = 0;
    HIP_TRY(hipMemcpy(cur->loop_start.p, &zero, 4, hipMemcpyHostToDevice));
  }
  if (st_out) *st_out = st;
  if (!dry) *out = cur.release();
  return GSDF_OK;
}

namespace {
thread_local double g_measures_ms = 0;
thread_local double g_sections_ms = 0;

// What one pass over the loops leaves on the host: the measures' sums, with `sections` the section sums (kernels_mass.h) behind
// them, the loops' extents and layers, the exponent, the device time of all of it.
struct MeasureRun {
  std::vector<CmeasAcc> acc;
  std::vector<CsectAcc> sect;
  std::vector<unsigned> start, layer;
  int e = -125;
  double ms = 0;
};
int measure_run(const gsdf_contour* c, bool sections, MeasureRun* r) {
  const uint64_t V = c->n_verts, NL = c->n_loops;
  r->acc.resize(NL);
  r->sect.resize(sections ? NL : 0);
  r->start.resize(NL + 1);
  r->layer.resize(NL);
  unsigned long long h_maxbits = 0;
  if (V > 0 && NL > 0) {
    HIP_TRY(hipSetDevice(c->device));
    Stream stream;
    DevPtr<unsigned> loop_of;
    DevPtr<CmeasAcc> acc;
    DevPtr<CsectAcc> sect;
    DevPtr<unsigned long long> maxbits;
    Job job(stream);
    if (int rc = job.open()) return rc;
    hipStream_t s = job.s;
    if (!dev_alloc(loop_of, V) || !dev_alloc(acc, NL) || !dev_alloc(maxbits, 1) || (sections && !dev_alloc(sect, NL)))
      return fail(GSDF_ERR_HIP, "contour measures: no device memory for the workspace");
    const unsigned nb = blocks_of(V);
    HIP_TRY(hipEventRecord(job.ev[0], s));
    if (int rc = maxbits_enqueue(c, maxbits.p, s)) return rc;
    LAUNCH(cmeas_init_kernel, blocks_of(NL), s, acc.p, (unsigned)NL);
    LAUNCH(cloop_of_kernel, nb, s, c->loop_start.p, (unsigned)NL, (unsigned)V, loop_of.p);
    LAUNCH(cmeas_kernel, nb, s, c->xy.p, c->loop_start.p, loop_of.p, (unsigned)V, maxbits.p, acc.p);
    if (sections) {
      HIP_TRY(hipMemsetAsync(sect.p, 0, (size_t)NL * sizeof(CsectAcc), s));
      LAUNCH(csect_kernel, nb, s, c->xy.p, c->loop_start.p, loop_of.p, (unsigned)V, maxbits.p, sect.p);
    }
    HIP_TRY(hipEventRecord(job.ev[1], s));
    HIP_TRY(hipMemcpyAsync(r->acc.data(), acc.p, (size_t)NL * sizeof(CmeasAcc), hipMemcpyDeviceToHost, s));
    if (sections) HIP_TRY(hipMemcpyAsync(r->sect.data(), sect.p, (size_t)NL * sizeof(CsectAcc), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(r->start.data(), c->loop_start.p, (size_t)(NL + 1) * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(r->layer.data(), c->loop_layer.p, (size_t)NL * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&h_maxbits, maxbits.p, 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    r->ms = job.ms(0, 1);
  }
  r->e = exponent_of(h_maxbits);
  return GSDF_OK;
}
}  // namespace
extern "C" double gsdf_hip_contour_measures_ms(void) { return g_measures_ms; }
extern "C" double gsdf_hip_contour_sections_ms(void) { return g_sections_ms; }

extern "C" int gsdf_hip_contour_measures(const gsdf_contour* c, gsdf_loop_measure* loops, gsdf_layer_measure* layers) {
  if (!c) return fail(GSDF_ERR_BAD_ARGUMENT, "null contour");
  g_measures_ms = 0;
  const uint64_t NL = c->n_loops;
  const uint32_t L = c->st.n_layers;
  const float inf = std::numeric_limits<float>::infinity();
  MeasureRun run;
  if (int rc = measure_run(c, false, &run)) return rc;
  g_measures_ms = run.ms;
  // integers -> float64 with one rounding each, times the inverse power of two (exact); area = sum / 2
  const int e = run.e;
  const std::vector<unsigned>&h_start = run.start, &h_layer = run.layer;
  struct LayerAcc { __int128 area = 0, length = 0; unsigned bb[4] = {CMEAS_BB_MIN_INIT, CMEAS_BB_MIN_INIT, CMEAS_BB_MAX_INIT, CMEAS_BB_MAX_INIT}; uint32_t n_loops = 0, n_verts = 0; };
  std::vector<LayerAcc> la(layers ? L : 0);
  for (uint64_t q = 0; q < NL; q++) {
    const CmeasAcc& a = run.acc[q];
    const __int128 area = mass::whole(a.sum[0], a.sum[1]), length = mass::whole(a.sum[2], a.sum[3]);
    if (loops) {
      gsdf_loop_measure& m = loops[q];
      m.area = mass::value(area, 62 - 2 * e);
      m.length = mass::value(length, 60 - e);
      for (int k = 0; k < 4; k++) m.bbox[k] = unordered(a.bb[k]);
      m.n_verts = h_start[q + 1] - h_start[q];
      m.layer = h_layer[q];
    }
    if (layers && h_layer[q] < L) {
      LayerAcc& l = la[h_layer[q]];
      l.area += area;
      l.length += length;
      for (int k = 0; k < 2; k++) {
        l.bb[k] = std::min(l.bb[k], a.bb[k]);
        l.bb[2 + k] = std::max(l.bb[2 + k], a.bb[2 + k]);
      }
      l.n_loops++;
      l.n_verts += h_start[q + 1] - h_start[q];
    }
  }
  if (layers)
    for (uint32_t l = 0; l < L; l++) {
      gsdf_layer_measure& m = layers[l];
      m.area = mass::value(la[l].area, 62 - 2 * e);
      m.length = mass::value(la[l].length, 60 - e);
      for (int k = 0; k < 4; k++) m.bbox[k] = la[l].n_loops ? unordered(la[l].bb[k]) : (k < 2 ? inf : -inf);
      m.n_loops = la[l].n_loops;
      m.n_verts = la[l].n_verts;
    }
  return GSDF_OK;
}

// ---- section properties (gsdf_hip.h, "contours: section properties"; kernels_mass.h, mass_host.h) -----------------------------------
extern "C" int gsdf_hip_contour_sections(const gsdf_contour* c, gsdf_section* loops, gsdf_section* layers) {
  g_sections_ms = 0;
  if (!c) return fail(GSDF_ERR_BAD_ARGUMENT, "null contour");
  const uint64_t NL = c->n_loops;
  const uint32_t L = c->st.n_layers;
  MeasureRun run;
  if (int rc = measure_run(c, true, &run)) return rc;
  g_sections_ms = run.ms;
  struct LayerAcc { __int128 sums[6] = {0, 0, 0, 0, 0, 0}; uint32_t n_loops = 0, n_verts = 0; };
  std::vector<LayerAcc> la(layers ? L : 0);
  for (uint64_t q = 0; q < NL; q++) {
    __int128 sums[6];
    sums[0] = mass::whole(run.acc[q].sum[0], run.acc[q].sum[1]);
    for (int k = 0; k < 5; k++) sums[1 + k] = mass::whole(run.sect[q].sum[2 * k], run.sect[q].sum[2 * k + 1]);
    const uint32_t nv = run.start[q + 1] - run.start[q];
    if (loops) mass::fill_section(&loops[q], sums, run.e, nv, run.layer[q]);
    if (layers && run.layer[q] < L) {
      LayerAcc& l = la[run.layer[q]];
      for (int k = 0; k < 6; k++) l.sums[k] += sums[k];
      l.n_loops++;
      l.n_verts += nv;
    }
  }
  if (layers)
    for (uint32_t l = 0; l < L; l++) mass::fill_section(&layers[l], la[l].sums, run.e, la[l].n_verts, la[l].n_loops);
  return GSDF_OK;
}

// ---- hatch fill (gsdf_hip.h, "contours: hatch fill"; kernels_hatch.h) ---------------------------------------------------------------
struct gsdf_hatch {
  int device = 0;
  uint32_t n_layers = 0;
  uint64_t n_segments = 0;
  DevPtr<float> seg;  // 4 n_segments
  DevPtr<int> line;   // n_segments
  std::vector<uint32_t> layer_start;  // n_layers + 1
  std::vector<gsdf_hatch_layer> layers;
  // a skin handle (gsdf_hip_contour_hatch_skin) only: every segment's class, the layers' records by class
  bool has_classes = false;
  DevPtr<unsigned char> cls;  // n_segments
  std::vector<gsdf_skin_layer> skin_layers;
};

extern "C" void gsdf_hip_hatch_destroy(gsdf_hatch* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  delete h;
}

namespace {
struct HatchDelete { void operator()(gsdf_hatch* h) const { gsdf_hip_hatch_destroy(h); } };
using HatchPtr = std::unique_ptr<gsdf_hatch, HatchDelete>;

// a handle of n_layers layers without a segment: host records only, the segments' buffers come with their count
int hatch_new(int device, uint32_t n_layers, bool with_classes, HatchPtr* out) {
  HatchPtr h(new (std::nothrow) gsdf_hatch());
  if (!h) return fail(GSDF_ERR_BAD_ARGUMENT, "out of memory");
  h->device = device;
  h->n_layers = n_layers;
  h->layer_start.assign((size_t)n_layers + 1, 0u);
  h->layers.assign(n_layers, gsdf_hatch_layer{0.0, 0, 0, -1});
  h->has_classes = with_classes;
  if (with_classes) h->skin_layers.assign(n_layers, gsdf_skin_layer{});
  *out = std::move(h);
  return GSDF_OK;
}

struct HatchWs {
  DevPtr<unsigned long long> maxbits, total;
  DevPtr<unsigned> loop_of, cnt, edge_off, blk_cnt, blk_base;
  DevPtr<int> k_first, layer_kmin, rec_k;
  DevPtr<HatchLayerAcc> acc;
  DevPtr<HatchCounters> ctr;
  DevPtr<unsigned> slot_base, line_cnt, line_start, cursor, cross_edge, cross_slot, rec_j, rec_slot, layer_start;
  DevPtr<double> rec_u, u_sorted;
  DevPtr<float> rec_xy;
};
thread_local double g_hatch_rank_ms = 0;

// ---- what gsdf_hip_contour_hatch and gsdf_hip_contour_hatch_skin share: the options' checks, the exponent, the layers' own lines
int hatch_params(const gsdf_hatch_opts* o, const void* out, HatchParams* P_out) {
  if (!std::isfinite(o->spacing) || !(o->spacing > 0.f)) return fail(GSDF_ERR_BAD_ARGUMENT, "hatch: spacing must be finite and positive");
  if (!std::isfinite(o->offset)) return fail(GSDF_ERR_BAD_ARGUMENT, "hatch: offset must be finite");
  if (o->n_dirs == 0 || o->n_dirs > 4) return fail(GSDF_ERR_BAD_ARGUMENT, "hatch: n_dirs must be 1 .. 4");
  for (uint32_t d = 0; d < o->n_dirs; d++) {
    const float dx = o->dir[d][0], dy = o->dir[d][1];
    if (!std::isfinite(dx) || !std::isfinite(dy) || !(std::fabs(dx) <= 1.f) || !(std::fabs(dy) <= 1.f) || (dx == 0.f && dy == 0.f))
      return fail(GSDF_ERR_BAD_ARGUMENT, "hatch: dir " + std::to_string(d) + " must be finite, within [-1, 1] and not (0, 0)");
  }
  if (!out && o->dry == 0) return fail(GSDF_ERR_BAD_ARGUMENT, "hatch: out may be null in a dry run only");
  HatchParams P{};
  P.offset = (double)o->offset;
  P.spacing = (double)o->spacing;
  const float(*dir)[2] = o->dir;
  P.dx0 = dir[0][0]; P.dy0 = dir[0][1];
  P.dx1 = dir[1 % o->n_dirs][0]; P.dy1 = dir[1 % o->n_dirs][1];
  P.dx2 = dir[2 % o->n_dirs][0]; P.dy2 = dir[2 % o->n_dirs][1];
  P.dx3 = dir[3 % o->n_dirs][0]; P.dy3 = dir[3 % o->n_dirs][1];
  P.n_dirs = o->n_dirs;
  *P_out = P;
  return GSDF_OK;
}

bool hatch_too_small(const HatchParams& P, int e) { return (std::ldexp(1.0, e + 1) + std::fabs(P.offset)) / P.spacing >= 536870912.0; }
const char* const kHatchSmallText = "hatch: spacing is too small for these coordinates ((2^(e+1) + |offset|) / spacing must stay below 2^29)";
const char* const kHatchNoMem = "hatch: no device memory for the workspace";
const char* const kSkinNoMem = "skin: no device memory for the workspace";

// What both entry points open with. The caller declares it first: an unfinished handle goes behind the call's workspace and stream.
struct HatchOpening {
  HatchParams P{};
  HatchPtr h;          // n_layers empty layers
  bool loops = false;  // the handle has loops: the job is open and what follows is set
  int e = 0;
  std::vector<HatchLayerAcc> own;   // the layers' own line ranges (k_min > k_max: none)
  std::vector<unsigned> slot_base;  // the layers' line slots (layer, k - k_min) behind one another
  std::vector<int> k_min;
  uint64_t n_slots = 0, n_own = 0;  // line slots, own crossings
};

// Steps 0 and 1 of a hatch on the job's stream (events 0 and 1; w.maxbits is the caller's): the exponent and the one argument check that
// needs it; every edge's lines (k_first, cnt, edge_off), the layers' line ranges, the crossings of the call. Waits for the stream.
int hatch_ranges(const gsdf_contour* c, Job& job, HatchWs& w, HatchOpening* a, double* ms) {
  const uint64_t V = c->n_verts, NL = c->n_loops;
  const uint32_t L = c->st.n_layers;
  hipStream_t s = job.s;
  // 0. the exponent; the one argument check that needs it
  const unsigned nb = blocks_of(V);
  unsigned long long h_maxbits = 0;
  HIP_TRY(hipEventRecord(job.ev[0], s));
  if (int rc = maxbits_enqueue(c, w.maxbits.p, s)) return rc;
  HIP_TRY(hipEventRecord(job.ev[1], s));
  HIP_TRY(hipMemcpyAsync(&h_maxbits, w.maxbits.p, 8, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *ms += job.ms(0, 1);
  a->e = exponent_of(h_maxbits);
  if (hatch_too_small(a->P, a->e)) return fail(GSDF_ERR_BAD_ARGUMENT, kHatchSmallText);
  // 1. every edge's lines, the layers' line ranges, the edges' offsets
  if (!dev_alloc(w.loop_of, V) || !dev_alloc(w.k_first, V) || !dev_alloc(w.cnt, V) || !dev_alloc(w.edge_off, V + 1) || !dev_alloc(w.blk_cnt, nb) ||
      !dev_alloc(w.blk_base, nb) || !dev_alloc(w.total, 1) || !dev_alloc(w.acc, L) || !dev_alloc(w.ctr, 1) || !dev_alloc(w.slot_base, (uint64_t)L + 1) ||
      !dev_alloc(w.layer_kmin, L) || !dev_alloc(w.layer_start, (uint64_t)L + 1))
    return fail(GSDF_ERR_HIP, kHatchNoMem);
  a->own.assign(L, HatchLayerAcc{});
  HatchCounters h_ctr{};
  HIP_TRY(hipEventRecord(job.ev[0], s));
  HIP_TRY(hipMemsetAsync(w.ctr.p, 0, sizeof(HatchCounters), s));
  LAUNCH(hatch_init_kernel, blocks_of(L), s, w.acc.p, (unsigned)L);
  LAUNCH(cloop_of_kernel, nb, s, c->loop_start.p, (unsigned)NL, (unsigned)V, w.loop_of.p);
  LAUNCH(hatch_range_kernel, nb, s, c->xy.p, c->loop_start.p, w.loop_of.p, c->loop_layer.p, (unsigned)V, (unsigned)L, a->P, w.k_first.p, w.cnt.p, w.blk_cnt.p, w.acc.p, w.ctr.p);
  if (int rc = scan_offsets(w.cnt.p, V, w.blk_cnt.p, w.blk_base.p, w.total.p, w.edge_off.p, s)) return rc;
  HIP_TRY(hipEventRecord(job.ev[1], s));
  HIP_TRY(hipMemcpyAsync(&h_ctr, w.ctr.p, sizeof h_ctr, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(a->own.data(), w.acc.p, (size_t)L * sizeof(HatchLayerAcc), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  *ms += job.ms(0, 1);
  if (h_ctr.bad) return fail(GSDF_ERR_HIP, "hatch: internal error (a loop names a layer the handle does not have)");
  a->n_own = h_ctr.n_crossings;
  if (h_ctr.n_crossings >= ((uint64_t)1 << 32)) return fail(GSDF_ERR_CAPACITY, "hatch: 2^32 crossings or more");
  return GSDF_OK;
}

// In this order: the options' checks (k: the skin's, or null), the handle, the device; a handle without loops is held to the smallest
// exponent, otherwise the job opens, w.maxbits comes, hatch_ranges runs (device time added to *ms) and the layers get their slots. A
// plain hatch's layers take their own line range here (a skin's take the range of their pieces, later).
int hatch_open(const gsdf_contour* c, const gsdf_hatch_opts* o, const gsdf_skin_opts* k, const void* out, Job& job, HatchWs& w, HatchOpening* a, double* ms) {
  if (int rc = hatch_params(o, out, &a->P)) return rc;
  if (k && (k->below > SKIN_MAX_WINDOW || k->above > SKIN_MAX_WINDOW)) return fail(GSDF_ERR_BAD_ARGUMENT, "skin: below and above must be 0 .. 8");
  const uint32_t L = c->st.n_layers;
  if (int rc = hatch_new(c->device, L, k != nullptr, &a->h)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if (c->n_verts == 0 || c->n_loops == 0) return hatch_too_small(a->P, -125) ? fail(GSDF_ERR_BAD_ARGUMENT, kHatchSmallText) : GSDF_OK;
  a->loops = true;
  if (int rc = job.open()) return rc;
  if (!dev_alloc(w.maxbits, 1)) return fail(GSDF_ERR_HIP, k ? kSkinNoMem : kHatchNoMem);
  if (int rc = hatch_ranges(c, job, w, a, ms)) return rc;
  a->slot_base.assign((size_t)L + 1, 0u);
  a->k_min.assign(L, 0);
  uint64_t S = 0;
  for (uint32_t l = 0; l < L; l++) {
    const HatchLayerAcc& r = a->own[l];
    a->slot_base[l] = (unsigned)S;
    if (r.k_min <= r.k_max) {
      a->k_min[l] = r.k_min;
      S += (uint64_t)((int64_t)r.k_max - (int64_t)r.k_min + 1);
      if (!k) a->h->layers[l].k_min = r.k_min, a->h->layers[l].k_max = r.k_max;
    }
    if (S >= ((uint64_t)1 << 31)) return fail(GSDF_ERR_CAPACITY, "hatch: 2^31 line slots or more");
  }
  a->slot_base[L] = (unsigned)S;
  a->n_slots = S;
  return GSDF_OK;
}

// The tail of both: fixed-point sums of segment lengths (two words each: low 32 bits summed, the signed rest summed) added up as
// integers, then float64 at exponent e with one rounding, times the inverse power of two (exact).
struct LengthSum {
  __int128 t = 0;
  LengthSum& add(const unsigned long long sum[2]) { t += mass::whole(sum[0], sum[1]); return *this; }
  double at(int e) const { return mass::value(t, 58 - e); }
};
}  // namespace
extern "C" double gsdf_hip_hatch_rank_ms(void) { return g_hatch_rank_ms; }

extern "C" int gsdf_hip_contour_hatch(const gsdf_contour* c, const gsdf_hatch_opts* o, gsdf_hatch** out, gsdf_hatch_stats* st_out) {
  if (out) *out = nullptr;
  g_hatch_rank_ms = 0;
  if (!c || !o) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  const uint64_t V = c->n_verts;
  const uint32_t L = c->st.n_layers;
  gsdf_hatch_stats st{};
  st.n_layers = L;
  HatchOpening a;
  Stream stream;
  HatchWs w;
  Job job(stream);
  if (int rc = hatch_open(c, o, nullptr, out, job, w, &a, &st.ms_device)) return rc;
  gsdf_hatch* h = a.h.get();
  const HatchParams& P = a.P;
  const uint64_t N = a.n_own, S = a.n_slots;
  if (N > 0) {
    hipStream_t s = job.s;
    std::vector<HatchLayerAcc>& h_acc = a.own;  // (the ranges are used up: the layers' sums come into it)
    HatchCounters h_ctr{};
    if ((N & 1) || S == 0) return fail(GSDF_ERR_HIP, "hatch: internal error (an odd number of crossings)");
    const uint64_t NS = N / 2;
    // 2. crossings per line slot, the buckets' starts
    const unsigned nb_x = blocks_of(N), nb_s = blocks_of(S);
    if (!dev_alloc(w.line_cnt, S) || !dev_alloc(w.line_start, S + 1) || !dev_alloc(w.cursor, S) || !dev_alloc(w.cross_edge, N) || !dev_alloc(w.cross_slot, N) ||
        !dev_alloc(w.blk_cnt, nb_s) || !dev_alloc(w.blk_base, nb_s) || !dev_alloc(w.rec_u, N) || !dev_alloc(w.rec_j, N) || !dev_alloc(w.rec_xy, 2 * N) ||
        !dev_alloc(w.rec_slot, N) || !dev_alloc(w.rec_k, N) || !dev_alloc(w.u_sorted, N))
      return fail(GSDF_ERR_HIP, kHatchNoMem);
    if (!dev_alloc(h->seg, 4 * NS) || !dev_alloc(h->line, NS)) return fail(GSDF_ERR_HIP, "hatch: no device memory for the result");
    HIP_TRY(hipMemcpyAsync(w.slot_base.p, a.slot_base.data(), ((size_t)L + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(w.layer_kmin.p, a.k_min.data(), (size_t)L * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(job.ev[2], s));
    HIP_TRY(hipMemsetAsync(w.line_cnt.p, 0, (size_t)S * 4, s));
    HIP_TRY(hipMemsetAsync(w.cursor.p, 0, (size_t)S * 4, s));
    HIP_TRY(hipMemsetAsync(w.rec_slot.p, 0xff, (size_t)N * 4, s));
    LAUNCH(hatch_count_kernel, nb_x, s, w.edge_off.p, (unsigned)V, w.k_first.p, w.loop_of.p, c->loop_layer.p, w.slot_base.p, w.layer_kmin.p, (unsigned)L, (unsigned)S, (unsigned)N,
           w.cross_edge.p, w.cross_slot.p, w.line_cnt.p, w.ctr.p);
    LAUNCH(hatch_lines_kernel, nb_s, s, w.line_cnt.p, (unsigned)S, w.blk_cnt.p, w.ctr.p);
    if (int rc = scan_offsets(w.line_cnt.p, S, w.blk_cnt.p, w.blk_base.p, w.total.p, w.line_start.p, s)) return rc;
    // 3. records into their buckets, 4. each to its rank; the layers' starts and lengths
    LAUNCH(hatch_emit_kernel, nb_x, s, c->xy.p, c->loop_start.p, w.loop_of.p, c->loop_layer.p, P, w.edge_off.p, w.k_first.p, w.cross_edge.p, w.cross_slot.p, w.line_start.p,
           (unsigned)S, (unsigned)N, w.cursor.p, w.rec_u.p, w.rec_j.p, w.rec_xy.p, w.rec_slot.p, w.rec_k.p, w.ctr.p);
    HIP_TRY(hipEventRecord(job.ev[3], s));
    LAUNCH(hatch_rank_kernel, nb_x, s, w.rec_u.p, w.rec_j.p, w.rec_xy.p, w.rec_slot.p, w.rec_k.p, w.line_start.p, (unsigned)S, (unsigned)N, h->seg.p, h->line.p, w.u_sorted.p,
           w.ctr.p);
    HIP_TRY(hipEventRecord(job.ev[4], s));
    LAUNCH(hatch_layer_start_kernel, blocks_of((uint64_t)L + 1), s, w.line_start.p, w.slot_base.p, (unsigned)L, w.layer_start.p);
    LAUNCH(hatch_length_kernel, blocks_of(NS), s, w.u_sorted.p, (const unsigned*)h->seg.p, w.layer_start.p, (unsigned)L, (unsigned)NS, w.maxbits.p, w.acc.p, w.ctr.p);
    HIP_TRY(hipEventRecord(job.ev[5], s));
    HIP_TRY(hipMemcpyAsync(&h_ctr, w.ctr.p, sizeof h_ctr, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_acc.data(), w.acc.p, (size_t)L * sizeof(HatchLayerAcc), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h->layer_start.data(), w.layer_start.p, ((size_t)L + 1) * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    st.ms_device += job.ms(2, 3) + job.ms(3, 4) + job.ms(4, 5);
    g_hatch_rank_ms = job.ms(3, 4);
    if (h_ctr.bad || h->layer_start[L] != NS) return fail(GSDF_ERR_HIP, "hatch: internal error (a line with an odd number of crossings, or a record out of range)");
    h->n_segments = NS;
    st.n_segments = NS;
    st.n_crossings = N;
    st.n_lines = h_ctr.n_lines;
    st.max_line_crossings = h_ctr.max_line;
    st.zero_length = h_ctr.zero_length;
    LengthSum all;
    for (uint32_t l = 0; l < L; l++) {
      all.add(h_acc[l].sum);
      h->layers[l].length = LengthSum().add(h_acc[l].sum).at(a.e);
      h->layers[l].n_segments = h->layer_start[l + 1] - h->layer_start[l];
    }
    st.length = all.at(a.e);
  }
  if (st_out) *st_out = st;
  if (o->dry == 0) *out = a.h.release();
  return GSDF_OK;
}

// ---- skin classification of the hatch (gsdf_hip.h, "contours: skin classification of the hatch"; kernels_skin.h) --------------------
namespace {
struct SkinWs {
  HatchWs own;  // the hatch's range pass: the exponent, loop_of, the layers' own line ranges
  DevPtr<int> layer_kmax, k_first, rec_k;
  DevPtr<unsigned> cnt, pair_off, blk_cnt, blk_base, blk_cnt2, blk_base2;
  DevPtr<unsigned> line_cnt, own_cnt, line_start, cursor, cross_pair, cross_slot, rec_slot, bnd_off, piece_off, bnd_pos;
  DevPtr<SkinLayerAcc> acc;
  DevPtr<SkinCounters> ctr;
  DevPtr<SkinRec> rec;
  DevPtr<float> rec_xy, xy_sorted;
  DevPtr<double> u_sorted;
  DevPtr<unsigned char> flag;
};
thread_local double g_skin_rank_ms = 0;
}  // namespace
extern "C" double gsdf_hip_skin_rank_ms(void) { return g_skin_rank_ms; }

extern "C" int gsdf_hip_contour_hatch_skin(const gsdf_contour* c, const gsdf_hatch_opts* o, const gsdf_skin_opts* k, gsdf_hatch** out, gsdf_skin_stats* st_out) {
  if (out) *out = nullptr;
  g_skin_rank_ms = 0;
  if (!c || !o || !k) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  const uint64_t V = c->n_verts;
  const uint32_t L = c->st.n_layers;
  gsdf_skin_stats st{};
  st.n_layers = L;
  st.below = k->below;
  st.above = k->above;
  HatchOpening a;
  Stream stream;
  SkinWs w;
  Job job(stream);
  // 0, 1. the exponent and the layers' own line ranges: the hatch's range pass
  if (int rc = hatch_open(c, o, k, out, job, w.own, &a, &st.ms_device)) return rc;
  gsdf_hatch* h = a.h.get();
  const HatchParams& P = a.P;
  SkinParams K{};
  K.below = k->below;
  K.above = k->above;
  K.n_src = 1u + k->below + k->above;
  K.need_below = ((1u << k->below) - 1u) << 1;
  K.need_above = ((1u << k->above) - 1u) << (1u + k->below);
  const uint64_t n_own = a.n_own, S = a.n_slots, n_pairs = V * K.n_src;
  if (a.loops && n_pairs >= ((uint64_t)1 << 32)) return fail(GSDF_ERR_CAPACITY, "skin: 2^32 (edge, source layer) pairs or more");
  if (n_own > 0) {
    hipStream_t s = job.s;
    const int e = a.e;
    const char* nomem = kSkinNoMem;
    std::vector<int> h_kmax(L, -1);
    for (uint32_t l = 0; l < L; l++)
      if (a.own[l].k_min <= a.own[l].k_max) h_kmax[l] = a.own[l].k_max;
    if ((n_own & 1) || S == 0) return fail(GSDF_ERR_HIP, "skin: internal error (an odd number of crossings)");
    // 2. every (edge, source number)'s lines inside the target's own range, their offsets
    const unsigned nb_p = blocks_of(n_pairs), nb_s = blocks_of(S);
    if (!dev_alloc(w.layer_kmax, L) || !dev_alloc(w.k_first, n_pairs) || !dev_alloc(w.cnt, n_pairs) || !dev_alloc(w.pair_off, n_pairs + 1) || !dev_alloc(w.blk_cnt, nb_p) ||
        !dev_alloc(w.blk_base, nb_p) || !dev_alloc(w.acc, L) || !dev_alloc(w.ctr, 1))
      return fail(GSDF_ERR_HIP, nomem);
    SkinCounters h_ctr{};
    HIP_TRY(hipMemcpyAsync(w.own.slot_base.p, a.slot_base.data(), ((size_t)L + 1) * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(w.own.layer_kmin.p, a.k_min.data(), (size_t)L * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipMemcpyAsync(w.layer_kmax.p, h_kmax.data(), (size_t)L * 4, hipMemcpyHostToDevice, s));
    HIP_TRY(hipEventRecord(job.ev[0], s));
    HIP_TRY(hipMemsetAsync(w.ctr.p, 0, sizeof(SkinCounters), s));
    LAUNCH(skin_init_kernel, blocks_of(L), s, w.acc.p, (unsigned)L);
    LAUNCH(skin_range_kernel, nb_p, s, c->xy.p, c->loop_start.p, w.own.loop_of.p, c->loop_layer.p, (unsigned)V, (unsigned)L, P, K, w.own.layer_kmin.p, w.layer_kmax.p, w.k_first.p,
           w.cnt.p, w.blk_cnt.p, w.ctr.p);
    if (int rc = scan_offsets(w.cnt.p, n_pairs, w.blk_cnt.p, w.blk_base.p, w.own.total.p, w.pair_off.p, s)) return rc;
    HIP_TRY(hipEventRecord(job.ev[1], s));
    HIP_TRY(hipMemcpyAsync(&h_ctr, w.ctr.p, sizeof h_ctr, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    st.ms_device += job.ms(0, 1);
    if (h_ctr.bad) return fail(GSDF_ERR_HIP, "skin: internal error (a loop names a layer the handle does not have)");
    const uint64_t N = h_ctr.n_cand;
    if (N >= ((uint64_t)1 << 32)) return fail(GSDF_ERR_CAPACITY, "skin: 2^32 crossings or more");
    if (N < n_own) return fail(GSDF_ERR_HIP, "skin: internal error (fewer crossings than the layers' own)");
    // 3. crossings per line slot (slots without an own crossing emptied), the buckets' starts; 4. records into their buckets
    const unsigned nb_x = blocks_of(N);
    if (!dev_alloc(w.line_cnt, S) || !dev_alloc(w.own_cnt, S) || !dev_alloc(w.line_start, S + 1) || !dev_alloc(w.cursor, S) || !dev_alloc(w.cross_pair, N) ||
        !dev_alloc(w.cross_slot, N) || !dev_alloc(w.blk_cnt, nb_s > nb_x ? nb_s : nb_x) || !dev_alloc(w.blk_base, nb_s > nb_x ? nb_s : nb_x) || !dev_alloc(w.blk_cnt2, nb_x) ||
        !dev_alloc(w.blk_base2, nb_x) || !dev_alloc(w.rec, N) || !dev_alloc(w.rec_xy, 2 * N) || !dev_alloc(w.rec_slot, N) || !dev_alloc(w.rec_k, N) ||
        !dev_alloc(w.u_sorted, N) || !dev_alloc(w.xy_sorted, 2 * N) || !dev_alloc(w.flag, N) || !dev_alloc(w.bnd_off, N) || !dev_alloc(w.piece_off, N + 1) ||
        !dev_alloc(w.bnd_pos, N))
      return fail(GSDF_ERR_HIP, nomem);
    HIP_TRY(hipEventRecord(job.ev[2], s));
    HIP_TRY(hipMemsetAsync(w.line_cnt.p, 0, (size_t)S * 4, s));
    HIP_TRY(hipMemsetAsync(w.own_cnt.p, 0, (size_t)S * 4, s));
    HIP_TRY(hipMemsetAsync(w.cursor.p, 0, (size_t)S * 4, s));
    HIP_TRY(hipMemsetAsync(w.rec_slot.p, 0xff, (size_t)N * 4, s));
    HIP_TRY(hipMemsetAsync(w.flag.p, 0, (size_t)N, s));
    HIP_TRY(hipMemsetAsync(w.piece_off.p, 0, ((size_t)N + 1) * 4, s));
    LAUNCH(skin_count_kernel, nb_x, s, w.pair_off.p, (unsigned)n_pairs, (unsigned)V, w.k_first.p, w.own.loop_of.p, c->loop_layer.p, K, w.own.slot_base.p, w.own.layer_kmin.p,
           (unsigned)L, (unsigned)S, (unsigned)N, w.cross_pair.p, w.cross_slot.p, w.line_cnt.p, w.own_cnt.p, w.ctr.p);
    LAUNCH(skin_lines_kernel, nb_s, s, w.line_cnt.p, w.own_cnt.p, (unsigned)S, w.blk_cnt.p, w.ctr.p);
    if (int rc = scan_offsets(w.line_cnt.p, S, w.blk_cnt.p, w.blk_base.p, w.own.total.p, w.line_start.p, s)) return rc;
    LAUNCH(skin_emit_kernel, nb_x, s, c->xy.p, c->loop_start.p, w.own.loop_of.p, c->loop_layer.p, P, K, (unsigned)V, (unsigned)L, w.pair_off.p, w.k_first.p, w.cross_pair.p,
           w.cross_slot.p, w.line_start.p, (unsigned)S, (unsigned)N, w.cursor.p, w.rec.p, w.rec_xy.p, w.rec_slot.p, w.rec_k.p, w.ctr.p);
    // 5. each record to its rank, the sources' parity around it; 6. boundaries and pieces numbered
    HIP_TRY(hipEventRecord(job.ev[3], s));
    LAUNCH(skin_rank_kernel, nb_x, s, w.rec.p, w.rec_xy.p, w.rec_slot.p, w.line_start.p, (unsigned)S, (unsigned)N, K, w.u_sorted.p, w.xy_sorted.p, w.flag.p, w.ctr.p);
    HIP_TRY(hipEventRecord(job.ev[4], s));
    LAUNCH(skin_flags_kernel, nb_x, s, w.flag.p, w.line_start.p, (unsigned)S, (unsigned)N, w.blk_cnt.p, w.blk_cnt2.p, w.ctr.p);
    if (int rc = launch_block_scan(w.blk_cnt.p, nb_x, w.blk_base.p, w.own.total.p, s)) return rc;
    if (int rc = launch_block_scan(w.blk_cnt2.p, nb_x, w.blk_base2.p, w.own.total.p, s)) return rc;
    LAUNCH(skin_compact_kernel, nb_x, s, w.flag.p, w.line_start.p, (unsigned)S, (unsigned)N, w.blk_base.p, w.blk_base2.p, w.bnd_off.p, w.piece_off.p, w.bnd_pos.p, w.ctr.p);
    LAUNCH(skin_layer_start_kernel, blocks_of((uint64_t)L + 1), s, w.line_start.p, w.own.slot_base.p, w.piece_off.p, (unsigned)L, (unsigned)S, (unsigned)N, w.own.layer_start.p);
    HIP_TRY(hipEventRecord(job.ev[5], s));
    HIP_TRY(hipMemcpyAsync(&h_ctr, w.ctr.p, sizeof h_ctr, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h->layer_start.data(), w.own.layer_start.p, ((size_t)L + 1) * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    st.ms_device += job.ms(2, 3) + job.ms(3, 4) + job.ms(4, 5);
    g_skin_rank_ms = job.ms(3, 4);
    const uint64_t NB = h_ctr.n_bnd, NS = h_ctr.n_pieces;
    if (h_ctr.bad || h_ctr.n_own != n_own || NB > N || NS > NB || h->layer_start[L] != NS)
      return fail(GSDF_ERR_HIP, "skin: internal error (a line with an odd number of crossings, or a record out of range)");
    // 7. the pieces: end points, classes, lengths by (layer, class)
    if (!dev_alloc(h->seg, 4 * NS) || !dev_alloc(h->line, NS) || !dev_alloc(h->cls, NS)) return fail(GSDF_ERR_HIP, "skin: no device memory for the result");
    std::vector<SkinLayerAcc> h_acc(L);
    HIP_TRY(hipEventRecord(job.ev[6], s));
    LAUNCH(skin_piece_kernel, nb_x, s, w.flag.p, w.u_sorted.p, (const unsigned*)w.xy_sorted.p, w.rec_slot.p, w.rec_k.p, w.line_start.p, w.own.slot_base.p, (unsigned)L, (unsigned)S,
           (unsigned)N, w.bnd_off.p, w.piece_off.p, w.bnd_pos.p, (unsigned)NB, (unsigned)NS, w.own.maxbits.p, (unsigned*)h->seg.p, h->line.p, h->cls.p, w.acc.p, w.ctr.p);
    HIP_TRY(hipEventRecord(job.ev[7], s));
    HIP_TRY(hipMemcpyAsync(&h_ctr, w.ctr.p, sizeof h_ctr, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_acc.data(), w.acc.p, (size_t)L * sizeof(SkinLayerAcc), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    st.ms_device += job.ms(6, 7);
    if (h_ctr.bad) return fail(GSDF_ERR_HIP, "skin: internal error (a line that does not end outside, or a piece out of range)");
    h->n_segments = NS;
    st.n_segments = NS;
    st.n_crossings = h_ctr.n_crossings;
    st.n_own_crossings = h_ctr.n_own;
    st.n_lines = h_ctr.n_lines;
    st.max_line_crossings = h_ctr.max_line;
    st.zero_length = h_ctr.zero_length;
    LengthSum all[4];
    for (uint32_t l = 0; l < L; l++) {
      LengthSum layer;
      uint64_t layer_n = 0;
      for (int q = 0; q < 4; q++) {
        all[q].add(h_acc[l].sum[q]);
        layer.add(h_acc[l].sum[q]);
        layer_n += h_acc[l].n[q];
        st.n_class[q] += h_acc[l].n[q];
        h->skin_layers[l].length[q] = LengthSum().add(h_acc[l].sum[q]).at(e);
        h->skin_layers[l].n_segments[q] = h_acc[l].n[q];
      }
      if (layer_n != (uint64_t)h->layer_start[l + 1] - h->layer_start[l]) return fail(GSDF_ERR_HIP, "skin: internal error (a layer's pieces and its classes' counts differ)");
      h->layers[l].length = layer.at(e);
      h->layers[l].n_segments = layer_n;
      if (h_acc[l].k_min <= h_acc[l].k_max) {
        h->layers[l].k_min = h_acc[l].k_min;
        h->layers[l].k_max = h_acc[l].k_max;
      }
    }
    for (int q = 0; q < 4; q++) st.length[q] = all[q].at(e);
  }
  if (st_out) *st_out = st;
  if (o->dry == 0) *out = a.h.release();
  return GSDF_OK;
}

extern "C" int gsdf_hip_hatch_read_skin(const gsdf_hatch* h, uint8_t* cls, gsdf_skin_layer* layers) {
  if (!h) return fail(GSDF_ERR_BAD_ARGUMENT, "null hatch");
  if (!h->has_classes) return fail(GSDF_ERR_BAD_ARGUMENT, "this handle has no classes (it was made by gsdf_hip_contour_hatch)");
  HIP_TRY(hipSetDevice(h->device));
  if (cls && h->n_segments) HIP_TRY(hipMemcpy(cls, h->cls.p, (size_t)h->n_segments, hipMemcpyDeviceToHost));
  if (layers && h->n_layers) std::memcpy(layers, h->skin_layers.data(), (size_t)h->n_layers * sizeof(gsdf_skin_layer));
  return GSDF_OK;
}

extern "C" int gsdf_hip_hatch_counts(const gsdf_hatch* h, uint32_t* n_layers, uint64_t* n_segments) {
  if (!h) return fail(GSDF_ERR_BAD_ARGUMENT, "null hatch");
  if (n_layers) *n_layers = h->n_layers;
  if (n_segments) *n_segments = h->n_segments;
  return GSDF_OK;
}

extern "C" int gsdf_hip_hatch_read(const gsdf_hatch* h, float* seg, int32_t* line, uint32_t* layer_start, gsdf_hatch_layer* layers) {
  if (!h) return fail(GSDF_ERR_BAD_ARGUMENT, "null hatch");
  HIP_TRY(hipSetDevice(h->device));
  if (seg && h->n_segments) HIP_TRY(hipMemcpy(seg, h->seg.p, (size_t)h->n_segments * 16, hipMemcpyDeviceToHost));
  if (line && h->n_segments) HIP_TRY(hipMemcpy(line, h->line.p, (size_t)h->n_segments * 4, hipMemcpyDeviceToHost));
  if (layer_start) std::memcpy(layer_start, h->layer_start.data(), h->layer_start.size() * 4);
  if (layers && h->n_layers) std::memcpy(layers, h->layers.data(), (size_t)h->n_layers * sizeof(gsdf_hatch_layer));
  return GSDF_OK;
}

// ---- offset (gsdf_hip.h, "contours: offset"; kernels_offset.h) ----------------------------------------------------------------------
namespace {
struct OffsetWs {
  DevPtr<unsigned> loop_of, bb, layer_edge;
  DevPtr<float4> edges;
  DevPtr<float> D;
  DevPtr<OffsetCounters> ctr;
};

// what gsdf_hip_contour_offset and gsdf_hip_contour_distance share: the options' checks, the one lattice of the call, the band
struct OffsetPlan {
  ContourLattice lat{};
  uint64_t N = 0;
  float band = 0.f;
  unsigned tiles_x = 0, tiles_y = 0;
  OffsetInsets insets{};
};
const char* const kOffsetNoMem = "offset: no device memory for the workspace";

int offset_check(const gsdf_offset_opts* o) {
  if (!std::isfinite(o->res) || !(o->res > 0.f)) return fail(GSDF_ERR_BAD_ARGUMENT, "offset: res must be finite and positive");
  if (o->n_insets == 0 || o->n_insets > OFFSET_MAX_INSETS) return fail(GSDF_ERR_BAD_ARGUMENT, "offset: n_insets must be 1 .. 8");
  for (uint32_t i = 0; i < o->n_insets; i++)
    if (!std::isfinite(o->inset[i])) return fail(GSDF_ERR_BAD_ARGUMENT, "offset: inset " + std::to_string(i) + " is not finite");
  if (o->reserved != 0) return fail(GSDF_ERR_BAD_ARGUMENT, "offset: reserved must be 0");
  return GSDF_OK;
}

// The lattice (the handle's exact box grown for the negative insets, then the tracer's rules) and the handle's edges on s: ws.edges in
// vertex order, ws.layer_edge the first edge of every layer. Waits for s.
int offset_prepare(const gsdf_contour* c, const gsdf_offset_opts* o, hipStream_t s, OffsetWs& ws, OffsetPlan* plan) {
  const uint64_t V = c->n_verts, NL = c->n_loops;
  const uint32_t L = c->st.n_layers;
  float box[4] = {0.f, 0.f, 0.f, 0.f};  // (a handle without vertices: the origin)
  if (V > 0) {
    const unsigned init[4] = {0xffffffffu, 0xffffffffu, 0u, 0u};
    unsigned h_bb[4];
    if (!dev_alloc(ws.bb, 4)) return fail(GSDF_ERR_HIP, kOffsetNoMem);
    HIP_TRY(hipMemcpyAsync(ws.bb.p, init, sizeof init, hipMemcpyHostToDevice, s));
    LAUNCH(offset_bbox_kernel, blocks_of(V), s, c->xy.p, (unsigned)V, ws.bb.p);
    HIP_TRY(hipMemcpyAsync(h_bb, ws.bb.p, sizeof h_bb, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (int k = 0; k < 4; k++) box[k] = unordered(h_bb[k]);
  }
  float grow = 0.f, reach = 0.f;
  for (uint32_t i = 0; i < o->n_insets; i++) {
    grow = std::max(grow, -o->inset[i]);
    reach = std::max(reach, std::fabs(o->inset[i]));
    plan->insets.v[i] = o->inset[i];
  }
  const float res = o->res;
  const float lo_x = box[0] - grow, lo_y = box[1] - grow, hi_x = box[2] + grow, hi_y = box[3] + grow;
  if (!std::isfinite(lo_x) || !std::isfinite(lo_y) || !std::isfinite(hi_x) || !std::isfinite(hi_y)) return fail(GSDF_ERR_BAD_ARGUMENT, "offset: the grown bounds are not finite");
  const uint64_t nx = axis_nodes(lo_x, hi_x, res), ny = axis_nodes(lo_y, hi_y, res);
  if (nx == 0 || ny == 0 || nx * ny >= ((uint64_t)1 << 31)) return fail(GSDF_ERR_BAD_ARGUMENT, "offset: the lattice needs 2^31 nodes or more at this res");
  if (nx * ny * o->n_insets >= ((uint64_t)1 << 31)) return fail(GSDF_ERR_BAD_ARGUMENT, "offset: the lattices of one layer's insets need 2^31 nodes or more at this res");
  plan->lat = ContourLattice{(unsigned)nx, (unsigned)ny, lo_x - res, lo_y - res, res};
  plan->N = nx * ny;
  const float two_res = 2.f * res;
  plan->band = reach + two_res;
  plan->tiles_x = (unsigned)((nx + OFFSET_TILE - 1) / OFFSET_TILE);
  plan->tiles_y = (unsigned)((ny + OFFSET_TILE - 1) / OFFSET_TILE);
  // the layers' edges: a layer's loops, and with them its vertices, are contiguous (loop_layer is non-decreasing)
  std::vector<unsigned> h_start(NL + 1, 0u), h_layer(NL, 0u), h_edge((size_t)L + 1, (unsigned)V);
  if (!dev_alloc(ws.layer_edge, (uint64_t)L + 1) || !dev_alloc(ws.loop_of, V) || !dev_alloc(ws.edges, V)) return fail(GSDF_ERR_HIP, kOffsetNoMem);
  if (V > 0 && NL > 0) {
    HIP_TRY(hipMemcpyAsync(h_start.data(), c->loop_start.p, (size_t)(NL + 1) * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(h_layer.data(), c->loop_layer.p, (size_t)NL * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    uint64_t q = 0;
    for (uint32_t l = 0; l <= L; l++) {
      while (q < NL && h_layer[q] < l) q++;
      h_edge[l] = q < NL ? h_start[q] : (unsigned)V;
    }
    h_edge[L] = (unsigned)V;
    LAUNCH(cloop_of_kernel, blocks_of(V), s, c->loop_start.p, (unsigned)NL, (unsigned)V, ws.loop_of.p);
    LAUNCH(offset_edges_kernel, blocks_of(V), s, c->xy.p, c->loop_start.p, ws.loop_of.p, (unsigned)V, ws.edges.p);
  }
  HIP_TRY(hipMemcpyAsync(ws.layer_edge.p, h_edge.data(), ((size_t)L + 1) * 4, hipMemcpyHostToDevice, s));
  HIP_TRY(hipStreamSynchronize(s));
  return GSDF_OK;
}

void offset_stats_of(const OffsetPlan& plan, const gsdf_offset_opts* o, uint32_t n_layers_in, gsdf_offset_stats* st) {
  st->nx = plan.lat.nx;
  st->ny = plan.lat.ny;
  st->n_layers_in = n_layers_in;
  st->n_insets = o->n_insets;
  st->x0 = plan.lat.x0;
  st->y0 = plan.lat.y0;
  st->band = plan.band;
  st->res = o->res;
}
}  // namespace

extern "C" int gsdf_hip_contour_offset(const gsdf_contour* c, const gsdf_offset_opts* o, gsdf_contour** out, gsdf_offset_stats* st_out) {
  if (out) *out = nullptr;
  if (!c || !o) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (int rc = offset_check(o)) return rc;
  const bool dry = o->dry != 0;
  if (!out && !dry) return fail(GSDF_ERR_BAD_ARGUMENT, "offset: out may be null in a dry run only");
  const uint64_t L_in = c->st.n_layers, K = o->n_insets, L_out = L_in * K;
  if (L_out >= ((uint64_t)1 << 32)) return fail(GSDF_ERR_CAPACITY, "offset: 2^32 output layers or more");

  HIP_TRY(hipSetDevice(c->device));
  gsdf_contour_stats st{};
  Stream stream;
  Tracer t{st};
  OffsetWs ws;
  ContourPtr r;
  Job job(stream);
  if (int rc = job.open()) return rc;
  hipStream_t s = job.s;
  OffsetPlan plan;
  if (int rc = offset_prepare(c, o, s, ws, &plan)) return rc;
  const ContourLattice& lat = plan.lat;
  const uint64_t N = plan.N, tiles = (uint64_t)plan.tiles_x * plan.tiles_y;
  // a chunk is whole input layers, each with all its insets
  t.plan(lat, o->max_nodes ? o->max_nodes : (uint64_t)GSDF_CONTOUR_DEFAULT_MAX_NODES, K, L_in);
  if (!dev_alloc(ws.D, t.per_chunk * N) || !dev_alloc(ws.ctr, 1)) return fail(GSDF_ERR_HIP, kOffsetNoMem);
  if (int rc = t.alloc(job, 2, nullptr, 0, kOffsetNoMem)) return rc;
  HIP_TRY(hipMemsetAsync(ws.ctr.p, 0, sizeof(OffsetCounters), s));

  for (uint64_t l0 = 0; l0 < L_in; l0 += t.per_chunk) {
    const uint64_t Lc = L_in - l0 < t.per_chunk ? L_in - l0 : t.per_chunk;
    const uint64_t nodes = Lc * K * N;
    // 1. the field: D of the chunk's input layers, then every inset's lattice where the tracer reads its distances
    HIP_TRY(hipEventRecord(job.ev[0], s));
    const unsigned tile_blocks = (unsigned)(tiles * Lc);  // (tiles <= N: below 2^31 with the chunk's nodes)
    LAUNCH(offset_tile_kernel, tile_blocks, s, lat, ws.edges.p, ws.layer_edge.p, (unsigned)l0, plan.tiles_x, plan.tiles_y, plan.band, ws.D.p, ws.ctr.p);
    LAUNCH(offset_field_kernel, blocks_of(nodes), s, ws.D.p, (unsigned)N, (unsigned)K, plan.insets, (unsigned long long)nodes, t.w.dist.p);
    // 2 .. 5. trace
    if (int rc = t.chunk(job, Lc * K, l0 * K, !dry)) return rc;
  }
  if (int rc = t.finish(job, c->device, dry ? nullptr : &r)) return rc;
  OffsetCounters h_ctr{};
  HIP_TRY(hipMemcpyAsync(&h_ctr, ws.ctr.p, sizeof h_ctr, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (st_out) {
    gsdf_offset_stats os{};
    offset_stats_of(plan, o, (uint32_t)L_in, &os);
    os.n_verts = st.n_verts;
    os.n_loops = st.n_loops;
    os.border_inside = st.border_inside;
    os.saddle_cells = st.saddle_cells;
    os.inside_nodes = h_ctr.inside_nodes;
    os.band_nodes = h_ctr.band_nodes;
    os.ms_field = st.ms_eval;
    os.ms_trace = st.ms_trace;
    os.ms_device = st.ms_device;
    *st_out = os;
  }
  if (!dry) *out = r.release();
  return GSDF_OK;
}

extern "C" int gsdf_hip_contour_distance(const gsdf_contour* c, const gsdf_offset_opts* o, uint32_t layer, float* d_out, gsdf_offset_stats* st_out) {
  if (!c || !o || !d_out) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (int rc = offset_check(o)) return rc;
  if (layer >= c->st.n_layers) return fail(GSDF_ERR_BAD_ARGUMENT, "offset: layer " + std::to_string(layer) + " of a handle with " + std::to_string(c->st.n_layers) + " layers");
  HIP_TRY(hipSetDevice(c->device));
  Stream stream;
  OffsetWs ws;
  Job job(stream);
  if (int rc = job.open()) return rc;
  hipStream_t s = job.s;
  OffsetPlan plan;
  if (int rc = offset_prepare(c, o, s, ws, &plan)) return rc;
  if (!dev_alloc(ws.D, plan.N) || !dev_alloc(ws.ctr, 1)) return fail(GSDF_ERR_HIP, kOffsetNoMem);
  OffsetCounters h_ctr{};
  HIP_TRY(hipMemsetAsync(ws.ctr.p, 0, sizeof(OffsetCounters), s));
  HIP_TRY(hipEventRecord(job.ev[0], s));
  LAUNCH(offset_tile_kernel, plan.tiles_x * plan.tiles_y, s, plan.lat, ws.edges.p, ws.layer_edge.p, (unsigned)layer, plan.tiles_x, plan.tiles_y, plan.band, ws.D.p, ws.ctr.p);
  HIP_TRY(hipEventRecord(job.ev[1], s));
  HIP_TRY(hipMemcpyAsync(d_out, ws.D.p, (size_t)plan.N * 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(&h_ctr, ws.ctr.p, sizeof h_ctr, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (st_out) {
    gsdf_offset_stats os{};
    offset_stats_of(plan, o, c->st.n_layers, &os);
    os.inside_nodes = h_ctr.inside_nodes;
    os.band_nodes = h_ctr.band_nodes;
    os.ms_field = os.ms_device = job.ms(0, 1);
    *st_out = os;
  }
  return GSDF_OK;
}
