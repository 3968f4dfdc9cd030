// abi_mesh.hip -- C ABI (include/gsdf_hip.h), mesher side: glrender.Octree + marchCubes, FlatRenderer and
// DualContourRenderer on device, and the accessors of the resulting mesh (ReadTriangles drain, STL, pinned host views).
// Kernels: kernels_octree.h, kernels_flat.h, kernels_dc.h, kernels_dc_indexed.h, kernels_stl.h, kernels_minecraft.h. Indexed meshes
// (weld, PLY, report, extract) are abi_indexed.hip's; what it takes from here is mesh_march_dense, and what dual contouring's indexed
// entry takes from there is indexed_from_cube_slots.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "kernels_common.h"
#include "kernels_octree.h"
#include "kernels_flat.h"
#include "kernels_dc.h"
#include "kernels_dc_indexed.h"
#include "kernels_stl.h"
#include "kernels_minecraft.h"
#include "abi_program.h"
#include "host_math.h"

// ---- glrender.Octree on device ----------------------------------------------------------------------------------------------
// One mesh = one chain of launches with no host round trip (each kernel reads its input count from the previous one's counter in
// device memory), then one wait. The chain and the wait are two entry points -- gsdf_hip_mesh_octree_start / _wait -- so that a
// caller with several meshes to make enqueues the next chain before it waits for the previous one: the ~30 us between the last
// kernel of a mesh and the first kernel of the next (completion wake-up, the caller's own bookkeeping, launch latency) then pass
// under a running chain instead of an idle GPU. Up to two chains per handle; they run back to back on the handle's stream, so the
// workspace arenas are reused in stream order and only the pinned counter block and the timing events exist twice.
namespace {
constexpr size_t kCtrBytes = (sizeof(MeshCounters) + 255) & ~(size_t)255;  // the group sums follow the counters: one memset clears both
const bool ctr_from_kernel = env_flag_on("GSDF_HIP_CTR_FROM_KERNEL");  // developer knobs (A/B timing)

// The ahead-of-time kernel of a variant: exactly the instantiations this library launches, null for every other. (A per-tree
// build has the same parameters whatever its template arguments: launch_kernel takes their types from these.) The kernels come
// out in the code object in the order they are first named here.
using leaf_eval_kernel_t = decltype(&leaf_eval_kernel<4, 3>);
using leaf_dense_kernel_t = decltype(&leaf_dense_kernel<3, true, false>);
using dc_origin_kernel_t = decltype(&dc_origin_kernel<4, 3>);
using flat_grid_kernel_t = decltype(&flat_grid_kernel<4, 4>);
leaf_dense_kernel_t leaf_dense_aot(int w) {  // passes of four points per lane, scratch-free occupancies only
  if (w == 3) return leaf_dense_kernel<3, true, false>;
  if (w == 2) return leaf_dense_kernel<2, true, false>;
  return nullptr;
}
leaf_eval_kernel_t leaf_eval_aot(const LeafVariant& v) {  // (K, W): gsdf_program::leaf_aot_waves
  struct Row { int k, w; bool ucube, ntlds, dz; leaf_eval_kernel_t f; };
  static const Row rows[] = {
      // distinct z rows: column bricks at four points per lane
      {4, 2, true, true, true, leaf_eval_kernel<4, 2, true, true, false, true>},   {4, 3, true, true, true, leaf_eval_kernel<4, 3, true, true, false, true>},
      {4, 2, true, false, true, leaf_eval_kernel<4, 2, true, false, false, true>}, {4, 3, true, false, true, leaf_eval_kernel<4, 3, true, false, false, true>},
      // a few leaves per pass | a level-3 cube per pass with its case-count table in LDS | in global memory
      {4, 2, false, true, false, leaf_eval_kernel<4, 2, false, true>}, {4, 2, true, true, false, leaf_eval_kernel<4, 2, true, true>}, {4, 2, true, false, false, leaf_eval_kernel<4, 2, true, false>},
      {4, 3, false, true, false, leaf_eval_kernel<4, 3, false, true>}, {4, 3, true, true, false, leaf_eval_kernel<4, 3, true, true>}, {4, 3, true, false, false, leaf_eval_kernel<4, 3, true, false>},
      {2, 3, false, true, false, leaf_eval_kernel<2, 3, false, true>}, {2, 3, true, true, false, leaf_eval_kernel<2, 3, true, true>}, {2, 3, true, false, false, leaf_eval_kernel<2, 3, true, false>},
      {1, 4, false, true, false, leaf_eval_kernel<1, 4, false, true>}, {1, 4, true, true, false, leaf_eval_kernel<1, 4, true, true>}, {1, 4, true, false, false, leaf_eval_kernel<1, 4, true, false>},
  };
  if (v.both) return nullptr;
  for (const Row& r : rows)
    if (r.k == v.k && r.w == v.w && r.ucube == v.ucube && r.ntlds == v.ntlds && r.dz == v.dz) return r.f;
  return nullptr;
}
dc_origin_kernel_t dc_origin_aot(SweepVariant v) {  // (gsdf_program::dc_origin_variant)
  if (v.k == 4 && v.w == 3) return dc_origin_kernel<4, 3>;  // <4, 4> needs scratch: not built (see fn_scratch_bytes)
  if (v.k == 2 && v.w == 3) return dc_origin_kernel<2, 3>;  // (<2, 4> sits at its register budget: with the block verdicts' pointer it spills four VGPRs, and a kernel with scratch is not shipped)
  if (v.k == 1 && v.w == 4) return dc_origin_kernel<1, 4>;
  return nullptr;
}
flat_grid_kernel_t flat_grid_aot(SweepVariant v) {  // (gsdf_program::sweep_variant)
  if (v.k == 4) return v.w == 4 ? flat_grid_kernel<4, 4> : flat_grid_kernel<4, 3>;
  if (v.k == 2) return v.w == 4 ? flat_grid_kernel<2, 4> : flat_grid_kernel<2, 3>;
  return flat_grid_kernel<1, 4>;
}
}  // namespace

struct gsdf_mesh_job {
  gsdf_program* p = nullptr;
  gsdf_mesh* m = nullptr;
  gsdf_mesh_opts opts{};
  float res = 0, ox = 0, oy = 0, oz = 0;
  hipStream_t s = nullptr;
  int levels = 0, lq = 0, ls = 0, prune_cols = 0, pmask = 0, ptest = 0, lk = 0;
  size_t lds_prune = 0, lds_m = 0;
  bool want_recs = false;
  uint64_t qcap = 0, want = 0, want_rec_n = 0;  // capacities of the next attempt
  // the attempt in flight
  int attempt = 0, slot;
  bool ctr_on_host = false, used_dz = false, used_dense = false;
  int chain_first = 0;  // levels <= chain_first were tested by prune_kernel (one launch per level), the ones above speculatively
  uint64_t nblk = 0, nblk_q = 0, lbound = 0;  // 64-leaf blocks the record arena holds / the queue capacity allows for; leaves the latter bounds
  size_t clear_bytes = 0;
  bool masks_valid = false;
  Cube* q[2] = {nullptr, nullptr};  // the cube queues by level parity, and their capacities
  uint64_t capq[2] = {0, 0};
  MeshCounters* d_ctr = nullptr;
  MeshCounters* hcp = nullptr;  // this job's pinned counter block
  hipEvent_t ev_done = nullptr;
  // this job's workspace: the handle has three, so that chains in flight do not share one (they run on streams of their own, the
  // latency-bound top and tail of one under the leaf kernel of the other)
  gsdf_program::OctreeWs& w;
  explicit gsdf_mesh_job(gsdf_program* pp, int sl) : p(pp), slot(sl), w(pp->ws[sl]) {}

  int enqueue();            // one attempt: the whole chain onto the stream, nothing waited for
  int prepare_outputs();    //   its stages: outputs and capacities,
  int enqueue_descent();    //   the speculative top and the per-level chain,
  int enqueue_leaf();       //   the leaf phase,
  int enqueue_handover();   //   the counters' way to the host
  int finish(bool* again);  // waits for it; *again: a capacity was short -- enqueue() once more (nothing was dropped silently)
  int stats();              // the mesh's statistics from the counters
};

int gsdf_mesh_job::enqueue() {
  ctr_on_host = false;
  used_dz = false;
  used_dense = false;
  if (int rc = prepare_outputs()) return rc;
  if (int rc = enqueue_descent()) return rc;  // (ev[0] .. ev[1])
  if (int rc = enqueue_leaf()) return rc;
  HIP_TRY(hipEventRecord(w.ev[2], s));
  return enqueue_handover();
}

int gsdf_mesh_job::prepare_outputs() {
  HIP_TRY(w.q0.ensure(qcap * sizeof(Cube)));
  HIP_TRY(w.q1.ensure(qcap * sizeof(Cube)));
  q[0] = (Cube*)w.q0.p; q[1] = (Cube*)w.q1.p;
  capq[0] = w.q0.cap / sizeof(Cube); capq[1] = w.q1.cap / sizeof(Cube);
  // records payload: room for the packed records instead (sized like the triangles: previous mesh, else a guess + one exact rerun)
  if (want_recs && !m->d_recs) {
    const uint64_t nrec = want_rec_n ? want_rec_n : (p->last_recs ? p->last_recs + p->last_recs / 16 + 1024 : (uint64_t)1 << 20);
    const uint64_t units = (dense_bytes(nrec) + 35) / 36;
    m->d_recs = (uint8_t*)pool_take(p->device, units, &m->recs_cap36);
    if (!m->d_recs) { HIP_TRY(hipMalloc((void**)&m->d_recs, units * 36)); m->recs_cap36 = units; }
  }
  // triangle buffer: caller's size, else a pooled buffer, else a guess that is corrected by one exact rerun
  if (!want_recs && !m->d_tris) {
    uint64_t need = want ? want : (p->last_tris ? p->last_tris + p->last_tris / 16 + 1024 : (uint64_t)1 << 20);
    if (opts.host_output) {
      // triangles straight into pinned host memory: the marching kernel's stores are coalesced bursts, which PCIe takes
      // well; the transfer then overlaps the kernel instead of following it
      void* hb = nullptr;
      size_t hcap = 0;
      if (int rc = host_buf(&hb, &hcap, (size_t)need * 36)) return rc;
      m->d_tris = (float*)hb;
      m->cap = hcap / 36;
      m->host_out = true;
    } else {
      m->d_tris = pool_take(p->device, need, &m->cap);
      if (!m->d_tris) {
        HIP_TRY(hipMalloc((void**)&m->d_tris, need * 36));
        m->cap = need;
      }
    }
  }
  // 64-leaf blocks the queue capacity allows for, and their groups
  lbound = capq[lq & 1] << (3 * (lq - 1));
  {
    const uint64_t full = (levels - lq) * 3 >= 40 ? UINT64_MAX : ((uint64_t)1 << (3 * (levels - 1)));
    if (lbound > full) lbound = full;
  }
  // The record arena (2 560 B per block) is sized for the blocks a mesh of this handle actually had (+ 1/8), not for the queue
  // capacity: a million-cube queue would ask for 2.7 GB, and each queue regrowth for four times more. First mesh: 384 K
  // blocks (1 GB); a mesh that needs more says so through its survivor count and is repeated once with the exact size.
  constexpr uint64_t kRecBlocks0 = (uint64_t)384 << 10;
  nblk_q = (lbound + 63) / 64;
  nblk = p->rec_blocks ? p->rec_blocks : kRecBlocks0;
  if (nblk > nblk_q) nblk = nblk_q;
  const uint64_t ngrp = (nblk + MARCH_GROUP - 1) / MARCH_GROUP;
  const size_t hdr_bytes = nblk * sizeof(uint32_t), rec_bytes = nblk * (size_t)REC_BLOCK * sizeof(uint32_t);
  if (w.hdr.ensure(hdr_bytes) != hipSuccess || w.rec.ensure(rec_bytes) != hipSuccess) {
    (void)hipGetLastError();
    w.hdr.release(); w.rec.release();  // (the workspace stays usable: a later mesh asks again)
    return fail(GSDF_ERR_CAPACITY, "no device memory for the cut-leaf record arena (" + std::to_string(nblk) + " blocks: " + std::to_string(hdr_bytes) + " + " +
                                       std::to_string(rec_bytes) + " bytes)");
  }
  if (want_recs && w.grp.ensure(ngrp * sizeof(unsigned long long)) != hipSuccess) {
    (void)hipGetLastError();
    return (fail(GSDF_ERR_CAPACITY, "no device memory for the cut-leaf record arena (payload = records needs it)"));
  }
  clear_bytes = kCtrBytes + ngrp * sizeof(unsigned long long);
  HIP_TRY(w.ctr.ensure(clear_bytes));
  d_ctr = (MeshCounters*)w.ctr.p;
  // Brick masks (dev_ops.h: D_SKIP): valid when the last level of cubes, which the leaf kernels continue from, is a level-3 brick
  // that was centre-tested by interval evaluation -- that test leaves, in every surviving cube's w field, which operand
  // subtrees of the program cannot matter anywhere in the cube. GSDF_HIP_NO_BRICK_MASKS=1: no numbers in the program at all.
  masks_valid = lq == 3 && ptest == 1 && p->prog.n_skip_ids > 0 && (pmask == 1 || (pmask > 1 && ((pmask >> lq) & 1)));
  return GSDF_OK;
}

int gsdf_mesh_job::enqueue_descent() {
  // the counters and the group sums are cleared by the chain's first kernel (prune_spec_kernel); one launch per level: a memset
  static const bool use_spec = env_flag_on("GSDF_HIP_PRUNE_SPEC");
  if (!use_spec) HIP_TRY(hipMemsetAsync(d_ctr, 0, clear_bytes, s));
  HIP_TRY(hipEventRecord(w.ev[0], s));
  static const int prune_bpc = env_int("GSDF_HIP_PRUNE_BPC", 2);  // tuning knob: 2 workgroups per CU (round 4: 4 -> 2 is -3 us on a blocking mesh and leaves the CUs to the other mesh in flight: 0.503 -> 0.486 ms per mesh, two in flight)
  // The first S levels (at most 7: 299,593 cubes) are centre-tested speculatively, every cube of the complete octree at once,
  // and resolved by a second launch (kernels.h: prune_spec_kernel / prune_resolve_kernel): two launches instead of a chain of
  // S dependent ones. GSDF_HIP_PRUNE_SPEC=0 keeps one launch per level (cross-check in the tests).
  int first_level = levels;  // first level of the per-level chain
  chain_first = levels;
  unsigned* spec_part = nullptr;  // statistics rows of the speculative top, for the first per-level launch to add up
  unsigned spec_rows = 0, spec_mask = 0;
  int spec_top_S = 0;
  const unsigned test_mask = pmask == 1 ? 0xffffffffu : (unsigned)pmask;
  if (use_spec) {
    const int S = levels - lq + 1 < 7 ? levels - lq + 1 : 7;
    const int last_spec = levels - (S - 1);
    unsigned n_spec = 0;
    for (int j = 0; j < S; j++) n_spec += 1u << (3 * j);
    // the resolve stage's statistics: a row of 16 counts per workgroup behind the pass bytes, added up by the first per-level
    // launch -- if there is one (else the resolve stage issues its atomics itself)
    const unsigned rrows = (n_spec + SPEC_STAGE - 1) / SPEC_STAGE;
    const size_t part_off = ((size_t)n_spec + 63) & ~(size_t)63;
    // brick masks of the block's last level, when that is the level the leaf kernels continue from (meshes of up to nine levels):
    // two bytes per cube of that level, behind the statistics rows
    const unsigned n_last = 1u << (3 * (S - 1));
    const size_t mask_off_b = (part_off + (size_t)rrows * 16 * sizeof(unsigned) + 63) & ~(size_t)63;
    const bool spec_masks = masks_valid && last_spec == lq;
    HIP_TRY(w.spec_pass.ensure(mask_off_b + (spec_masks ? (size_t)n_last * sizeof(uint16_t) : 0)));
    uint16_t* d_mask16 = spec_masks ? (uint16_t*)((char*)w.spec_pass.p + mask_off_b) : nullptr;
    const bool chain_follows = last_spec - 1 >= lq;
    spec_part = chain_follows ? (unsigned*)((char*)w.spec_pass.p + part_off) : nullptr;
    spec_rows = rrows;
    spec_top_S = levels | (S << 8);
    spec_mask = test_mask;
    const int shard_level = opts.shard_count > 1 ? ls : -1;
    HIP_TRY(launch_kernel(prune_spec_kernel, p->spec.f_prune_spec, grid_for(n_spec, p->num_cu, 8), BLOCK, lds_prune, s, p->d_code.p, levels, n_spec, prune_cols, p->prog.nslots, ox, oy,
                          oz, res, test_mask, ptest, shard_level, opts.shard_rank, opts.shard_count, w.spec_pass.p, (unsigned*)d_ctr, clear_bytes / 4, d_mask16, n_spec - n_last));
    hipLaunchKernelGGL(prune_resolve_kernel, dim3((n_spec + SPEC_STAGE - 1) / SPEC_STAGE), dim3(BLOCK), 0, s, (const uint8_t*)w.spec_pass.p, levels, S,
                       n_spec, test_mask, q[last_spec & 1], (unsigned long long)capq[last_spec & 1], d_ctr, spec_part,
                       (const uint16_t*)d_mask16);
    HIP_TRY(hipGetLastError());
    first_level = last_spec - 1;
    chain_first = first_level;
  }
  for (int level = first_level; level >= lq; level--) {
    const int expand = level != levels;
    const int do_test = (level >= 3 && (pmask == 1 || (pmask > 1 && ((pmask >> level) & 1)))) ? ptest : 0;
    // upper bound of candidates at this level (for the grid only): 8^(levels-level), capped by the queue
    uint64_t bound = (levels - level) * 3 >= 40 ? UINT64_MAX : ((uint64_t)1 << (3 * (levels - level)));
    if (bound > capq[(level + 1) & 1] * 8) bound = capq[(level + 1) & 1] * 8;
    HIP_TRY(launch_kernel(prune_kernel, p->spec.f_prune, grid_for(bound, p->num_cu, prune_bpc), BLOCK, lds_prune, s, p->d_code.p, q[(level + 1) & 1], capq[(level + 1) & 1], expand, level,
                          prune_cols, p->prog.nslots, ox, oy, oz, res, do_test, q[level & 1], capq[level & 1], (opts.shard_count > 1 && level == ls) ? 1 : 0, opts.shard_rank,
                          opts.shard_count, d_ctr, level == first_level ? spec_part : nullptr, spec_rows, spec_top_S, spec_mask));
  }
  HIP_TRY(hipEventRecord(w.ev[1], s));
  return GSDF_OK;
}

int gsdf_mesh_job::enqueue_leaf() {
  const uint64_t bound = lbound;
  const unsigned long long tcap = opts.max_tris ? opts.max_tris : m->cap;
  static const int leaf_bpc = env_int("GSDF_HIP_LEAF_BPC", 32);  // (round 4: 32 -- the same for one mesh at a time, 0.503 -> 0.475 ms per mesh with two in flight: the other chain's small kernels are dispatched sooner behind a shorter queue of workgroups; the sentence that follows describes the round-3 sweep)  // grid = up to 64 workgroups per CU (4 resident): a few grid-stride iterations each, so the CUs drain evenly at the end (8 per CU: +8 % kernel time; one iteration per workgroup: +10 %)
  const unsigned grid = grid_for(bound, p->num_cu, leaf_bpc);
  const Cube* cubes = q[lq & 1];
  const uint64_t ncubes = capq[lq & 1];
  // evaluation + cut-leaf records, then marching cubes over the records
  uint32_t* d_hdr = (uint32_t*)w.hdr.p;
  uint32_t* d_rec = (uint32_t*)w.rec.p;
  unsigned long long* d_psum = (unsigned long long*)((char*)w.ctr.p + kCtrBytes);  // cleared with the counters
  const unsigned use_masks = masks_valid ? 1u : 0u;
  // share_corners = 1: every bitwise-distinct lattice point of a brick once (kernels_octree.h: leaf_dense_kernel)
  used_dense = opts.share_corners == 1 && lq == 3 && lk == 4;
  // share_corners = 2: the distinct z rows of a brick once each (kernels_octree.h: DZ) -- column bricks at four points per lane
  const bool want_dz = opts.share_corners == 2 && lq == 3 && lk == 4;
  if (used_dense) {
    spec_ensure(p, SPEC_DENSE);
    const size_t lds_d = p->lds_dense();
    HIP_TRY(launch_kernel(leaf_dense_aot(3 * lds_d <= gsdf_program::kLdsPerCu ? 3 : 2), p->spec.f_leaf_dense, grid, BLOCK, lds_d, s, p->d_code.p, cubes, ncubes, p->prog.nslots, ox, oy, oz, res,
                          d_hdr, d_rec, d_psum, nblk, d_ctr, use_masks));
  } else {
    if (want_dz) spec_ensure(p, SPEC_ROWS);
    const LeafPick pick = p->leaf_pick(lq, want_dz);
    used_dz = pick.v.dz;
    // (fewer than three levels: a few leaves per pass, and room for the case table whether lds_m counts it or not)
    HIP_TRY(launch_kernel(leaf_eval_aot(pick.v), pick.f, grid, BLOCK, lq != 3 ? lds_m + 256 : lds_m, s, p->d_code.p, cubes, ncubes, lq, p->prog.nslots, ox, oy, oz, res, d_hdr, d_rec,
                          d_psum, nblk, d_ctr, use_masks));
  }
  HIP_TRY(hipEventRecord(w.ev[3], s));
  if (want_recs) {
    // no marching here: the records are packed for the gather (scan_groups_kernel + pack_records_kernel), marching cubes
    // runs where they arrive (march_dense_kernel)
    uint64_t rec_cap = m->recs_cap36 * 36 / 41;  // 40 B per record + 4 B per 256 of them, rounded: stays inside the buffer
    if (rec_cap > 2) rec_cap -= 2;
    hipLaunchKernelGGL(scan_groups_kernel, dim3(1), dim3(1024), 0, s, (const unsigned long long*)d_psum, (unsigned long long)nblk, lq, d_ctr,
                       (unsigned long long*)w.grp.p, m->d_recs, (unsigned long long)rec_cap,
                       ctr_from_kernel ? hcp : (MeshCounters*)nullptr);
    HIP_TRY(hipGetLastError());
    const uint64_t ngrp_q = (nblk_q + MARCH_GROUP - 1) / MARCH_GROUP;
    const uint64_t gmax = (uint64_t)p->num_cu * 8;
    hipLaunchKernelGGL(pack_records_kernel, dim3((unsigned)(ngrp_q < gmax ? (ngrp_q ? ngrp_q : 1) : gmax)), dim3(BLOCK), 0, s, (const uint32_t*)d_hdr,
                       (const uint32_t*)d_rec, (const unsigned long long*)w.grp.p, (unsigned long long)nblk, lq, (const MeshCounters*)d_ctr,
                       m->d_recs, (unsigned long long)rec_cap);
  } else {
    // one wave of workgroups: each takes an equal share of the records (computed on device from the group sums)
    static const int march_bpc = env_int("GSDF_HIP_MARCH_BPC", 4);  // tuning knob (7 fit a CU; 4 leave LDS and wave slots to the other mesh in flight: 0.503 -> 0.495 ms per mesh, and a blocking mesh loses nothing)
    const size_t lds_march = MARCH_LDS_BYTES;
    hipLaunchKernelGGL(march_records_kernel, dim3(grid_for(nblk_q, p->num_cu, march_bpc)), dim3(BLOCK), lds_march, s, d_hdr, d_rec,
                       d_psum, (unsigned long long)nblk, lq, ox, oy, oz, res, m->d_tris, (uint64_t)tcap, d_ctr,
                       ctr_from_kernel ? hcp : (MeshCounters*)nullptr);
  }
  ctr_on_host = ctr_from_kernel;
  HIP_TRY(hipGetLastError());
  return GSDF_OK;
}

int gsdf_mesh_job::enqueue_handover() {
  // the completion event: the leaf phase's own when the last kernel has handed the counters to the host (nothing sits between them)
  if (!ctr_on_host) {
    HIP_TRY(hipMemcpyAsync(hcp, d_ctr, sizeof(MeshCounters), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipEventRecord(w.ev[4], s));
  }
  ev_done = ctr_on_host ? w.ev[2] : w.ev[4];
  return GSDF_OK;
}

int gsdf_mesh_job::finish(bool* again) {
    MeshCounters& hc = *hcp;
    HIP_TRY(hipEventSynchronize(ev_done));
    if (hc.q_overflow) {  // a cube queue was too small: double and redo (exact: nothing was dropped silently)
      if (attempt >= 8) return (fail(GSDF_ERR_CAPACITY, "octree queue capacity exceeded"));
      qcap *= 4;
      *again = true;
      return GSDF_OK;
    }
    // more blocks than the record arena holds: the blocks beyond it were skipped -- repeat with room for all
    const uint64_t need = ((hc.n_level[lq] << (3 * (lq - 1))) + 63) / 64;
    if (need > nblk) {
      if (attempt >= 8) return (fail(GSDF_ERR_CAPACITY, "cut-leaf record arena capacity exceeded"));
      p->rec_blocks = need + need / 8 + 1024;
      *again = true;
      return GSDF_OK;
    }
    if (hc.overflow && want_recs) {  // record payload too small: the scan knows the exact count
      if (attempt >= 8) return (fail(GSDF_ERR_CAPACITY, "device record buffer capacity exceeded"));
      pool_give(p->device, (float*)m->d_recs, m->recs_cap36);
      m->d_recs = nullptr; m->recs_cap36 = 0;
      want_rec_n = hc.n_cut + hc.n_cut / 16 + 1024;
      *again = true;
      return GSDF_OK;
    }
    if (hc.overflow) {  // triangle buffer too small: the kernel kept counting, so the exact size is known
      if (opts.max_tris) return (fail(GSDF_ERR_CAPACITY, "device triangle buffer capacity exceeded"));
      if (attempt >= 8) return (fail(GSDF_ERR_CAPACITY, "device triangle buffer capacity exceeded"));
      release_tris(m);
      want = hc.n_tris + hc.n_tris / 16 + 1024;
      *again = true;
      return GSDF_OK;
    }
    *again = false;
    return GSDF_OK;
}

int gsdf_mesh_job::stats() {
  MeshCounters& hc = *hcp;
  float ms01 = 0, ms12 = 0, ms13 = 0;
  HIP_TRY(hipEventElapsedTime(&ms01, w.ev[0], w.ev[1]));
  HIP_TRY(hipEventElapsedTime(&ms12, w.ev[1], w.ev[2]));
  HIP_TRY(hipEventElapsedTime(&ms13, w.ev[1], w.ev[3]));  // the evaluating kernel alone
  uint64_t evals_prune = 0, pruned = 0;
  for (int level = levels; level >= lq; level--) {
    evals_prune += hc.n_items[level];
    // cubes that passed their test: counted apart only where "passed" and "kept by this rank" differ (prune_kernel)
    const bool dealt_here = opts.shard_count > 1 && level == ls;
    const uint64_t passed = (level <= chain_first && !dealt_here) ? hc.n_level[level] : hc.n_pass[level];
    if (hc.n_items[level]) pruned += (hc.n_items[level] - passed) << (3 * (level - 1));  // DecomposesTo(1) = 8^(level-1)
  }
  const uint64_t n_leaves = hc.n_level[lq] << (3 * (lq - 1));
  const uint64_t evals_leaf = used_dz || used_dense ? hc.n_points  // distinct lattice points (share_corners = 1) / distinct z rows of the bricks (= 2) evaluated once each
                                                    : n_leaves * (uint64_t)lk + (uint64_t)(8 - lk) * (lq == 3 ? n_leaves : hc.n_cont);  // evaluations actually executed (a column brick always evaluates all eight rows: leaf_eval_kernel counts nothing)
  m->st.n_tris = hc.n_tris;
  m->st.evals = evals_prune + evals_leaf;
  m->st.evals_prune = evals_prune;
  m->st.evals_leaf = evals_leaf;
  m->st.pruned_leaves = pruned;
  m->st.leaf_cubes = n_leaves;
  m->st.active_leaves = hc.n_active;
  m->st.ms_prune = ms01;
  m->st.ms_leaf = ms12;
  m->st.ms_march = ms13;
  m->st.ms_emit = ms12 - ms13;
  m->st.cut_leaves = hc.n_cut;
  m->st.ms_total = (double)ms01 + (double)ms12;
  p->evals += m->st.evals;
  p->last_tris = hc.n_tris;
  if (want_recs) { m->payload = GSDF_PAYLOAD_RECORDS; m->n_recs = hc.n_cut; p->last_recs = hc.n_cut; m->weldable = opts.shard_count == 1; }
  return GSDF_OK;
}

static void job_release(gsdf_mesh_job* j, bool failed = true) {
  if (!j) return;
  // the way out of a failed start / wait: a partly enqueued chain may still be running -- nothing goes back to the pool, and the
  // workspace is not handed to the next job, under it
  if (failed && j->s) { (void)hipStreamSynchronize(j->s); (void)hipGetLastError(); }
  if (j->p) j->w.job_busy = false;
  if (j->m) gsdf_hip_mesh_destroy(j->m);
  delete j;
}

// LDS of the centre tests (kernels_octree.h: prune_kernel): two points per lane over the program's slots and its interval stack, the
// stage of PRUNE_STAGE cubes, the wave totals. prune_spec_kernel declares a stage of SPEC_STAGE cubes and a few words statically.
static constexpr size_t lds_prune_of(int cols) { return (size_t)(cols > 0 ? cols : 1) * 2 * BLOCK * sizeof(float) + PRUNE_STAGE * sizeof(Cube) + 64; }
static constexpr size_t kPruneSpecStatic = SPEC_STAGE * sizeof(Cube) + 256;
static_assert(lds_prune_of(GSDF_HIP_MAX_COLS_OCTREE) + kPruneSpecStatic <= gsdf_program::kLdsPerCu && lds_prune_of(GSDF_HIP_MAX_COLS_OCTREE + 1) + kPruneSpecStatic > gsdf_program::kLdsPerCu,
              "gsdf_hip.h: GSDF_HIP_MAX_COLS_OCTREE is the largest slots + interval stack the centre tests fit into a CU's LDS");
// dual contouring's edge pass: three points per lane and what dc_edges_kernel declares statically (s_pend .. s_word)
static constexpr size_t lds_dc_edges_of(int slots) { return (size_t)(slots > 0 ? slots : 1) * 3 * BLOCK * sizeof(float) + DC_EDGE_PASSES * BLOCK * sizeof(uint16_t) + 64; }
static_assert(lds_dc_edges_of(GSDF_HIP_MAX_SLOTS_DC) <= gsdf_program::kLdsPerCu && lds_dc_edges_of(GSDF_HIP_MAX_SLOTS_DC + 1) > gsdf_program::kLdsPerCu,
              "gsdf_hip.h: GSDF_HIP_MAX_SLOTS_DC is the largest slot count the edge pass fits into a CU's LDS");
static_assert(GSDF_HIP_MAX_SLOTS_ALL + 16 == GSDF_HIP_MAX_COLS_OCTREE && GSDF_HIP_MAX_SLOTS_ALL <= GSDF_HIP_MAX_SLOTS_DC, "gsdf_hip.h: GSDF_HIP_MAX_SLOTS_ALL");

extern "C" int gsdf_hip_mesh_octree_start(gsdf_program* p, float res, const gsdf_mesh_opts* opts_in, gsdf_mesh_job** out) {
  if (!p || !out) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *out = nullptr;
  spec_adopt(p);  // (a background build that has finished: its kernels from here on)
  if (p->prog.is2d) return fail(GSDF_ERR_DIMENSION, "program is 2D");
  if (!(res > 0) || std::isnan(res) || std::isinf(res)) return fail(GSDF_ERR_RESOLUTION, "invalid renderer cube resolution");
  gsdf_mesh_opts opts{};
  opts.prune = 1; opts.shard_rank = 0; opts.shard_count = 1; opts.share_corners = 0;
  if (opts_in) opts = *opts_in;
  if (opts.shard_count < 1 || opts.shard_rank < 0 || opts.shard_rank >= opts.shard_count) return fail(GSDF_ERR_BAD_ARGUMENT, "bad shard rank/count");
  if (opts.payload != GSDF_PAYLOAD_TRIANGLES && opts.payload != GSDF_PAYLOAD_RECORDS) return fail(GSDF_ERR_BAD_ARGUMENT, "bad payload kind");
  const bool want_recs = opts.payload == GSDF_PAYLOAD_RECORDS;
  if (opts.share_corners < 0 || opts.share_corners > 3) return fail(GSDF_ERR_BAD_ARGUMENT, "share_corners is 0 (every corner of every leaf, as the reference), 1 (distinct lattice points of a brick), 2 (distinct z rows of a brick) or 3 (1 or 2, whichever suits the tree)");
  // 3: by the program's share of work that depends on x and y alone (the column bricks of 0 and 2 compute it once per lane for all z
  // rows, the packed points of 1 give that up): hypot / atan2 sharing instructions weighted as for the one-body leaf kernel. bolt (0)
  // and knurled-cylinder (2) gain 9 % / 17 % from 1, npt-flange (7) loses 40 % with it and breaks even with 2.
  if (opts.share_corners == 3) opts.share_corners = gsdf_dev::spec_xy_shared_weight(p->prog) < 3 ? 1 : 2;
  if (want_recs && (opts.host_output || opts.max_tris))
    return fail(GSDF_ERR_BAD_ARGUMENT, "payload = records goes with the two-kernel leaf phase only (no host_output, max_tris)");
  {
    // the largest launch of the descent: prune_spec_kernel (lds_prune_of and its static stage of SPEC_STAGE cubes); of the leaf phase:
    // the evaluating kernel with its case table (and what its marching half declares statically)
    const size_t need_prune = lds_prune_of(p->prog.nslots + p->prog.lip_depth) + kPruneSpecStatic, need_leaf = p->leaf_config().lds + 256 + 1024;
    if (int rc = p->lds_refused("gsdf_hip_mesh_octree", need_prune > need_leaf ? need_prune : need_leaf, "slots + interval stack <= " + std::to_string(GSDF_HIP_MAX_COLS_OCTREE))) return rc;
  }
  HIP_TRY(hipSetDevice(p->device));

  // Octree.Reset (octreerenderer.go:71-128) + makeICube (:222-235)
  float mn[3], mx[3];
  scale_centered(p->prog.bb, 1.01f, mn, mx);
  const float longAxis = fmaxf(mx[0] - mn[0], fmaxf(mx[1] - mn[1], mx[2] - mn[2]));
  const float l2 = gsdf::log2f32(longAxis / res);
  const int levels = (int)std::ceil(l2) + 1;
  if (levels <= 1) return fail(GSDF_ERR_RESOLUTION, "resolution not fine enough for marching cubes");
  if (levels > 17) return fail(GSDF_ERR_RESOLUTION, "resolution too fine: more than 17 octree levels");

  int slot = -1;
  for (int k = 0; k < gsdf_program::kJobs; k++) if (!p->ws[k].job_busy) { slot = k; break; }
  if (slot < 0) return fail(GSDF_ERR_BAD_ARGUMENT, "three meshes of this program are in flight already: wait for one (gsdf_hip_mesh_octree_wait)");
  // Each slot has a workspace and a stream of its own: two chains in flight run beside each other (a caller's stream takes both).
  // Measured at npt-flange resdiv 1600, per mesh: one blocking call at a time 0.59 ms; two chains back to back on ONE stream 0.58;
  // on TWO streams 0.50 -- the centre tests and the marching kernel of one mesh (latency- and HBM-bound) run under the evaluating
  // kernel of the other. Tried and dropped: one stream for the evaluating kernels of all meshes and side streams for the stages
  // around them, ordered by events (a three-stage pipeline): 0.54, and a blocking call 0.61 -- every cross-stream event wait is
  // ~10 us on this runtime.
  gsdf_program::OctreeWs& w = p->ws[slot];
  if (slot > 0 && !opts.stream && w.own.ensure() != hipSuccess) {  // (slot 0 runs on the handle's stream)
    (void)hipGetLastError();
    return fail(GSDF_ERR_HIP, "hipStreamCreate failed");
  }
  hipStream_t s = opts.stream ? (hipStream_t)opts.stream : (slot > 0 ? w.own.s : p->stream.s);
  gsdf_mesh_job* j = new (std::nothrow) gsdf_mesh_job(p, slot);
  gsdf_mesh* m = new (std::nothrow) gsdf_mesh();
  if (!j || !m) { delete j; delete m; return fail(GSDF_ERR_BAD_ARGUMENT, "out of memory"); }
  j->m = m; j->opts = opts; j->res = res; j->s = s; j->levels = levels; j->want_recs = want_recs;
  j->ox = mn[0]; j->oy = mn[1]; j->oz = mn[2];
  w.job_busy = true;
  w.job_stream = s;
  m->device = p->device;
  m->stream = s;
  m->num_cu = p->num_cu;
  m->st.levels = levels;
  m->st.res = res;
  m->st.origin[0] = j->ox; m->st.origin[1] = j->oy; m->st.origin[2] = j->oz;
  auto bail = [&](int code) { job_release(j); return code; };
  static_assert(sizeof(MeshCounters) <= 2048, "counters: a 2 KB slot of the pinned block each (slot 1: DCCounters of dual contouring)");
  if (!p->h_ctr.p && hipHostMalloc(&p->h_ctr.p, 16384, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return bail(fail(GSDF_ERR_HIP, "hipHostMalloc of the counter block failed")); }
  j->hcp = (MeshCounters*)((char*)p->h_ctr.p + (size_t)slot * 4096);
  if (w.ev.ensure() != hipSuccess) return bail(fail(GSDF_ERR_HIP, "hipEventCreate failed"));

  // ---- level-synchronous descent from the top cube to level lq = min(levels, 3). The whole chain
  // (memset, one prune launch per level, the leaf kernel) is enqueued without a host round trip: each
  // kernel reads its input count from the previous level's counter in device memory.
  j->lq = levels < 3 ? levels : 3;
  // multi-GPU: bricks of level ls are dealt to ranks by a hash of their coordinates (brick_owner).
  j->ls = levels < j->lq + 2 ? levels : j->lq + 2;
  j->prune_cols = p->prog.nslots + p->prog.lip_depth;  // interval mode: two points per lane + the interval stack
  j->lds_prune = lds_prune_of(j->prune_cols);
  j->pmask = opts.prune & ~GSDF_PRUNE_ASSUME_SDF;  // levels to test: 0 none, 1 all, else bit L = Level L
  if ((opts.prune & GSDF_PRUNE_ASSUME_SDF) && j->pmask == 0) j->pmask = 1;
  j->ptest = (opts.prune & GSDF_PRUNE_ASSUME_SDF) ? 2 : 1;
  static const size_t lds_pad = (size_t)env_int("GSDF_HIP_LEAF_LDS_PAD", 0);  // developer knob: LDS a leaf workgroup asks for beyond its need (occupancy experiments)
  j->lk = p->leaf_config().k;
  j->lds_m = p->leaf_config().lds + lds_pad;
  j->qcap = j->w.q0.cap / sizeof(Cube);
  {
    // 1 M cubes (8 MB) per queue to start with; GSDF_HIP_QCAP_MIN lowers it so that tests can drive the
    // overflow -> grow -> rerun path (the arenas only ever grow, so a handle that already meshed keeps its size)
    const uint64_t qmin = env_u64("GSDF_HIP_QCAP_MIN", (uint64_t)1 << 20);  // (read at every mesh)
    if (j->qcap < qmin) j->qcap = qmin;
    if (j->qcap < 64) j->qcap = 64;
  }
  j->want = opts.max_tris;
  *j->hcp = MeshCounters{};
  j->chain_first = levels;
  if (int rc = j->enqueue()) return bail(rc);
  *out = j;
  return GSDF_OK;
}

extern "C" int gsdf_hip_mesh_octree_wait(gsdf_mesh_job* j, gsdf_mesh** out) {
  if (!j || !out) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *out = nullptr;
  (void)hipSetDevice(j->p->device);
  for (;;) {
    bool again = false;
    if (int rc = j->finish(&again)) { job_release(j); return rc; }
    if (!again) break;
    j->attempt++;
    if (int rc = j->enqueue()) { job_release(j); return rc; }
  }
  if (int rc = j->stats()) { job_release(j); return rc; }
  *out = j->m;
  j->m = nullptr;
  job_release(j, /*failed=*/false);
  return GSDF_OK;
}

extern "C" int gsdf_hip_mesh_octree(gsdf_program* p, float res, const gsdf_mesh_opts* opts_in, gsdf_mesh** out) {
  if (!out) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *out = nullptr;
  gsdf_mesh_job* j = nullptr;
  if (int rc = gsdf_hip_mesh_octree_start(p, res, opts_in, &j)) return rc;
  return gsdf_hip_mesh_octree_wait(j, out);
}

// ---- packed cut-leaf records -> triangles (kernels_octree.h: march_dense_kernel) ------------------------------------------
static_assert(sizeof(gsdf_dense_part) == sizeof(DensePart) && kDenseMaxParts == DENSE_MAX_PARTS, "abi_host.h mirrors kernels_octree.h");
size_t dense_parts_bytes() { return sizeof(DenseParts) + 8; }  // (+ 8: the table starts at the next 8-byte boundary behind the triangles)
void* dense_parts_at(float* d_tris, uint64_t n_tris) {  // n_tris * 36 bytes is a multiple of 4 only: the table holds 64-bit fields
  return (void*)(((uintptr_t)(d_tris + n_tris * 9) + 7) & ~(uintptr_t)7);
}
int mesh_march_dense(const uint8_t* d_buf, const gsdf_dense_part* parts, int nparts, void* d_parts, float ox, float oy, float oz, float res,
                     float* d_tris, int num_cu, hipStream_t s) {
  if (nparts < 1 || nparts > DENSE_MAX_PARTS) return fail(GSDF_ERR_BAD_ARGUMENT, "march over packed records: 1 to 64 parts");
  DenseParts h{};
  h.n = nparts;
  uint64_t chunks = 0;
  for (int i = 0; i < nparts; i++) {
    h.p[i].off = parts[i].off; h.p[i].n_recs = parts[i].n_recs; h.p[i].tri0 = parts[i].tri0;
    chunks += (parts[i].n_recs + DENSE_CHUNK - 1) / DENSE_CHUNK;
    if (dense_bytes(parts[i].n_recs) != dense_payload_bytes(parts[i].n_recs)) return fail(GSDF_ERR_BAD_ARGUMENT, "internal: payload layouts differ");
  }
  if (chunks == 0) return GSDF_OK;
  // the table is small and the copy's source is this stack frame: hipMemcpyAsync from pageable memory stages it before returning
  HIP_TRY(hipMemcpyAsync(d_parts, &h, sizeof h, hipMemcpyHostToDevice, s));
  static const int march_bpc = env_int("GSDF_HIP_MARCH_BPC", 4);  // tuning knob (see enqueue_leaf)
  const uint64_t gmax = (uint64_t)num_cu * (uint64_t)(march_bpc > 0 ? march_bpc : 4);
  const size_t lds = MARCH_DENSE_LDS_BYTES;
  hipLaunchKernelGGL(march_dense_kernel, dim3((unsigned)(chunks < gmax ? chunks : gmax)), dim3(BLOCK), lds, s, d_buf, (const DenseParts*)d_parts, ox, oy, oz, res, d_tris);
  HIP_TRY(hipGetLastError());
  return GSDF_OK;
}

extern "C" int gsdf_hip_mesh_stage_ms(const gsdf_mesh* m, double* ms, const char** names, int cap, int* n) {
  if (!m || !n) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *n = m->n_stages;
  for (int k = 0; k < m->n_stages && k < cap; k++) {
    if (ms) ms[k] = m->stage_ms[k];
    if (names) names[k] = m->stage_name[k];
  }
  return GSDF_OK;
}

extern "C" int gsdf_hip_mesh_payload(const gsdf_mesh* m, uint64_t* n_records, uint64_t* payload_bytes) {
  if (!m) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  const bool r = m->payload == GSDF_PAYLOAD_RECORDS;
  if (n_records) *n_records = r ? m->n_recs : 0;
  if (payload_bytes) *payload_bytes = r ? dense_bytes(m->n_recs) : 0;
  return m->payload;
}

extern "C" int gsdf_hip_mesh_read_records(const gsdf_mesh* m, uint32_t* dst, uint64_t dst_records, uint64_t* n_records) {
  if (!m) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  const bool r = m->payload == GSDF_PAYLOAD_RECORDS;
  const uint8_t* d = r ? m->d_recs : m->d_wrecs;
  const uint64_t n = r ? m->n_recs : m->n_wrecs;
  if (!r && !m->weldable) return fail(GSDF_ERR_BAD_ARGUMENT, "the mesh holds no cut-leaf records (payload = GSDF_PAYLOAD_RECORDS keeps them)");
  if (n_records) *n_records = n;
  if (!dst) return GSDF_OK;
  if (dst_records < n) return fail(GSDF_ERR_SHORT_BUFFER, "short buffer");
  if (n == 0) return GSDF_OK;
  HIP_TRY(hipSetDevice(m->device));
  HIP_TRY(hipMemcpy(dst, d, n * 40ull, hipMemcpyDeviceToHost));
  return GSDF_OK;
}

extern "C" int gsdf_hip_mesh_march(gsdf_mesh* m) {
  if (!m) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (m->payload != GSDF_PAYLOAD_RECORDS) return GSDF_OK;
  if (m->inflight.load() > 0) return fail(GSDF_ERR_BAD_ARGUMENT, "the mesh is being gathered: wait for the gather first");
  HIP_TRY(hipSetDevice(m->device));
  const uint64_t n = m->st.n_tris;
  if (n) {
    const uint64_t units = n + (dense_parts_bytes() + 35) / 36;  // the parts table rides behind the triangles
    m->d_tris = pool_take(m->device, units, &m->cap);
    if (!m->d_tris) {
      if (hipMalloc((void**)&m->d_tris, units * 36) != hipSuccess) { (void)hipGetLastError(); return fail(GSDF_ERR_HIP, "hipMalloc of the triangle buffer failed"); }
      m->cap = units;
    }
    const gsdf_dense_part part{0, m->n_recs, 0};
    hipStream_t rs = mesh_stream(m);
    const int rc = mesh_march_dense(m->d_recs, &part, 1, dense_parts_at(m->d_tris, n), m->st.origin[0], m->st.origin[1], m->st.origin[2], m->st.res, m->d_tris,
                                    m->num_cu, rs);
    if (rc) { release_tris(m); return rc; }
    hipError_t e = hipStreamSynchronize(rs);
    if (e != hipSuccess) { release_tris(m); return fail(GSDF_ERR_HIP, std::string("march over the records: ") + hipGetErrorString(e)); }
  }
  if (m->weldable) { m->d_wrecs = m->d_recs; m->wrecs_cap36 = m->recs_cap36; m->n_wrecs = m->n_recs; }  // kept for gsdf_hip_mesh_weld
  else pool_give(m->device, (float*)m->d_recs, m->recs_cap36);
  m->d_recs = nullptr; m->recs_cap36 = 0; m->n_recs = 0;
  m->payload = GSDF_PAYLOAD_TRIANGLES;
  return GSDF_OK;
}

// Workspace of dual contouring's indexed quad stage (kernels_dc_indexed.h) in one arena: byte offsets.
namespace {
struct DcIndexedWs {
  uint64_t n_rows = 0;  // lattice rows (z, y): n^2
  unsigned n_row_blocks = 0;
  size_t quad = 0, place = 0, row_cnt = 0, row_base = 0, blk_cnt = 0, blk_base = 0, total = 0, bad = 0, bytes = 0;
  static DcIndexedWs of(uint64_t ecap, int nshift) {
    DcIndexedWs w;
    w.n_rows = (uint64_t)1 << (2 * nshift);
    w.n_row_blocks = (unsigned)((w.n_rows + BLOCK - 1) / BLOCK);
    w.quad = 0;                                    // uint4 per edge: first, 16-byte aligned
    w.place = w.quad + (size_t)ecap * 16;
    w.row_cnt = w.place + (size_t)ecap * 4;
    w.row_base = w.row_cnt + (size_t)w.n_rows * 4;
    w.blk_cnt = w.row_base + (size_t)w.n_rows * 4;
    w.blk_base = w.blk_cnt + (size_t)w.n_row_blocks * 4;
    w.total = (w.blk_base + (size_t)w.n_row_blocks * 4 + 7) & ~(size_t)7;
    w.bad = w.total + 8;  // violations counted by passes C and D (none, by construction)
    w.bytes = w.bad + 8;
    return w;
  }
};
}  // namespace

// glrender.DualContourRenderer.Reset + RenderAll with DualContourLeastSquares on device.
// out_ix == nullptr: the triangle soup (dc_quads_kernel). Else the quads in lattice order as an indexed mesh (kernels_dc_indexed.h
// in the place of dc_quads_kernel; *out then carries the statistics alone).
static int dc_mesh(gsdf_program* p, float res, int chiseled, int shard_rank, int shard_count, void* stream, gsdf_mesh** out, gsdf_indexed** out_ix) {
  if (!p || !out) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *out = nullptr;
  spec_adopt(p);  // (a background build that has finished: its kernels from here on)
  if (p->prog.is2d) return fail(GSDF_ERR_DIMENSION, "program is 2D");
  if (!(res > 0) || std::isnan(res) || std::isinf(res)) return fail(GSDF_ERR_RESOLUTION, "invalid renderer cube resolution");
  if (shard_count < 1 || shard_rank < 0 || shard_rank >= shard_count) return fail(GSDF_ERR_BAD_ARGUMENT, "bad shard rank/count");
  if (p->mesh_in_flight()) return fail(GSDF_ERR_BAD_ARGUMENT, "an octree mesh of this program is in flight: wait for it first (shared workspace)");
  {
    // the largest launch: dc_edges_kernel (three points per lane + 2104 bytes declared statically: s_pend .. s_word), unless a forced
    // batch size makes it the origin sweep (K points per lane + 32 bytes)
    const size_t need_edges = lds_dc_edges_of(p->prog.nslots), need_origin = p->lds_bytes(p->batch_k()) + 32;
    if (int rc = p->lds_refused("dual contouring", need_edges > need_origin ? need_edges : need_origin, std::to_string(GSDF_HIP_MAX_SLOTS_DC) + " slots")) return rc;
  }
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t s = stream ? (hipStream_t)stream : p->stream.s;
  // Reset (dual_contour.go:26-41): bounds shifted by -res/2, makeICube
  const float sub = res / 2;
  float mn[3], mx[3];
  for (int a = 0; a < 3; a++) { mn[a] = p->prog.bb[a] + -sub; mx[a] = p->prog.bb[a + 3] + -sub; }
  const float longAxis = fmaxf(mx[0] - mn[0], fmaxf(mx[1] - mn[1], mx[2] - mn[2]));
  const int levels = (int)std::ceil(gsdf::log2f32(longAxis / res)) + 1;
  if (levels <= 1) return fail(GSDF_ERR_RESOLUTION, "resolution not fine enough for marching cubes");
  // the neighbour lookup is a dense int32 index grid over the 2^(levels-1) cube lattice: 4.3 GB at 11 levels, 34 GB at 12 --
  // what one 288 GB device holds beside the rest of the workspace (13 levels would be 275 GB)
  if (levels > 12) return fail(GSDF_ERR_RESOLUTION, "dual contouring lattice too large: more than 12 octree levels");
  const int nshift = levels - 1;
  const uint64_t ncell = (uint64_t)1 << (3 * nshift);
  const float ox = mn[0], oy = mn[1], oz = mn[2];
  // multi-GPU: z-slabs. A rank owns the quads of cubes with z in [zown_lo, zown_hi); their vertices need the cubes of
  // [zown_lo-1, zown_hi) placed, which in turn need the distances and normals of [zown_lo-1, zown_hi+1). Every stage is
  // a pure function of the lattice cell, so the halo is recomputed instead of exchanged (no data-path collective).
  const unsigned nz = 1u << nshift;
  uint32_t zown_lo = 0, zown_hi = 0;
  gsdf_hip_slab_range(nz, (uint32_t)shard_rank, (uint32_t)shard_count, &zown_lo, &zown_hi);
  const unsigned zlo = zown_lo > 0 ? zown_lo - 1 : 0, zhi = zown_hi < nz ? zown_hi + 1 : nz;
  const uint64_t nslab = (uint64_t)(zhi - zlo) << (2 * nshift);

  gsdf_mesh* m = new (std::nothrow) gsdf_mesh();
  if (!m) return fail(GSDF_ERR_BAD_ARGUMENT, "out of memory");
  m->device = p->device; m->stream = s; m->num_cu = p->num_cu;
  m->st.levels = levels; m->st.res = res;
  m->st.origin[0] = ox; m->st.origin[1] = oy; m->st.origin[2] = oz;
  auto bail = [&](int code) {
    if (out_ix && *out_ix) { gsdf_hip_indexed_destroy(*out_ix); *out_ix = nullptr; }
    gsdf_hip_mesh_destroy(m);
    return code;
  };
  gsdf_program::OctreeWs& w0 = p->ws[0];  // its first queue, its counters and its events serve here too (no octree mesh is in flight)
  const EventSet<5>& ev = w0.ev;
  HIP_TRYM(w0.ev.ensure());
  HIP_TRYM(p->dc_ev.ensure());
  // Workspace lives in the program handle (grow-only): the index grid alone is 4.3 GB at 1024^3 cells, and a
  // hipMalloc/hipFree pair of that size per mesh cost more wall time than the whole device pass.
  Arena &grid = p->dc_grid, &d2 = p->dc_dist, &f2 = p->dc_fv, &n2 = p->dc_nrm, &e2 = p->dc_edge;
  HIP_TRYM(grid.ensure(ncell * sizeof(int)));
  HIP_TRYM(w0.ctr.ensure(sizeof(MeshCounters) > sizeof(DCCounters) ? sizeof(MeshCounters) : sizeof(DCCounters)));
  DCCounters* d_ctr = (DCCounters*)w0.ctr.p;
  const int lk = p->batch_k();
  // Kept cubes hug the surface: ~ c * n^2 of the n^3 lattice. Start from the previous pass on this handle, else from
  // 12 n^2 (an overflow repeats the full-lattice origin pass, so be generous: 84 B per cube).
  uint64_t ccap = p->last_dc_cubes ? p->last_dc_cubes + p->last_dc_cubes / 8 + 4096 : (uint64_t)12 << (2 * nshift);
  if (ccap < (1u << 20)) ccap = 1u << 20;
  DCCounters hc{};
  uint64_t n_cubes = 0, n_edges = 0, n_cube_runs = 0, n_edge_runs = 0, last_cap = 0, final_ccap = 0;
  unsigned long long n_quads = 0;  // (indexed: pass B's total)
  DcIndexedWs ixw{};
  const float h = (chiseled ? (float)1e-4 : (float)2e-8) * 0.5f;  // NormalsCentralDiff: step *= 0.5
  const float sqrtLambda = chiseled ? (float)(std::sqrt(1e-5) * 1e-4) : (float)std::sqrt(1e-5);
  spec_ensure(p, SPEC_AUX);
  const int ub = p->prog.has_exact_bb ? 1 : 0;
  const float* eb = p->prog.exact_bb;
  // tile range of the origin sweep (8 x 8 x 4K cells per tile, z tiles counted from zlo)
  const unsigned ncell1 = 1u << nshift, tzk = 4u * (unsigned)lk;
  unsigned t0[3] = {0, 0, 0}, tn[3] = {(ncell1 + 7u) >> 3, (ncell1 + 7u) >> 3, (zhi - zlo + tzk - 1u) / tzk};
  if (ub) {
    const float org[3] = {ox, oy, oz}, grow = res * 2 * 1.001f + 2 * res;
    const unsigned lo_lim[3] = {0, 0, zlo}, hi_lim[3] = {ncell1, ncell1, zhi}, tsz[3] = {8, 8, tzk};
    for (int a = 0; a < 3; a++) {
      double c0 = std::floor(((double)eb[a] - grow - org[a]) / res) - 1, c1 = std::ceil(((double)eb[a + 3] + grow - org[a]) / res) + 2;
      if (c0 < lo_lim[a]) c0 = lo_lim[a];
      if (c1 > hi_lim[a]) c1 = hi_lim[a];
      if (c1 <= c0) { c0 = lo_lim[a]; c1 = lo_lim[a]; }  // nothing of the box in this slab
      const unsigned first = ((unsigned)c0 - lo_lim[a]) / tsz[a], last = ((unsigned)c1 - lo_lim[a] + tsz[a] - 1) / tsz[a];
      t0[a] = first;
      tn[a] = last > first ? last - first : 0;
    }
  }
  const uint64_t ntiles = (uint64_t)tn[0] * tn[1] * tn[2];  // of the origin sweep
  for (int attempt = 0;; attempt++) {
    // the lists are kept in DC_PARTS parts (kernels_dc.h), an equal share of the arrays each; a part cannot hold more than the cells
    // of the tiles that go to it
    const uint64_t cmax = DC_PARTS * ((ntiles + DC_PARTS - 1) / DC_PARTS) * (uint64_t)(256 * lk);
    if (ccap > cmax) ccap = cmax;
    ccap = (ccap + DC_PARTS - 1) / DC_PARTS * DC_PARTS;
    if (ccap < DC_PARTS) ccap = DC_PARTS;
    const uint64_t ecap = 3 * ccap, tcap = 2 * ecap;
    // run descriptors (kernels_dc.h: DC_DESC): the origin sweep's follow the cubes in q0, the edge stage's have an arena of their own
    const uint64_t crun_cap = DC_PARTS * dc_cube_run_seg(ntiles), erun_cap = DC_PARTS * dc_edge_run_seg(ccap, ntiles);
    HIP_TRYM(w0.q0.ensure((ccap + crun_cap) * sizeof(Cube) + ccap * sizeof(float)));  // (+ the sweep's distance of every kept cube, behind the descriptors)
    HIP_TRYM(p->dc_erun.ensure(erun_cap * sizeof(unsigned long long)));
    HIP_TRYM(p->dc_flag.ensure(ccap));  // "this cube is placed", a byte per cube: set by the edge stage, read by the placement stage
    HIP_TRYM(d2.ensure(ccap * sizeof(float4)));
    HIP_TRYM(f2.ensure(ccap * 12));
    HIP_TRYM(n2.ensure(ccap * 36));
    HIP_TRYM(e2.ensure(ecap * sizeof(unsigned)));
    if (!out_ix && (!m->d_tris || m->cap < tcap)) {
      pool_give(p->device, m->d_tris, m->cap);
      m->d_tris = pool_take(p->device, tcap, &m->cap);
      if (!m->d_tris) { HIP_TRYM(hipMalloc((void**)&m->d_tris, tcap * 36)); m->cap = tcap; }
    }
    HIP_TRYM(hipMemsetAsync(d_ctr, 0, sizeof(DCCounters), s));
    HIP_TRYM(hipMemsetAsync(p->dc_flag.p, 0, ccap, s));
    if (shard_count > 1) HIP_TRYM(hipMemsetAsync(grid.p, 0xff, ncell * sizeof(int), s));  // cells outside the slab read as empty
    HIP_TRYM(hipEventRecord(ev[0], s));
    static const int origin_grid = env_int("GSDF_HIP_DC_ORIGIN_GRID", 0);  // developer knob: workgroups of the origin sweep (1 = tiles strictly in order)
    unsigned g1 = origin_grid > 0 ? (unsigned)origin_grid : grid_for((nslab + lk - 1) / lk, p->num_cu, 32);
    g1 = (g1 + DC_PARTS - 1) / DC_PARTS * DC_PARTS;  // tile T goes to workgroup T % g1, hence to part T % DC_PARTS: what bounds a part's run descriptors (dc_cube_run_seg)
    // Stage 0: the interval test of the sweep's blocks (kernels_dc.h: dc_block_test_kernel), one lane per block of 8 x 8 x K origins.
    // GSDF_HIP_NO_DC_BLOCK_TEST=1: every block is evaluated (developer knob: A/B timing, cross-check in the tests).
    static const bool block_test_off = env_flag("GSDF_HIP_NO_DC_BLOCK_TEST");
    const uint32_t* d_keep = nullptr;
    {
      const uint64_t nblk = (uint64_t)tn[0] * tn[1] * tn[2] * 4ull;
      const int cols = p->prog.nslots + p->prog.lip_depth;
      const size_t lds_t = (size_t)(cols > 0 ? cols : 1) * 2 * BLOCK * sizeof(float);
      // (a tree whose interval stack makes the test ask for more LDS than a CU has goes without it: every block is evaluated)
      if (!block_test_off && nblk > 0 && lds_t <= gsdf_program::kLdsPerCu && p->dc_tile.ensure((size_t)nblk * sizeof(uint32_t)) == hipSuccess) {
        const unsigned gt = grid_for(nblk, p->num_cu, 8);
        HIP_TRYM(launch_kernel(dc_block_test_kernel, p->spec.f_dc_block_test, gt, BLOCK, lds_t, s, p->d_code.p, cols, p->prog.nslots, lk, ox, oy, oz, res, zlo, t0[0], t0[1], t0[2], tn[0],
                               tn[1], tn[2], p->dc_tile.p));
        // ... and "no cube here" in the cleared tiles next to evaluated ones: the cells the later stages read and the sweep does not write
        hipLaunchKernelGGL(dc_grid_clear_kernel, dim3(grid_for((uint64_t)((tn[0] + 3) / 4) * ((tn[1] + 3) / 4) * ((tn[2] + 3) / 4) * BLOCK, p->num_cu, 16)), dim3(BLOCK), 0, s, (int*)grid.p, nshift, lk, zlo, zhi, t0[0], t0[1], t0[2], tn[0], tn[1],
                           tn[2], (const uint32_t*)p->dc_tile.p);
        HIP_TRYM(hipGetLastError());
        d_keep = (const uint32_t*)p->dc_tile.p;
      } else {
        (void)hipGetLastError();
      }
    }
    {  // (a per-tree kernel is the same launch whichever W it was built for)
      const dc_origin_kernel_t aot = dc_origin_aot(gsdf_program::dc_origin_variant(lk));
      if (!aot && !p->spec.f_dc_origin) return bail(fail(GSDF_ERR_BAD_ARGUMENT, "dual contouring: no origin sweep built for this K and W"));
      HIP_TRYM(launch_kernel(aot, p->spec.f_dc_origin, g1, BLOCK, p->lds_bytes(lk) + 32, s, p->d_code.p, p->prog.nslots, nshift, ox, oy, oz, res, grid.p, w0.q0.p, ccap, zlo, zhi, ub, eb[0], eb[1],
                             eb[2], eb[3], eb[4], eb[5], t0[0], t0[1], t0[2], tn[0], tn[1], tn[2], d_ctr, d_keep));
    }
    HIP_TRYM(hipEventRecord(p->dc_ev[0], s));  // origin sweep done
    // (a multiple of DC_PARTS like the sweep's grid: run r goes to workgroup r % grid, hence to the edge list's part r % DC_PARTS --
    // what bounds a part's edge-run descriptors, dc_edge_run_seg)
    const unsigned g_edges = (grid_for(ccap, p->num_cu, 8) + DC_PARTS - 1) / DC_PARTS * DC_PARTS;
    HIP_TRYM(launch_kernel(dc_edges_kernel, p->spec.f_dc_edges, g_edges, BLOCK, p->lds_bytes(3), s, p->d_code.p, w0.q0.p, ccap, ox, oy, oz, res, d2.p, f2.p, e2.p, ecap, p->dc_erun.p, ntiles, grid.p,
                           nshift, p->dc_flag.p, d_ctr));
    HIP_TRYM(hipEventRecord(p->dc_ev[1], s));  // edges done
    HIP_TRYM(launch_kernel(dc_normals_kernel, p->spec.f_dc_normals, grid_for(ecap, p->num_cu, 8), BLOCK, p->lds_bytes(2), s, p->d_code.p, w0.q0.p, d2.p, e2.p, p->dc_erun.p, ccap, ntiles, ox, oy, oz,
                           res, h, n2.p, d_ctr));
    HIP_TRYM(hipEventRecord(p->dc_ev[2], s));  // normals done
    hipLaunchKernelGGL(dc_place_kernel, dim3(grid_for(ccap * 4, p->num_cu, 16)), dim3(DC_BLOCK), 0, s, (const Cube*)w0.q0.p,
                       (unsigned long long)ccap, (const float4*)d2.p, (const int*)grid.p, (const float*)n2.p, nshift, ox, oy, oz, res,
                       sqrtLambda, (float*)f2.p, zown_hi, (const unsigned char*)p->dc_flag.p, d_ctr);
    HIP_TRYM(hipGetLastError());
    HIP_TRYM(hipEventRecord(p->dc_ev[3], s));  // placement done
    if (out_ix) {
      // the quads counted row by row and the rows scanned (kernels_dc_indexed.h, passes A and B); their number comes back with the
      // counters, and the rest of the stage runs once the lists are known to have held
      ixw = DcIndexedWs::of(ecap, nshift);
      HIP_TRYM(p->dc_ix.ensure(ixw.bytes));
      uint8_t* w = (uint8_t*)p->dc_ix.p;
      HIP_TRYM(hipMemsetAsync(w + ixw.row_cnt, 0, ixw.n_rows * 4, s));
      hipLaunchKernelGGL(dci_count_kernel, dim3(grid_for(ecap, p->num_cu, 8)), dim3(BLOCK), 0, s, (const Cube*)w0.q0.p, (const float4*)d2.p, (const unsigned*)e2.p,
                         (unsigned long long)ecap, (const int*)grid.p, nshift, (unsigned*)(w + ixw.row_cnt), (unsigned*)(w + ixw.place), (uint4*)(w + ixw.quad), d_ctr);
      HIP_TRYM(hipGetLastError());
      hipLaunchKernelGGL(dci_row_sum_kernel, dim3(ixw.n_row_blocks), dim3(BLOCK), 0, s, (const unsigned*)(w + ixw.row_cnt), (unsigned)ixw.n_rows,
                         (unsigned*)(w + ixw.blk_cnt));
      HIP_TRYM(hipGetLastError());
      if (int rc = launch_block_scan((const unsigned*)(w + ixw.blk_cnt), ixw.n_row_blocks, (unsigned*)(w + ixw.blk_base), (unsigned long long*)(w + ixw.total), s))
        return bail(rc);
      hipLaunchKernelGGL(dci_row_base_kernel, dim3(ixw.n_row_blocks), dim3(BLOCK), 0, s, (const unsigned*)(w + ixw.row_cnt), (unsigned)ixw.n_rows,
                         (const unsigned*)(w + ixw.blk_base), (unsigned*)(w + ixw.row_base));
      HIP_TRYM(hipGetLastError());
      HIP_TRYM(hipEventRecord(ev[2], s));
      HIP_TRYM(hipMemcpyAsync(&n_quads, w + ixw.total, sizeof n_quads, hipMemcpyDeviceToHost, s));
    } else {
    hipLaunchKernelGGL(dc_quads_kernel, dim3(grid_for(ecap, p->num_cu, 8)), dim3(BLOCK), 0, s, (const Cube*)w0.q0.p, (const float4*)d2.p,
                       (const unsigned*)e2.p, (unsigned long long)ecap, (const int*)grid.p, (const float*)f2.p, nshift, zown_lo, zown_hi,
                       m->d_tris, (unsigned long long)m->cap, d_ctr);
    HIP_TRYM(hipGetLastError());
    HIP_TRYM(hipEventRecord(ev[1], s));
    }
    HIP_TRYM(hipMemcpyAsync(&hc, d_ctr, sizeof(hc), hipMemcpyDeviceToHost, s));
    HIP_TRYM(hipStreamSynchronize(s));
    n_cubes = n_edges = n_cube_runs = n_edge_runs = 0;
    uint64_t max_part = 0;  // the fullest part of the cubes' list: what the capacity has to hold DC_PARTS times
    for (int k = 0; k < DC_PARTS; k++) {
      const uint64_t c = DC_W_COUNT(hc.cubes_w[k * DC_WORD_STRIDE]);
      n_cubes += c; n_edges += DC_W_COUNT(hc.edges_w[k * DC_WORD_STRIDE]);
      n_cube_runs += DC_W_RUNS(hc.cubes_w[k * DC_WORD_STRIDE]); n_edge_runs += DC_W_RUNS(hc.edges_w[k * DC_WORD_STRIDE]);
      if (c > max_part) max_part = c;
    }
    if (hc.q_overflow || hc.t_overflow || max_part > ccap / DC_PARTS) {
      if (attempt >= 8 || ccap >= cmax) return bail(fail(GSDF_ERR_CAPACITY, "dual contouring queue capacity exceeded"));
      // the origin pass keeps counting past the capacity, so the exact number of kept cubes is known (part by part)
      ccap = max_part > ccap / DC_PARTS ? DC_PARTS * (max_part + max_part / 16 + 512) : ccap * 2;
      continue;
    }
    last_cap = DC_PARTS * max_part;
    final_ccap = ccap;
    break;
  }
  if (out_ix) {
    // passes C and D, then the numbering (abi_indexed.hip) -- all of it before the next mesh of this handle overwrites the arenas
    const uint64_t Q = n_quads, ecap = 3 * final_ccap;
    if (Q > n_edges) return bail(fail(GSDF_ERR_HIP, "dual contouring, indexed: internal error (more quads than active edges)"));
    if (Q == 0) return bail(fail(GSDF_ERR_EMPTY_BUFFERS, "empty triangle slice"));
    if (6 * Q >= ((uint64_t)1 << 32)) return bail(fail(GSDF_ERR_CAPACITY, "dual contouring, indexed: 3 x triangles must stay below 2^32 (32-bit vertex numbers)"));
    HIP_TRYM(p->dc_ix_sort.ensure(Q * 8));
    unsigned *xa = (unsigned*)p->dc_ix_sort.p, *src = xa + Q;
    const uint64_t units = (6 * Q * 4 + 35) / 36 + 1;
    uint64_t slot_cap = 0;
    float* slots = pool_take(p->device, units, &slot_cap);
    if (!slots) { HIP_TRYM(hipMalloc((void**)&slots, units * 36)); slot_cap = units; }
    const uint8_t* w = (const uint8_t*)p->dc_ix.p;
    unsigned long long* d_bad = (unsigned long long*)((uint8_t*)p->dc_ix.p + ixw.bad);
    unsigned long long n_bad = 0;
    hipError_t e = hipEventRecord(ev[3], s);
    if (e == hipSuccess) e = hipMemsetAsync(d_bad, 0, 8, s);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(dci_scatter_kernel, dim3(grid_for(ecap, p->num_cu, 8)), dim3(BLOCK), 0, s, (const Cube*)w0.q0.p, (const unsigned*)e2.p, (unsigned long long)ecap,
                         nshift, (const unsigned*)(w + ixw.row_base), (const unsigned*)(w + ixw.place), (unsigned long long)Q, xa, src, d_bad, d_ctr);
      e = hipGetLastError();
    }
    if (e == hipSuccess) {
      hipLaunchKernelGGL(dci_rank_kernel, dim3((unsigned)((Q + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, (const Cube*)w0.q0.p, (const unsigned*)e2.p, (unsigned long long)ecap,
                         nshift, (const unsigned*)(w + ixw.row_base), (const unsigned*)(w + ixw.row_cnt), (const unsigned*)xa, (const unsigned*)src,
                         (const uint4*)(w + ixw.quad), (unsigned long long)Q, (unsigned long long)final_ccap, (unsigned*)slots, d_bad);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(ev[1], s);
    // every slot written, every index in range? (kernels_dc_indexed.h: *bad) -- known before anything reads the slots
    if (e == hipSuccess) e = hipMemcpyAsync(&n_bad, d_bad, sizeof n_bad, hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess || n_bad != 0) {
      (void)hipStreamSynchronize(s);
      pool_give(p->device, slots, slot_cap);
      if (e == hipSuccess) return bail(fail(GSDF_ERR_HIP, "dual contouring, indexed: internal error (" + std::to_string(n_bad) + " quads out of place in the ordering pass)"));
      return bail(fail(GSDF_ERR_HIP, std::string("dual contouring, indexed: the ordering pass: ") + hipGetErrorString(e)));
    }
    const hipEvent_t key_ev[4] = {p->dc_ev[3], ev[2], ev[3], ev[1]};  // passes A + B, passes C + D
    if (int rc = indexed_from_cube_slots(p->device, p->num_cu, s, slots, slot_cap, 6 * Q, final_ccap, (const float*)f2.p, w0.q0.p, key_ev, out_ix)) return bail(rc);
    hc.n_tris = Q;
  }
  float ms = 0;
  HIP_TRYM(hipEventElapsedTime(&ms, ev[0], ev[1]));
  {  // per stage (gsdf_hip_mesh_stage_ms): origin sweep, edges, normals, placement, quads
    const hipEvent_t cut[6] = {ev[0], p->dc_ev[0], p->dc_ev[1], p->dc_ev[2], p->dc_ev[3], ev[1]};
    static const char* const names[5] = {"dc_origin", "dc_edges", "dc_normals", "dc_place", "dc_quads"};
    m->n_stages = 5;
    for (int k = 0; k < 5; k++) {
      float t = 0;
      HIP_TRYM(hipEventElapsedTime(&t, cut[k], cut[k + 1]));
      m->stage_ms[k] = t;
      m->stage_name[k] = names[k];
    }
  }
  {
    static const bool dbg = env_flag("GSDF_HIP_DC_DEBUG");  // developer knob
    if (dbg) fprintf(stderr, "dc: cubes %llu in %llu runs, edges %llu in %llu runs\n", (unsigned long long)n_cubes, (unsigned long long)n_cube_runs,
                     (unsigned long long)n_edges, (unsigned long long)n_edge_runs);
  }
  p->last_dc_cubes = last_cap;  // (DC_PARTS times the fullest part: what the next mesh of this handle sizes its arrays by)
  m->st.n_tris = 2 * hc.n_tris;  // quads -> 2 triangles
  for (int k = 0; k < 64; k++) hc.n_origin_evals += hc.n_origin_part[k * 8];
  m->st.evals = hc.n_origin_evals + 3 * n_cubes + 6 * n_edges;  // (performed: a kept cube's origin is the sweep's evaluation, not repeated by the edge stage)
  m->st.evals_prune = hc.n_origin_evals;  // of the nslab lattice cells; the rest lay outside the exact box by > 2 res
  m->st.evals_leaf = 3 * n_cubes + 6 * n_edges;
  m->st.pruned_leaves = nslab - n_cubes;
  m->st.leaf_cubes = n_cubes;
  m->st.active_leaves = n_edges;
  m->st.ms_total = ms;
  p->evals += m->st.evals;
  *out = m;
  return GSDF_OK;
}

extern "C" int gsdf_hip_mesh_dualcontour(gsdf_program* p, float res, int chiseled, int shard_rank, int shard_count, void* stream,
                                         gsdf_mesh** out) {
  return dc_mesh(p, res, chiseled, shard_rank, shard_count, stream, out, nullptr);
}

extern "C" int gsdf_hip_mesh_dualcontour_indexed(gsdf_program* p, float res, int chiseled, void* stream, gsdf_indexed** out, gsdf_mesh_stats* st) {
  if (out) *out = nullptr;
  if (!p || !out) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  gsdf_mesh* m = nullptr;
  gsdf_indexed* ix = nullptr;
  if (int rc = dc_mesh(p, res, chiseled, 0, 1, stream, &m, &ix)) return rc;
  if (st) *st = m->st;
  gsdf_hip_mesh_destroy(m);  // (it held the statistics; there are no triangles in it)
  *out = ix;
  return GSDF_OK;
}

// glrender.FlatRenderer (flatrenderer.go:36-256) on device: Reset's lattice, evalGrid into a dense grid in HBM,
// ReadTriangles as one marching-cubes pass over every cube. Multi-GPU: z-slabs of cubes like the reference's goroutines
// (:120-122); a rank evaluates the planes its cubes touch (one shared plane per boundary is recomputed, nothing exchanged).
// minecraftRender (glrender/dual_contour.go:297-403): the axis-aligned faces between cubes whose origins lie on different sides of
// the surface. Unexported in the reference and used by one test; here for completeness of row a20. Three steps on the caller's
// stream: the four positions of every level-1 cube to HBM, the program's ordinary Evaluate over them (gsdf_hip_eval3_dev: whatever
// kernels the handle runs), one pass that counts the faces and one that writes them.
extern "C" int gsdf_hip_mesh_minecraft(gsdf_program* p, float res, void* stream, gsdf_mesh** out) {
  if (!p || !out) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *out = nullptr;
  if (p->prog.is2d) return fail(GSDF_ERR_DIMENSION, "program is 2D");
  if (!(res > 0) || std::isnan(res) || std::isinf(res)) return fail(GSDF_ERR_RESOLUTION, "invalid renderer cube resolution");
  if (p->mesh_in_flight()) return fail(GSDF_ERR_BAD_ARGUMENT, "an octree mesh of this program is in flight: wait for it first (shared workspace)");
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t s = stream ? (hipStream_t)stream : p->stream.s;
  // makeICube over the SDF's own bounds (dual_contour.go:298-299; glrender.go:222-235)
  const float* bb = p->prog.bb;
  const float longAxis = fmaxf(bb[3] - bb[0], fmaxf(bb[4] - bb[1], bb[5] - bb[2]));
  const int levels = (int)std::ceil(gsdf::log2f32(longAxis / res)) + 1;
  if (levels <= 1) return fail(GSDF_ERR_RESOLUTION, "resolution not fine enough for marching cubes");
  if (levels > 9) return fail(GSDF_ERR_RESOLUTION, "minecraft render lattice too large: more than 9 octree levels (every cube of the lattice is evaluated)");
  const int nshift = levels - 1;
  const uint64_t n_cubes = (uint64_t)1 << (3 * nshift);
  gsdf_mesh* m = new (std::nothrow) gsdf_mesh();
  if (!m) return fail(GSDF_ERR_BAD_ARGUMENT, "out of memory");
  m->device = p->device; m->stream = s; m->num_cu = p->num_cu;
  m->st.levels = levels; m->st.res = res;
  m->st.origin[0] = bb[0]; m->st.origin[1] = bb[1]; m->st.origin[2] = bb[2];
  float* d_pos = nullptr;
  float* d_dist = nullptr;
  unsigned long long* d_ctr = nullptr;
  auto bail = [&](int code) {
    if (d_pos) (void)hipFree(d_pos);
    if (d_dist) (void)hipFree(d_dist);
    if (d_ctr) (void)hipFree(d_ctr);
    gsdf_hip_mesh_destroy(m);
    return code;
  };
  HIP_TRYM(hipMalloc((void**)&d_pos, n_cubes * 48));
  HIP_TRYM(hipMalloc((void**)&d_dist, n_cubes * 16));
  HIP_TRYM(hipMalloc((void**)&d_ctr, 8));
  const unsigned grid = grid_for(n_cubes, p->num_cu, 16);
  hipLaunchKernelGGL(mcr_positions_kernel, dim3(grid), dim3(BLOCK), 0, s, bb[0], bb[1], bb[2], res, nshift, n_cubes, d_pos);
  HIP_TRYM(hipGetLastError());
  if (int rc = gsdf_hip_eval3_dev(p, d_pos, 12, d_dist, (size_t)(4 * n_cubes), (void*)s)) return bail(rc);
  unsigned long long n_tris = 0;
  for (int pass = 0; pass < 2; pass++) {  // count, then emit into a buffer of exactly that size
    HIP_TRYM(hipMemsetAsync(d_ctr, 0, 8, s));
    hipLaunchKernelGGL(mcr_faces_kernel, dim3(grid), dim3(BLOCK), 0, s, (const float*)d_dist, bb[0], bb[1], bb[2], res, nshift, n_cubes,
                       pass == 0 ? (float*)nullptr : m->d_tris, (unsigned long long)m->cap, d_ctr);
    HIP_TRYM(hipGetLastError());
    HIP_TRYM(hipMemcpyAsync(&n_tris, d_ctr, 8, hipMemcpyDeviceToHost, s));
    HIP_TRYM(hipStreamSynchronize(s));
    if (pass == 0) {
      if (n_tris == 0) break;
      m->d_tris = pool_take(p->device, n_tris, &m->cap);
      if (!m->d_tris) { HIP_TRYM(hipMalloc((void**)&m->d_tris, n_tris * 36)); m->cap = n_tris; }
    }
  }
  m->st.n_tris = n_tris;
  m->st.evals = 4 * n_cubes;
  m->st.leaf_cubes = n_cubes;
  (void)hipFree(d_pos); (void)hipFree(d_dist); (void)hipFree(d_ctr);
  *out = m;
  return GSDF_OK;
}

extern "C" int gsdf_hip_mesh_flat(gsdf_program* p, float res, int shard_rank, int shard_count, void* stream, gsdf_mesh** out) {
  if (!p || !out) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *out = nullptr;
  spec_adopt(p);  // (a background build that has finished: its kernels from here on)
  if (p->prog.is2d) return fail(GSDF_ERR_DIMENSION, "program is 2D");
  if (!(res > 0) || std::isnan(res) || std::isinf(res)) return fail(GSDF_ERR_RESOLUTION, "invalid renderer cube resolution");
  if (shard_count < 1 || shard_rank < 0 || shard_rank >= shard_count) return fail(GSDF_ERR_BAD_ARGUMENT, "bad shard rank/count");
  if (p->mesh_in_flight()) return fail(GSDF_ERR_BAD_ARGUMENT, "an octree mesh of this program is in flight: wait for it first (shared workspace)");
  HIP_TRY(hipSetDevice(p->device));
  hipStream_t s = stream ? (hipStream_t)stream : p->stream.s;
  // Reset (:36-80)
  float mn[3], mx[3];
  scale_centered(p->prog.bb, 1.01f, mn, mx);
  double nd[3];
  for (int a = 0; a < 3; a++) nd[a] = (double)std::ceil((mx[a] - mn[a]) / res);
  if (!(nd[0] > 0) || !(nd[1] > 0) || !(nd[2] > 0)) return fail(GSDF_ERR_RESOLUTION, "resolution not fine enough for marching cubes");
  if (nd[0] > 65534 || nd[1] > 65534 || nd[2] > 1e9 || (nd[0] + 1) * (nd[1] + 1) >= 4294967296.0)
    return fail(GSDF_ERR_RESOLUTION, "resolution too fine for the flat renderer's lattice");
  const unsigned nx = (unsigned)nd[0], ny = (unsigned)nd[1], nz = (unsigned)nd[2];
  const unsigned sx = nx + 1, sy = ny + 1;
  const uint64_t sxy = (uint64_t)sx * sy;
  const uint64_t pxy = (uint64_t)FLAT_PITCH(sx) * sy;  // the grid's rows are padded to 256 bytes
  const float ox = mn[0], oy = mn[1], oz = mn[2];
  // this rank's cubes in z and the lattice planes they touch
  uint32_t c0 = 0, c1 = 0;
  gsdf_hip_slab_range(nz, (uint32_t)shard_rank, (uint32_t)shard_count, &c0, &c1);
  const unsigned ncz = c1 - c0, nk = ncz ? ncz + 1 : 0;

  gsdf_mesh* m = new (std::nothrow) gsdf_mesh();
  if (!m) return fail(GSDF_ERR_BAD_ARGUMENT, "out of memory");
  m->device = p->device; m->stream = s; m->num_cu = p->num_cu;
  m->st.levels = 0; m->st.res = res;
  m->st.origin[0] = ox; m->st.origin[1] = oy; m->st.origin[2] = oz;
  auto bail = [&](int code) { gsdf_hip_mesh_destroy(m); return code; };
  if (ncz == 0) { *out = m; return GSDF_OK; }  // more ranks than cube planes: nothing for this one
  gsdf_program::OctreeWs& w0 = p->ws[0];  // its counters and its events serve here too (no octree mesh is in flight)
  const EventSet<5>& ev = w0.ev;
  HIP_TRYM(w0.ev.ensure());
  HIP_TRYM(w0.ctr.ensure(sizeof(MeshCounters)));
  MeshCounters* d_ctr = (MeshCounters*)w0.ctr.p;
  {
    // refuse up front what cannot fit (a failed multi-hundred-GB hipMalloc is slow and leaves the allocator fragmented)
    size_t mfree = 0, mtotal = 0;
    const double need = (double)pxy * (double)nk * sizeof(float);
    if (hipMemGetInfo(&mfree, &mtotal) == hipSuccess && need > (double)mfree + (double)p->flat_grid.cap)
      return bail(fail(GSDF_ERR_CAPACITY, "flat renderer: the distance grid (" + std::to_string((unsigned long long)(need / 1e9)) +
                                              " GB) does not fit the device memory; use the octree renderer at this resolution"));
  }
  if (p->flat_grid.ensure(pxy * nk * sizeof(float)) != hipSuccess) {
    (void)hipGetLastError();
    return bail(fail(GSDF_ERR_CAPACITY, "flat renderer: no device memory for the distance grid (" + std::to_string(pxy * nk * 4) + " bytes)"));
  }
  float* grid = (float*)p->flat_grid.p;
  // two bit planes per lattice plane beside it (1/32 + 1/32 of the grid's size): "d < 0" and "|d| <= 2 sqrt3 res" per corner,
  // in whole words per flat_grid_kernel pass (BLOCK corners = BLOCK / 64 words)
  const unsigned wpp = (unsigned)((sxy + (uint64_t)BLOCK - 1) / (uint64_t)BLOCK) * (BLOCK / 64);
  if (p->flat_bits.ensure((size_t)2 * wpp * nk * sizeof(unsigned long long)) != hipSuccess) {
    (void)hipGetLastError();
    return bail(fail(GSDF_ERR_CAPACITY, "flat renderer: no device memory for the lattice's bit planes"));
  }
  unsigned long long* negbits = (unsigned long long*)p->flat_bits.p;
  unsigned long long* nearbits = negbits + (size_t)wpp * nk;
  const int ek = p->batch_k();
  spec_ensure(p, SPEC_AUX);
  HIP_TRYM(hipEventRecord(ev[0], s));
  {
    const uint64_t npass = ((sxy + (uint64_t)BLOCK - 1) / (uint64_t)BLOCK) * ((nk + ek - 1) / ek);
    static const int bpc = env_int("GSDF_HIP_EVAL_BPC", 64);
    const uint64_t gmax = (uint64_t)p->num_cu * (uint64_t)(bpc > 0 ? bpc : 64);
    const unsigned g = (unsigned)(npass < gmax ? npass : gmax);
    HIP_TRYM(launch_kernel(flat_grid_aot(p->sweep_variant(ek)), p->spec.f_flat_grid, g, BLOCK, p->lds_bytes(ek), s, p->d_code.p, ox, oy, oz, res, sx, sy, c0, nk, grid, negbits, nearbits));
  }
  HIP_TRYM(hipEventRecord(ev[1], s));
  // ReadTriangles: the triangle count is not known in advance; the pass is cheap (HBM-bound over the grid), so a
  // buffer that turns out too small is replaced by one of the exact size and only this pass is repeated.
  MeshCounters hc{};
  uint64_t want = p->last_tris ? p->last_tris + p->last_tris / 16 + 1024 : (uint64_t)1 << 20;
  float ms_march = 0;
  for (int attempt = 0;; attempt++) {
    if (!m->d_tris) {
      m->d_tris = pool_take(p->device, want, &m->cap);
      if (!m->d_tris) { HIP_TRYM(hipMalloc((void**)&m->d_tris, want * 36)); m->cap = want; }
    }
    HIP_TRYM(hipMemsetAsync(d_ctr, 0, sizeof(MeshCounters), s));
    HIP_TRYM(hipEventRecord(ev[2], s));
    // the marching pass over the bit planes: flat_cut_scan_kernel + flat_march_list_kernel
    if (nx >= 65536u || ny >= 65536u || (uint64_t)c0 + ncz >= 65536u)  // record coordinates are 16-bit
      return bail(fail(GSDF_ERR_RESOLUTION, "resolution too fine for the flat renderer's lattice"));
    // a cut cube has at least one triangle: a list of the triangle buffer's capacity overflows only if that does
    if (p->flat_list.ensure((size_t)m->cap * sizeof(unsigned long long)) != hipSuccess) {
      (void)hipGetLastError();
      return bail(fail(GSDF_ERR_CAPACITY, "flat renderer: no device memory for the list of cut cubes"));
    }
    unsigned long long* list = (unsigned long long*)p->flat_list.p;
    const uint64_t npass = (((uint64_t)sx * ny + 4095u) >> 12) * ncz;  // wave passes of the scan: 4096 cubes each
    static const int sbpc = env_int("GSDF_HIP_FLAT_SCAN_BPC", 16), lbpc = env_int("GSDF_HIP_FLAT_LIST_BPC", 6);  // tuning knobs
    const uint64_t gmax = (uint64_t)p->num_cu * (uint64_t)(sbpc > 0 ? sbpc : 16), nwg = (npass + 3) / 4;
    hipLaunchKernelGGL(flat_cut_scan_kernel, dim3((unsigned)(nwg < gmax ? (nwg ? nwg : 1) : gmax)), dim3(BLOCK), 0, s, (const unsigned long long*)negbits,
                       (const unsigned long long*)nearbits, wpp, nx, ny, ncz, list, (uint64_t)m->cap, d_ctr);
    hipLaunchKernelGGL(flat_march_list_kernel, dim3((unsigned)p->num_cu * (unsigned)(lbpc > 0 ? lbpc : 6)), dim3(BLOCK), FLATB_LDS_BYTES, s, (const float*)grid,
                       (const unsigned long long*)list, (uint64_t)m->cap, nx, ny, c0, ox, oy, oz, res, m->d_tris, (uint64_t)m->cap, d_ctr);
    HIP_TRYM(hipGetLastError());
    HIP_TRYM(hipEventRecord(ev[3], s));
    HIP_TRYM(hipMemcpyAsync(&hc, d_ctr, sizeof(hc), hipMemcpyDeviceToHost, s));
    HIP_TRYM(hipStreamSynchronize(s));
    if (hc.overflow) {
      // The marching pass keeps counting: n_tris is exact as long as its cut-cube list held every cut cube
      // (n_cut <= capacity); if not, n_cut is still exact and n_tris covers the listed cubes only: a cut cube
      // has 1 to 5 triangles (2.2 on the configs' surfaces), so room for 3 per cut cube holds the list for certain and
      // the triangles nearly always -- one more exact rerun otherwise.
      if (attempt >= 5) return bail(fail(GSDF_ERR_CAPACITY, "device triangle buffer capacity exceeded"));
      const bool list_short = hc.n_cut > m->cap;
      pool_give(p->device, m->d_tris, m->cap);
      m->d_tris = nullptr; m->cap = 0;
      want = hc.n_tris + hc.n_tris / 16 + 1024;
      if (list_short && want < 3 * hc.n_cut) want = 3 * hc.n_cut;
      continue;
    }
    break;
  }
  float ms_grid = 0;
  HIP_TRYM(hipEventElapsedTime(&ms_march, ev[2], ev[3]));  // the last (successful) marching pass
  HIP_TRYM(hipEventElapsedTime(&ms_grid, ev[0], ev[1]));
  m->st.n_tris = hc.n_tris;
  m->st.evals = sxy * nk;  // FlatRenderer.Evaluations(): every lattice corner once
  m->st.evals_prune = 0;
  m->st.evals_leaf = m->st.evals;
  m->st.pruned_leaves = 0;
  m->st.leaf_cubes = (uint64_t)nx * ny * ncz;
  m->st.active_leaves = hc.n_active;
  m->st.ms_prune = 0;
  m->st.ms_leaf = ms_grid;
  m->st.ms_march = ms_march;
  m->st.ms_total = (double)ms_grid + (double)ms_march;
  p->evals += m->st.evals;
  p->last_tris = hc.n_tris;
  *out = m;
  return GSDF_OK;
}

// Pure host helper (no GPU): owner rank of the brick (x,y,z) under the multi-GPU partition that
// gsdf_hip_mesh_octree applies on device (same function, SURVEY 8(e): no data-path collective).
// Pure host helper (no GPU): the z-slab [lo, hi) of n lattice planes that rank `rank` of `count` owns in the flat
// renderer and in dual contouring -- contiguous, disjoint, covering [0, n); ranks beyond n get empty slabs.
extern "C" void gsdf_hip_slab_range(uint32_t n, uint32_t rank, uint32_t count, uint32_t* lo, uint32_t* hi) {
  if (!count || rank >= count) { if (lo) *lo = 0; if (hi) *hi = 0; return; }
  if (lo) *lo = (uint32_t)(((uint64_t)n * (uint64_t)rank) / (uint64_t)count);
  if (hi) *hi = (uint32_t)(((uint64_t)n * (uint64_t)(rank + 1)) / (uint64_t)count);
}

extern "C" uint32_t gsdf_hip_brick_owner(uint32_t x, uint32_t y, uint32_t z, uint32_t count) {
  return count ? brick_owner(x, y, z, count) : 0;
}

static const char* const kRecordsMsg = "the mesh holds cut-leaf records, not triangles yet: gsdf_hip_mesh_march it, or gather it";
extern "C" int gsdf_hip_mesh_stats_get(const gsdf_mesh* m, gsdf_mesh_stats* st) {
  if (!m || !st) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *st = m->st;
  return GSDF_OK;
}
extern "C" int gsdf_hip_mesh_read(const gsdf_mesh* m, uint64_t first, uint64_t count, float* dst) {
  if (!m || (!dst && count)) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (m->payload == GSDF_PAYLOAD_RECORDS) return fail(GSDF_ERR_BAD_ARGUMENT, kRecordsMsg);
  if (first + count > m->st.n_tris) return fail(GSDF_ERR_BAD_ARGUMENT, "triangle range out of bounds");
  if (count == 0) return GSDF_OK;
  // The reference's pull loop (glrender.RenderAll: 4096 triangles per ReadTriangles call) would issue ~1700 small
  // device-to-host copies at resdiv 1600. Partial reads are served from the mesh's pinned host copy instead: one DMA
  // on the first call, plain memcpy afterwards.
  // A read of (nearly) everything takes the same route, with a multi-threaded copy out of the pinned buffer (a pageable
  // hipMemcpy is staged by the runtime at ~12 GB/s).
  {
    const float* h = nullptr;
    if (gsdf_hip_mesh_host_tris(const_cast<gsdf_mesh*>(m), &h) == GSDF_OK) {
      big_memcpy(dst, h + first * 9, count * 36);  // single memcpy below 32 MB
      return GSDF_OK;
    }
  }
  HIP_TRY(hipSetDevice(m->device));  // no pinned memory to be had: plain copy from the device
  HIP_TRY(hipMemcpy(dst, m->d_tris + first * 9, count * 36, hipMemcpyDeviceToHost));
  return GSDF_OK;
}
extern "C" const float* gsdf_hip_mesh_dev_tris(const gsdf_mesh* m) { return m ? m->d_tris : nullptr; }

extern "C" int gsdf_hip_mesh_stl(const gsdf_mesh* m, uint8_t* dst, size_t dst_cap) {
  if (!m || !dst) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  const uint64_t n = m->st.n_tris;
  if (n == 0) return fail(GSDF_ERR_EMPTY_BUFFERS, "empty triangle slice");
  if (n > 0xffffffffull) return fail(GSDF_ERR_BAD_ARGUMENT, "amount of triangles in model exceeds STL design limits");
  const size_t bytes = 84 + 50 * (size_t)n;
  if (dst_cap < bytes) return fail(GSDF_ERR_SHORT_BUFFER, "short buffer");
  // built on device and moved into the mesh's pinned host buffer (gsdf_hip_mesh_host_stl), then copied out
  const uint8_t* h = nullptr;
  size_t len = 0;
  const int rc = gsdf_hip_mesh_host_stl(const_cast<gsdf_mesh*>(m), &h, &len);
  if (rc) return rc;
  big_memcpy(dst, h, len);
  return GSDF_OK;
}

extern "C" int gsdf_hip_mesh_host_tris(gsdf_mesh* m, const float** tris) {
  if (!m || !tris) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *tris = nullptr;
  if (m->payload == GSDF_PAYLOAD_RECORDS) return fail(GSDF_ERR_BAD_ARGUMENT, kRecordsMsg);
  const uint64_t n = m->st.n_tris;
  if (n == 0) return GSDF_OK;
  if (m->host_out) {  // the mesher wrote them there
    *tris = m->d_tris;
    return GSDF_OK;
  }
  HIP_TRY(hipSetDevice(m->device));
  if (!m->h_tris) {
    const int rc = host_buf(&m->h_tris, &m->h_tris_cap, (size_t)n * 36);
    if (rc) return rc;
    hipStream_t rs = mesh_stream(m);
    hipError_t e = hipMemcpyAsync(m->h_tris, m->d_tris, (size_t)n * 36, hipMemcpyDeviceToHost, rs);
    if (e == hipSuccess) e = hipStreamSynchronize(rs);
    if (e != hipSuccess) { hpool_give(m->h_tris, m->h_tris_cap); m->h_tris = nullptr; m->h_tris_cap = 0; return fail(GSDF_ERR_HIP, std::string("D2H triangles: ") + hipGetErrorString(e)); }
  }
  *tris = (const float*)m->h_tris;
  return GSDF_OK;
}

extern "C" int gsdf_hip_mesh_host_stl(gsdf_mesh* m, const uint8_t** stl, size_t* len) {
  if (!m || !stl || !len) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *stl = nullptr; *len = 0;
  if (m->payload == GSDF_PAYLOAD_RECORDS) return fail(GSDF_ERR_BAD_ARGUMENT, kRecordsMsg);
  const uint64_t n = m->st.n_tris;
  if (n == 0) return fail(GSDF_ERR_EMPTY_BUFFERS, "empty triangle slice");
  if (n > 0xffffffffull) return fail(GSDF_ERR_BAD_ARGUMENT, "amount of triangles in model exceeds STL design limits");
  const size_t bytes = 84 + 50 * (size_t)n;
  HIP_TRY(hipSetDevice(m->device));
  if (!m->h_stl) {
    int rc = host_buf(&m->h_stl, &m->h_stl_cap, bytes);
    if (rc) return rc;
    // device scratch for the records from the triangle-buffer pool (sized in 36-byte units)
    const uint64_t units = (bytes + 4 + 35) / 36;
    uint64_t dcap = 0;
    float* d_out = pool_take(m->device, units, &dcap);
    if (!d_out) {
      if (hipMalloc((void**)&d_out, units * 36) != hipSuccess) { (void)hipGetLastError(); return fail(GSDF_ERR_HIP, "hipMalloc of the STL scratch failed"); }
      dcap = units;
    }
    uint8_t* hdr = (uint8_t*)m->h_stl;  // pinned: a valid source for the async header upload
    std::memset(hdr, 0, 84);
    const uint32_t cnt = (uint32_t)n;
    std::memcpy(hdr + 80, &cnt, 4);
    hipStream_t rs = mesh_stream(m);
    hipError_t e = hipMemcpyAsync(d_out, hdr, 84, hipMemcpyHostToDevice, rs);
    if (e == hipSuccess) {
      hipLaunchKernelGGL(stl_kernel, dim3(grid_for(n, m->num_cu, 8)), dim3(BLOCK), 0, rs, m->d_tris, n, (uint8_t*)d_out);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(m->h_stl, d_out, bytes, hipMemcpyDeviceToHost, rs);
    if (e == hipSuccess) e = hipStreamSynchronize(rs);
    pool_give(m->device, d_out, dcap);
    if (e != hipSuccess) { hpool_give(m->h_stl, m->h_stl_cap); m->h_stl = nullptr; m->h_stl_cap = 0; return fail(GSDF_ERR_HIP, std::string("STL build/transfer: ") + hipGetErrorString(e)); }
  }
  *stl = (const uint8_t*)m->h_stl;
  *len = bytes;
  return GSDF_OK;
}

static void mesh_free(gsdf_mesh* m) {
  release_tris(m);
  pool_give(m->device, (float*)m->d_recs, m->recs_cap36);
  pool_give(m->device, (float*)m->d_wrecs, m->wrecs_cap36);
  hpool_give(m->h_tris, m->h_tris_cap);
  hpool_give(m->h_stl, m->h_stl_cap);
  if (m->rstream) (void)hipStreamDestroy(m->rstream);
  delete m;
}
extern "C" void gsdf_hip_mesh_destroy(gsdf_mesh* m) {
  if (!m) return;
  // a gather may still be reading the buffers (gsdf_hip_mesh_gatherv_start .. _wait): the last reference frees them
  if (m->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) mesh_free(m);
}
void mesh_inflight_done(gsdf_mesh* m) {
  m->inflight.fetch_sub(1);
  if (m->refs.fetch_sub(1, std::memory_order_acq_rel) == 1) mesh_free(m);
}
