// abi_spec.hip -- C ABI (include/gsdf_hip.h), the per-tree ("specialised") kernels of a program handle: the first group's build
// (gsdf_hip_program_specialize), the same in the background and its adoption, the groups built on first use (spec_ensure), the report
// of what a handle launches (gsdf_hip_program_kernels), the host-only source / check entry points. Host code only: this unit owns no
// kernel and launches none; what it builds is kept in gsdf_program::spec (abi_program.h: SpecKernels) and launched by the other units.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <new>

#include "kernels_common.h"
#include "abi_program.h"

static std::string device_arch(int device) {
  hipDeviceProp_t pr;
  if (hipGetDeviceProperties(&pr, device) != hipSuccess) return "gfx950";
  std::string arch = pr.gcnArchName;
  if (arch.find(':') != std::string::npos) arch = arch.substr(0, arch.find(':'));
  return arch;
}

// hiprtc build + module load of `names` for the handle's program; fns receives one function per name.
static int spec_build(gsdf_program* p, const std::vector<std::string>& names, hipModule_t* mod_out, std::vector<hipFunction_t>& fns) {
  std::vector<char> co;
  std::vector<std::string> low;
  std::string log;
  const auto t0 = std::chrono::steady_clock::now();
  if (!gsdf_dev::spec_compile(p->prog, device_arch(p->device), names, co, low, log)) return fail(GSDF_ERR_HIP, "specialised build failed:\n" + log);
  p->spec.compile_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  hipModule_t mod = nullptr;
  HIP_TRY(hipModuleLoadData(&mod, co.data()));
  fns.assign(names.size(), nullptr);
  for (size_t i = 0; i < names.size(); i++) {
    hipError_t e = hipModuleGetFunction(&fns[i], mod, low[i].c_str());
    if (e != hipSuccess) {
      (void)hipModuleUnload(mod);
      return fail(GSDF_ERR_HIP, std::string("hipModuleGetFunction: ") + hipGetErrorString(e));
    }
  }
  *mod_out = mod;
  return GSDF_OK;
}

// Scratch (private segment) bytes per lane of a built kernel. A specialised kernel is used only if this is 0: its code
// shape is new for every tree, and a build that spills registers inside divergent regions has been seen to lose the
// spilled values of the lanes that were inactive at the spill (2-D fuzz tree 708: eval_kernel<2,4,4>, 128 VGPRs + 132 B
// of scratch, wrote the results of 216 points of a ragged last tile to the wrong addresses). The ahead-of-time
// interpreter kernels have ONE code shape each, and that shape is what the whole test suite runs.
static int fn_scratch_bytes(hipFunction_t f) {
  static const bool allow = env_set("GSDF_HIP_EXP_ALLOW_SCRATCH");  // developer experiments only: timing of a spilling build
  if (allow) return 0;
  int v = 0;
  if (hipFuncGetAttribute(&v, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, f) != hipSuccess) { (void)hipGetLastError(); return 1 << 30; }
  return v;
}
// No scratch, or not used (see fn_scratch_bytes); `take` says whether a usable build was wanted. The GSDF_HIP_DEBUG line says both.
template <typename Take>
static bool spec_usable(const std::string& name, hipFunction_t f, Take take) {
  const int scratch = fn_scratch_bytes(f);
  const bool used = scratch == 0 && take();
  if (env_set("GSDF_HIP_DEBUG")) {
    int regs = -1;
    (void)hipFuncGetAttribute(&regs, HIP_FUNC_ATTRIBUTE_NUM_REGS, f);
    fprintf(stderr, "gsdf_hip: specialised %s: %d registers, %d B scratch per lane -> %s\n", name.c_str(), regs, scratch, used ? "used" : "not used (interpreter kernel instead)");
  }
  return used;
}
// One kernel a group asks for: its name expression, the handle's function it is for, and the W / BOTH it was instantiated with where
// the handle records them.
struct SpecCand { std::string name; hipFunction_t* dst; int w = 0; bool both = false; };
// The shared tail of every build after the first: the candidates built into one module the handle keeps; in their order, a usable
// kernel is taken unless an earlier candidate has filled its function already (first usable wins), and taken(c) hears of it. A failed
// build takes nothing: the interpreter kernels stay in use.
template <typename Taken>
static void spec_build_group(gsdf_program* p, const std::vector<SpecCand>& cs, Taken taken) {
  std::vector<std::string> names;
  for (const SpecCand& c : cs) names.push_back(c.name);
  std::vector<hipFunction_t> f;
  hipModule_t mod = nullptr;
  if (names.empty() || spec_build(p, names, &mod, f) != GSDF_OK) return;
  p->spec.mods.push_back(mod);
  for (size_t i = 0; i < cs.size(); i++)
    spec_usable(names[i], f[i], [&] { if (*cs[i].dst) return false; *cs[i].dst = f[i]; taken(cs[i]); return true; });
}

// The on-first-use groups (abi_program.h: SpecGroup). Each case states what its group applies to and the kernels it asks for; the
// guard, the lock, the build, the scratch rule and the debug line are the same for all. The lock is the one under which the
// host-buffer calls -- the only entry points that run on several threads at once -- read their kernels (abi_eval.hip: eval_dev) and
// under which a background build is adopted, so a group's flag, its functions and those readers are under ONE mutex; every other
// group has one caller at a time (gsdf_hip.h) and takes it for uniformity. Each group has a module of its own: the first group's
// build key -- the handle's code identity -- stays what it is.
void spec_ensure(gsdf_program* p, SpecGroup g) {
  SpecKernels& k = p->spec;
  const unsigned bit = 1u << g;
  if (!(k.todo.load(std::memory_order_acquire) & bit)) return;  // not specialised, or tried already: the 20 us host-buffer call pays this load only
  std::lock_guard<std::mutex> lk(p->spec_async_mu);
  if (!(k.todo.load(std::memory_order_relaxed) & bit)) return;  // another thread of the caller was faster
  const bool is2d = p->prog.is2d;
  const int ek = p->batch_k();
  const gsdf_program::LeafConfig c = p->leaf_config();
  std::vector<SpecCand> cs;
  switch (g) {
    case SPEC_AUX:  // (both sweeps are built for sweep_variant's W; dual contouring's launch is the same whichever W its kernel was built for)
      if (is2d) cs = {{"image2_kernel<" + std::to_string(ek) + ">", &k.f_image}};
      else cs = {{p->sweep_variant(ek).spec_name("dc_origin_kernel"), &k.f_dc_origin}, {"dc_edges_kernel", &k.f_dc_edges}, {"dc_normals_kernel", &k.f_dc_normals},
                 {"normals_kernel", &k.f_normals}, {p->sweep_variant(ek).spec_name("flat_grid_kernel"), &k.f_flat_grid}, {"dc_block_test_kernel", &k.f_dc_block_test}};
      break;
    case SPEC_ROWS: {
      // leaf_eval_kernel with distinct z rows for a handle whose leaf phase runs four points per lane through its own kernel: the
      // one-body form at the occupancy that kernel has, then at the configured one, then the two-site form at each; the first that builds
      // without scratch is taken. If none does (knurled-cylinder with hipcc 7.2: three variants of the second pass in one body want more
      // than 128 registers; at three workgroups per CU the option costs more than it saves) every row keeps going through f_leaf.
      if (is2d || c.k != 4 || !k.f_leaf || k.leaf_k != 4) break;
      auto add = [&](int w, bool b) {
        for (const SpecCand& v : cs) if (v.w == w && v.both == b) return;
        cs.push_back({LeafVariant{4, w, true, c.ntlds, b, true}.spec_name(), &k.f_leaf_dz, w, b});
      };
      if (k.leaf_both) { add(k.leaf_w, true); add(c.w, true); }
      add(k.leaf_w, false); add(c.w, false);
      break;
    }
    case SPEC_EVAL_K1:  // one point per lane, what host-mapped Evaluate calls run (eval_dev); a handle whose K is 1 has it already
      if (ek != 1) cs = {{SweepVariant{1, 4}.spec_name("eval_kernel", is2d ? 2 : 3), &k.f_eval_k1}};
      break;
    case SPEC_DENSE:  // at the most workgroups per CU the LDS allows for which the compiler needs no scratch
      for (int w = 5; w >= 3 && !is2d; w--)
        if ((size_t)w * p->lds_dense() <= gsdf_program::kLdsPerCu) cs.push_back({"leaf_dense_kernel<" + std::to_string(w) + ", true, true>", &k.f_leaf_dense, w});
      break;
    case SPEC_VIEW:  // both forms; this module and the next two include their own kernel header only (specialize.cpp: spec_includes)
      if (!is2d) cs = {{"view_kernel<true>", &k.f_view}, {"view_kernel<false>", &k.f_view_plain}};
      break;
    case SPEC_PROJECT:
      if (!is2d) cs = {{"project_kernel", &k.f_project}};
      break;
    case SPEC_RAY:  // both forms: the caller's rays, and the rays of a mesh's vertices (wall thickness)
      if (!is2d) cs = {{"ray_kernel<false>", &k.f_ray}, {"ray_kernel<true>", &k.f_ray_thick}};
      break;
    case SPEC_PICTURE:
      for (int kind = 0; kind < 4 && is2d; kind++) cs.push_back({"image2_color_kernel<" + std::to_string(ek) + ", " + std::to_string(kind) + ">", &k.f_imgc[kind]});
      break;
    case SPEC_GROUPS: break;
  }
  spec_build_group(p, cs, [&](const SpecCand& t) {
    if (g == SPEC_ROWS) { k.rows_w = t.w; k.rows_both = t.both; }
    if (g == SPEC_DENSE) k.dense_w = t.w;
  });
  k.todo.fetch_and(~bit, std::memory_order_release);
}

// straight-line code grows with the program (multi-evaluation nodes are unrolled at lowering time): beyond a few
// thousand instructions the build takes minutes and the code no longer fits the instruction cache
static int spec_refused(const gsdf_program* p) {
  if (gsdf_dev::spec_instruction_count(p->prog) <= 4000) return GSDF_OK;
  return fail(GSDF_ERR_BAD_TREE, "program too large to specialise (more than 4000 instructions): the interpreter kernels stay in use");
}

// Compile and load kernels specialised for this handle's program (specialize.cpp): eval, prune and leaf kernels of
// the configuration the mesher would pick. Afterwards gsdf_hip_eval*/gsdf_hip_mesh_octree launch them instead of the
// interpreter kernels; results are bit-identical (same statements, same compiler flags). Idempotent.
extern "C" int gsdf_hip_program_specialize(gsdf_program* p) {
  if (!p) return fail(GSDF_ERR_BAD_ARGUMENT, "null program");
  SpecKernels& k = p->spec;
  if (k.specialised()) return GSDF_OK;
  if (int rc = spec_refused(p)) return rc;
  HIP_TRY(hipSetDevice(p->device));
  const gsdf_program::LeafConfig c = p->leaf_config();
  const int lk = c.k, lw = c.w, dim = p->prog.is2d ? 2 : 3;
  const SweepVariant ev = p->sweep_variant(p->batch_k());
  const LeafVariant leaf{lk, lw, true, c.ntlds, false, false};  // the configuration the mesher would pick
  auto leaf_with = [&](int w, bool both) { LeafVariant v = leaf; v.w = w; v.both = both; return v; };
  std::vector<std::string> names{ev.spec_name("eval_kernel", dim)};
  std::vector<LeafVariant> leaves;  // the leaf kernel's candidates: each later one that builds without scratch is preferred to the ones before it
  if (!p->prog.is2d) {
    names.push_back("prune_kernel");
    names.push_back("prune_spec_kernel");
    leaves.push_back(leaf);
    const bool room5 = lk == 4 && lw == 4 && 5 * c.lds <= gsdf_program::kLdsPerCu;
    // a fifth workgroup per CU where the LDS has room for it (npt-flange's 7 slots): the 96-register build is taken if the
    // compiler reaches it without scratch (-3 % on the evaluating kernel); built beside the 128-register one, same process
    if (room5) leaves.push_back(leaf_with(5, false));
    // both passes of a column brick in one body -- taken, ahead of the others, if the compiler reaches it without scratch: -7 %
    // where much of the program depends on x and y alone (an atan2, several hypots: npt-flange), -1..2 % elsewhere
    static const bool both_off = env_flag("GSDF_HIP_NO_BOTH_PASSES");  // developer knob (A/B timing)
    static const int both_min = env_int("GSDF_HIP_BOTH_MIN_WEIGHT", 0);  // developer knob. 0: always -- programs without x,y-only work gain 1-2 % too (bolt 1.029 -> 1.007 ms, knurled-cylinder 3.19 -> 3.16: one body of eight points schedules a little better than two of four)
    if (!both_off && lk == 4 && gsdf_dev::spec_xy_shared_weight(p->prog) >= both_min) {
      leaves.push_back(leaf_with(lw, true));
      // ... and at five workgroups per CU (96 registers) where the LDS has room: taken if it builds without scratch
      static const bool both5_off = env_flag("GSDF_HIP_NO_BOTH5");  // developer knob (A/B timing)
      if (!both5_off && room5) leaves.push_back(leaf_with(5, true));
    }
    for (const LeafVariant& v : leaves) names.push_back(v.spec_name());
  }
  std::vector<hipFunction_t> f;
  hipModule_t mod = nullptr;
  if (int rc = spec_build(p, names, &mod, f)) return rc;
  k.mods.push_back(mod);  // (from here on the handle is specialised)
  k.compiler = gsdf_dev::spec_last_compiler();
  k.key = gsdf_dev::spec_last_key();
  k.eval_k = ev.k; k.eval_w = ev.w; k.leaf_k = lk; k.leaf_w = lw;
  auto yes = [] { return true; };
  // No scratch, or not used (see fn_scratch_bytes). The eval kernel gets a second chance with the larger register
  // budget of 3 workgroups per CU before the handle falls back to the interpreter kernel for that entry point.
  if (spec_usable(names[0], f[0], yes)) k.f_eval = f[0];
  else if (ev.w == 4) spec_build_group(p, {{SweepVariant{ev.k, 3}.spec_name("eval_kernel", dim), &k.f_eval}}, [&](const SpecCand&) { k.eval_w = 3; });
  if (!p->prog.is2d) {
    if (spec_usable(names[1], f[1], yes)) k.f_prune = f[1];
    if (spec_usable(names[2], f[2], yes)) k.f_prune_spec = f[2];
    for (size_t i = 0; i < leaves.size(); i++)
      if (spec_usable(names[3 + i], f[3 + i], yes)) { k.f_leaf = f[3 + i]; k.leaf_w = leaves[i].w; k.leaf_both = leaves[i].both; }
    // the leaf kernel is where the time goes: before giving it up, trade occupancy for registers (W = workgroups per CU
    // the register budget is sized for; the launch is the same)
    for (int w2 = lw - 1; !k.f_leaf && w2 >= 2; w2--) {
      std::vector<hipFunction_t> fl;
      hipModule_t m2 = nullptr;
      const std::string nl = leaf_with(w2, false).spec_name();
      if (spec_build(p, {nl}, &m2, fl) != GSDF_OK) break;
      if (spec_usable(nl, fl[0], yes)) { k.f_leaf = fl[0]; k.leaf_w = w2; k.mods.push_back(m2); }
      else (void)hipModuleUnload(m2);
    }
  }
  k.todo.store((1u << SPEC_GROUPS) - 1u, std::memory_order_release);  // every group is still to be tried, at its first use
  return GSDF_OK;
}
// ---- specialisation in the background -----------------------------------------------------------------------------------------
// Every example of the reference is one tree -> one mesh -> one file (examples/npt-flange/flange.go:61-98): a caller that waits for
// a compiler before its only mesh has gained nothing. _async starts the build (and the module load) on a thread of its own and
// returns; the handle keeps meshing and evaluating through the interpreter kernels and switches to the specialised ones at the
// first entry-point call after they are ready -- same bits either way (same statements, same flags), so a mesh may even change
// kernels between its attempts. With GSDF_HIP_CACHE_DIR set and the tree seen before, "ready" is a file read away.
void spec_adopt_slow(gsdf_program* p) {
  std::lock_guard<std::mutex> lk(p->spec_async_mu);
  if (p->spec_async.load(std::memory_order_acquire) != 2) return;  // another thread of the caller was faster
  if (p->spec_thread.joinable()) p->spec_thread.join();
  gsdf_program* q = p->spec_shadow;
  p->spec_shadow = nullptr;
  // The whole of what the shadow built, in one move. That loses nothing of the adopter's: a handle adopts only while it is not yet
  // specialised (the test here), and no group is built on an unspecialised handle (spec_ensure: todo is 0), so p->spec holds nothing
  // but the seconds of builds that failed, which take() keeps.
  if (q && !p->spec.specialised()) p->spec.take(q->spec);
  delete q;
  p->spec_async.store(0, std::memory_order_release);
}

extern "C" int gsdf_hip_program_specialize_async(gsdf_program* p) {
  if (!p) return fail(GSDF_ERR_BAD_ARGUMENT, "null program");
  std::lock_guard<std::mutex> lk(p->spec_async_mu);
  if (p->spec.specialised() || p->spec_async.load() != 0) return GSDF_OK;  // specialised already, or a build is under way / waiting to be adopted
  if (int rc = spec_refused(p)) return rc;
  gsdf_program* q = new (std::nothrow) gsdf_program;
  if (!q) return fail(GSDF_ERR_CAPACITY, "out of memory");
  q->prog = p->prog; q->device = p->device; q->num_cu = p->num_cu;  // all a build reads (no streams, no device memory)
  p->spec_shadow = q;
  p->spec_async_err.clear();
  p->spec_async.store(1, std::memory_order_release);
  try {
    p->spec_thread = std::thread([p, q] {
      const int rc = gsdf_hip_program_specialize(q);
      if (rc != GSDF_OK) p->spec_async_err = gsdf_hip_last_error();  // (the error text is the building thread's)
      p->spec_async.store(rc == GSDF_OK ? 2 : 3, std::memory_order_release);
    });
  } catch (...) {
    p->spec_shadow = nullptr;
    delete q;
    p->spec_async.store(0);
    return fail(GSDF_ERR_CAPACITY, "cannot start the build thread");
  }
  return GSDF_OK;
}

/* 1: the handle runs specialised kernels now; 0: the build is still under way (wait = 0) or none was started; a negative status if
 * the build failed (the interpreter kernels stay in use; gsdf_hip_last_error has the compiler's words). wait != 0 blocks until the
 * build has finished. */
extern "C" int gsdf_hip_program_specialize_poll(gsdf_program* p, int wait) {
  if (!p) return fail(GSDF_ERR_BAD_ARGUMENT, "null program");
  if (wait) {
    std::unique_lock<std::mutex> lk(p->spec_async_mu);
    if (p->spec_async.load() == 1 && p->spec_thread.joinable()) p->spec_thread.join();
  }
  spec_adopt(p);
  if (p->spec_async.load(std::memory_order_acquire) == 3) {
    std::lock_guard<std::mutex> lk(p->spec_async_mu);
    if (p->spec_thread.joinable()) p->spec_thread.join();
    delete p->spec_shadow;
    p->spec_shadow = nullptr;
    p->spec_async.store(0);
    return fail(GSDF_ERR_HIP, "background specialisation failed: " + p->spec_async_err);
  }
  return p->spec.specialised() ? 1 : 0;
}

/* 1 if the handle runs specialised kernels; compile_seconds (optional) = what the build took */
extern "C" int gsdf_hip_program_is_specialized(const gsdf_program* p, double* compile_seconds) {
  if (compile_seconds) *compile_seconds = p ? p->spec.compile_s : 0.0;
  return p && p->spec.specialised() ? 1 : 0;
}

/* The kernels this handle launches, e.g. "eval=eval_kernel<3,4,4>:specialised leaf=leaf_eval_kernel<4,3>:specialised
 * prune=prune_kernel:specialised" (":interpreter" for the ahead-of-time kernels): what a profile of the handle shows. One cap: a
 * field is appended only while the whole text stays under 512 bytes, what the callers' buffers hold (the longest seen: 397 bytes,
 * npt-flange specialised with its distinct-rows and distinct-points kernels built, before the 27 bytes of " ray=" came behind them:
 * 424). Fields are appended in the order of their age, so the one a cap would drop first is the newest. */
extern "C" int gsdf_hip_program_kernels(const gsdf_program* p, char* dst, size_t dst_cap) {
  if (!p || !dst || dst_cap == 0) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  // the rules the launches go by: eval_dev's, the leaf phase of a mesh of three levels or more (gsdf_program::leaf_pick)
  const SpecKernels& k = p->spec;
  const bool is2d = p->prog.is2d;
  const int ek = p->batch_k();
  const bool se = k.f_eval && k.eval_k == ek;
  const SweepVariant ev = se ? SweepVariant{ek, k.eval_w} : p->sweep_variant(ek);
  const LeafPick leaf = p->leaf_pick(3);
  auto how = [](const void* f) { return std::string(f ? "specialised" : "interpreter"); };
  std::string s;
  auto add = [&](const std::string& field) { if (s.size() + field.size() < 512) s += field; };
  add("eval=" + ev.short_name("eval_kernel", is2d ? 2 : 3) + ":" + how(se ? k.f_eval : nullptr));
  if (!is2d) add(" leaf=" + leaf.v.short_name() + ":" + how(leaf.f) + " prune=prune_kernel:" + how(k.f_prune));
  // the evaluating kernels of share_corners = 1 and = 2, once they have been built
  if (k.f_leaf_dense) add(" leaf_dense=leaf_dense_kernel<" + std::to_string(k.dense_w) + ">:specialised");
  if (k.f_leaf_dz) add(" leaf_rows=" + p->leaf_pick(3, true).v.short_name() + ":specialised");
  if (is2d) {  // the picture kernels (a specialised handle builds its own at its first picture)
    std::string kinds;
    for (int i = 0; i < 4; i++) if (k.f_imgc[i]) kinds += std::to_string(i);
    add(" picture=image2_color_kernel<" + std::to_string(ek) + ",kind>:" + (kinds.empty() ? "interpreter" : "specialised/" + kinds));
  } else {  // the projection of mesh vertices (likewise at its first projection)
    add(" project=project_kernel:" + how(k.f_project));
  }
  // the sweeps that carry a K of their own, and what the LDS limits of the meshers count (gsdf_hip.h: Largest trees)
  if (is2d) add(" image=image2_kernel<" + std::to_string(ek) + ">:" + how(k.f_image));
  else add(" flat=" + p->sweep_variant(ek).short_name("flat_grid_kernel") + ":" + how(k.f_flat_grid) + " dc=" + gsdf_program::dc_origin_variant(ek).short_name("dc_origin_kernel") +
           ":" + how(k.f_dc_origin) + " interval=" + std::to_string(p->prog.lip_depth));
  if (k.specialised()) add(" compiler=" + k.compiler);
  // identity of the code that runs: a stored profile describes this handle's kernels only if it carries the same key
  add(" code=" + (k.specialised() ? k.key : gsdf_dev::spec_library_key()));
  // the lowering's division census (compile.h): with RN(1/d) / declined / polygons flagged / not flagged
  add(" recip=" + std::to_string(p->prog.n_recip) + "/" + std::to_string(p->prog.n_recip_declined) + "/" + std::to_string(p->prog.n_poly_recip) + "/" + std::to_string(p->prog.n_poly_plain));
  if (!is2d) add(" ray=ray_kernel:" + how(k.f_ray));  // rays and wall thickness (built at the first cast); the newest field, so the first to go
  if (s.size() + 1 > dst_cap) return fail(GSDF_ERR_SHORT_BUFFER, "short buffer");
  std::memcpy(dst, s.c_str(), s.size() + 1);
  return GSDF_OK;
}

// Host-only (no GPU): the generated evaluator source of a tree's specialised build, and a hiprtc compile of the
// specialised kernels for gfx950 that stops before loading them (proves the generated code builds).
extern "C" int gsdf_hip_specialize_source(const gsdf_tree* tree, char* dst, size_t dst_cap, size_t* len) {
  if (!tree) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  try {
    const std::string s = gsdf_dev::spec_source(gsdf_dev::compile(*tree));
    if (len) *len = s.size();
    if (dst) {
      if (dst_cap < s.size() + 1) return fail(GSDF_ERR_SHORT_BUFFER, "short buffer");
      std::memcpy(dst, s.c_str(), s.size() + 1);
    }
    return GSDF_OK;
  } catch (const std::exception& e) {
    return fail(GSDF_ERR_BAD_TREE, e.what());
  }
}
extern "C" int gsdf_hip_specialize_check(const gsdf_tree* tree, size_t* code_object_bytes) {
  if (!tree) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  try {
    const gsdf_dev::Program pr = gsdf_dev::compile(*tree);
    std::vector<char> co;
    std::vector<std::string> low;
    std::string log;
    const std::vector<std::string> names = pr.is2d ? std::vector<std::string>{"eval_kernel<2, 4, 4>"}
                                                   : std::vector<std::string>{"eval_kernel<3, 4, 4>", "prune_kernel", "prune_spec_kernel", "leaf_eval_kernel<4, 4, true, true, false, false>", "leaf_eval_kernel<4, 4, true, true, true, true>", "leaf_dense_kernel<4, true, true>", "flat_grid_kernel<4, 4>"};
    if (!gsdf_dev::spec_compile(pr, "gfx950", names, co, low, log)) return fail(GSDF_ERR_HIP, "specialised build failed:\n" + log);
    if (code_object_bytes) *code_object_bytes = co.size();
    return GSDF_OK;
  } catch (const std::exception& e) {
    return fail(GSDF_ERR_BAD_TREE, e.what());
  }
}
