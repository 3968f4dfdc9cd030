/*
 * gsdf_hip.h -- C ABI of libgsdfhip.so: the MI355X (gfx950) drop-in for the reference's GPU seam.
 *
 * What each entry point replaces in /root/reference (the cgo binding a maintainer would add is in
 * INTEGRATION.md):
 *   gsdf_hip_init              gleval.Init1x1GLFW                     gleval/gpu.go:21-32
 *   gsdf_hip_program_create    gleval.NewComputeGPUSDF3 / ...SDF2     gleval/gpu.go:35-55,105-130
 *                              (takes the flattened tree instead of GLSL text: glbuild.Programmer
 *                               .WriteComputeSDF3, gsdfaux/gsdfaux.go:122-126)
 *   gsdf_hip_program_bounds    (*SDF3Compute).Bounds                  gleval/gpu.go:75-77
 *   gsdf_hip_evaluations       (*SDF3Compute).Evaluations             gleval/gpu.go:80
 *   gsdf_hip_eval3 / _eval2    (*SDF3Compute).Evaluate / SDF2Compute  gleval/gpu.go:82-103,140-160
 *                              + computeEvaluate                      gleval/gpu_cgo.go:194-258
 *   gsdf_hip_eval3_dev         same, positions/distances already resident in HBM (no reference
 *                              equivalent: the GL path re-uploads every call, gpu_cgo.go:238-257)
 *   gsdf_hip_normals3          gleval.NormalsCentralDiff              gleval/gleval.go:53-108
 *   gsdf_hip_image2            glrender.ImageRendererSDF2.Render (default conversion)  glrender/image.go:46-118
 *   gsdf_hip_image2_color      ImageRendererSDF2.Render with gsdfaux's colour conversions (IQ, linear gradient, black and
 *                              white)                              gsdfaux/color.go, glrender/image.go:46-118
 *   gsdf_hip_picture_size,     RenderPNGFile's picture width and its default conversion
 *   gsdf_hip_color_iq / _gradient                                   gsdfaux/gsdfaux.go:264-296
 *   gsdf_hip_view_orbit        the camera of gsdfaux.UI's fragment shader (orbit about a target)  gsdfaux/ui.go:18,123,220,276-297
 *   gsdf_hip_render3           one gsdfaux.UI frame, headless: ray march + normal + two-light shading, uAA x uAA
 *                              supersampling                                                      gsdfaux/ui.go:247-355
 *   gsdf_hip_mesh_octree       glrender.NewOctreeRenderer + RenderAll glrender/octreerenderer.go:43-178,
 *                              (octree prune + marching cubes on device) glrender/marchcubes.go:14-98
 *   gsdf_hip_mesh_dualcontour  glrender.DualContourRenderer.Reset/RenderAll + DualContourLeastSquares
 *                                                                      glrender/dual_contour.go:26-219, dual_contour_vertexplacement.go:26-223
 *   gsdf_hip_mesh_read         (*Octree).ReadTriangles drain          glrender/octreerenderer.go:131-178
 *   gsdf_hip_mesh_stl          glrender.WriteBinarySTL                glrender/stl.go:15-62
 *
 * Conventions: plain pointers and sizes only; every function returns 0 on success or a negative
 * gsdf_status; gsdf_hip_last_error() gives the message for the calling thread. Buffers are borrowed
 * for the duration of the call only (Go pointer rules: nothing is retained). A handle is not
 * thread-safe (same as the reference's SDF3Compute, gpu.go:94-101); distinct handles are independent.
 */
#ifndef GSDF_HIP_H
#define GSDF_HIP_H
#include <stddef.h>
#include <stdint.h>

#include "gsdf_program.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef enum gsdf_status {
  GSDF_OK = 0,
  GSDF_ERR_EMPTY_BUFFERS = -1,   /* gleval.errEmptyBuffers (gleval/gleval.go:47) */
  GSDF_ERR_LENGTH_MISMATCH = -2, /* gleval.errMismatchBufferLength (gleval/gleval.go:48) */
  GSDF_ERR_BAD_ARGUMENT = -3,
  GSDF_ERR_BAD_TREE = -4,
  GSDF_ERR_HIP = -5,             /* HIP runtime error, message has hipGetErrorString */
  GSDF_ERR_NO_DEVICE = -6,
  GSDF_ERR_DIMENSION = -7,       /* 2D program given to a 3D entry point or vice versa */
  GSDF_ERR_RESOLUTION = -8,      /* "invalid renderer cube resolution" / "resolution not fine enough" */
  GSDF_ERR_SHORT_BUFFER = -9,    /* io.ErrShortBuffer */
  GSDF_ERR_CAPACITY = -10        /* device triangle buffer capacity exceeded */
} gsdf_status;

typedef struct gsdf_program gsdf_program; /* compiled tree, resident on one GPU */
typedef struct gsdf_mesh gsdf_mesh;       /* triangles produced on device, resident in HBM */

const char* gsdf_hip_last_error(void);

/* Select the HIP device for handles created by this thread afterwards. device < 0: keep current. */
int gsdf_hip_init(int device);

/* Largest trees. The evaluator keeps a tree's intermediate values in LDS: one KB per slot (gsdf_hip_program_info: lds_slots) and point
 * carried per lane, and a workgroup can have a CU's 160 KB at the most. What does not fit is refused on the host with
 * GSDF_ERR_BAD_TREE, before any kernel is launched, and the handle and the library stay usable:
 *   gsdf_hip_program_create                                   143 slots (one point per lane above 28 slots); a handle that exists
 *                                                             evaluates, renders (image2, image2_color, render3) and meshes flat;
 *   gsdf_hip_normals3, gsdf_hip_indexed_normals,
 *   gsdf_hip_indexed_project, _deviation,
 *   gsdf_hip_indexed_thickness                                80 slots (two points per lane);
 *   gsdf_hip_mesh_octree[_start]                              slots + interval stack <= 67 (the centre tests carry two points per lane
 *                                                             over both, beside 24 KB of cube stages; the interval stack is as deep as the
 *                                                             tree's position maps that stretch nest: twist, scale, ... -- "interval=" in
 *                                                             gsdf_hip_program_kernels);
 *   gsdf_hip_mesh_dualcontour[_indexed]                       52 slots (the edge pass carries three points per lane). Its block test
 *                                                             carries two over slots + interval stack: beyond 80 of them (an interval
 *                                                             stack deeper than 28) the test is left out and every block is
 *                                                             evaluated -- same triangles, more evaluations.
 * The library checks the macros below against its kernels' LDS arithmetic when it is compiled.
 * The interval stack takes a level per frame of brick masks (sixteen at the most) and per nested stretching map, so:
 * GSDF_HIP_MAX_SLOTS_ALL: up to here every entry point accepts a tree whose interval stack is no deeper than sixteen. */
#define GSDF_HIP_MAX_SLOTS_CREATE 143
#define GSDF_HIP_MAX_SLOTS_NORMALS 80
#define GSDF_HIP_MAX_COLS_OCTREE 67
#define GSDF_HIP_MAX_SLOTS_DC 52
#define GSDF_HIP_MAX_SLOTS_ALL 51
int gsdf_hip_program_create(const gsdf_tree* tree, gsdf_program** out);
void gsdf_hip_program_destroy(gsdf_program* p);
int gsdf_hip_program_bounds(const gsdf_program* p, float bb[6]);
int gsdf_hip_program_is2d(const gsdf_program* p);
/* Introspection for tests/benchmarks: lowered program size (32-bit words) and LDS slots per lane. */
int gsdf_hip_program_info(const gsdf_program* p, uint32_t* code_words, uint32_t* lds_slots);
uint64_t gsdf_hip_evaluations(const gsdf_program* p);
/* Test hook (needs a GPU): exhaustive check of the interpreter's exact division by a wave-uniform divisor d against
 * the IEEE division, over all 2^32 numerators. recip receives RN(1/d) (0: d not eligible, nothing to check). */
int gsdf_hip_selftest_div(float d, uint64_t* mismatches, uint64_t* fast_path_numerators, float* recip);
/* Test hook (needs a GPU): the interpreter's sqrt for hypot's [1,2] argument range against sqrtf, all floats in range; and the
 * per-tree kernels' sqrt without range handling (taken where a wave's arguments are all >= 2^-96) against sqrtf, every such float. */
int gsdf_hip_selftest_sqrt(uint64_t* mismatches);
/* Test hook (needs a GPU): the circular array's sector index from a float32 angle estimate (taken only where it provably
 * decides floor(atan2(y, x) / angle), cpu_evaluators.go:1047-1056) against that expression, over 2^32 points. */
int gsdf_hip_selftest_circ(float ncirc, uint64_t* mismatches, uint64_t* fast_path_points);
/* Test hook (needs a GPU): float32(math.Atan2(y, x)) by the short float64 route of the evaluator's screw / circular-array
 * instructions (forge/threads/threads.go:160, cpu_evaluators.go:1060), which is taken only where it provably rounds like the
 * reference's own operation sequence, against that sequence: 2^log2n pairs; mode 0 hashed pairs of every sign and magnitude,
 * 1 pairs searched towards float32 rounding boundaries, 2 lattice-shaped pairs. mismatches must come back 0. */
int gsdf_hip_selftest_atan2(int mode, int log2n, uint64_t* mismatches, uint64_t* fast_path_points);
/* Test hook (needs a GPU): float32(math.Cos(x)), float32(math.Sin(x)) of a twist's angle (cpu_evaluators.go:1269-1270) by the short
 * float64 route of the per-tree kernels, taken only where it provably rounds like the reference's own operation sequence, against that
 * sequence over EVERY float32 argument. mismatches must come back 0. */
int gsdf_hip_selftest_cossin(uint64_t* mismatches, uint64_t* fast_path_arguments);
/* Test hook (needs a GPU): the evaluator's own math routes -- the long ones the hooks above take as their yardstick -- applied to n
 * host values, one per lane, for a comparison with a reference on the host. fn: 0 hypot(x, y), 1 atan2(y = x[i], x = y[i]) by the
 * reference's float64 sequence, 2 sin, 3 cos, 4 acos, 5 cbrt, 6 / 7 Sincos' sine / cosine, 8 min, 9 max, 10 pow(x, 1/3), 11 round,
 * 12 floor, 13 / 14 the twist's cosine / sine, 15 atan2 as the evaluator calls it (short route where it decides), 16 sqrt,
 * 17 x[i] / divisor by the exact-reciprocal division where the divisor is eligible, 18 min(0, max(x, y)) + hypot(max(x, 0),
 * max(y, 0)) as the box-like primitives run it (max(x, y) + 0 where every wave of 64 consecutive values has x <= 0 or y <= 0 throughout,
 * else term by term), 19 the same term by term always, 20 / 21 likewise for three terms, the third being divisor. Each pair agrees
 * bit for bit. y may be null for one-operand functions. */
int gsdf_hip_selftest_math(int fn, const float* x, const float* y, float* out, uint64_t n, float divisor);
/* Test hook (needs a GPU): the CU count that a handle created now on `device` (< 0: the current one) would size its grids from: the
 * device's own, or GSDF_HIP_GRID_CUS (environment, read at every handle creation) where that is a number from 1 to the device's
 * count. With few CUs every grid-stride loop takes several trips at sizes a test can afford; results never depend on it.
 * real_cus (may be null) receives the device's own count. 0: no such device. */
int gsdf_hip_grid_cus(int device, int* real_cus);
/* Run-time specialisation (no reference counterpart; the reference's GPU path compiles GLSL per tree at
 * gleval/gpu.go:35-54, this is the same step for the HIP backend): builds, with hiprtc, eval / prune / leaf kernels in
 * which this program's instructions are laid out straight-line with literal parameters, and makes the handle launch
 * them. Same statements and compiler flags as the interpreter, so results stay bit-identical; costs a few seconds
 * once per handle. Without it (or if hiprtc is unavailable: GSDF_ERR_HIP) the handle runs the interpreter kernels.
 * Environment: GSDF_HIP_CACHE_DIR=<dir> keeps the built code objects on disk (key: generated source, device headers,
 * architecture, options, hiprtc version), so the next process that specialises the same tree reads a file instead. */
int gsdf_hip_program_specialize(gsdf_program* p);
int gsdf_hip_program_is_specialized(const gsdf_program* p, double* compile_seconds);
/* The same build on a thread of its own: returns at once, the handle keeps working through the interpreter kernels and switches to
 * the specialised ones at its first entry-point call after they are ready (bit-identical results either way). For the callers the
 * reference actually has -- one tree, one mesh, one file (examples/npt-flange/flange.go:61-98; gsdfaux.RenderShader3D,
 * gsdfaux/gsdfaux.go:93-171, compiles its shader and then renders once): the first mesh does not wait for a compiler.
 * _poll: 1 = specialised kernels in use, 0 = still building or never started (wait != 0: block until the build has finished),
 * negative status = the build failed (the interpreter kernels stay in use). Destroying the handle waits for a build under way. */
int gsdf_hip_program_specialize_async(gsdf_program* p);
int gsdf_hip_program_specialize_poll(gsdf_program* p, int wait);
/* Names of the kernels this handle launches, as a profiler shows them: "eval=eval_kernel<3,4,4>:specialised
 * leaf=leaf_eval_kernel<4,4>:specialised prune=prune_kernel:specialised compiler=hipcc code=<32 hex digits>" (":interpreter" =
 * the ahead-of-time kernels; compiler = what built the specialised ones: the installed hipcc out of process, or the process's
 * hiprtc; code = key of the code that runs: generated source + device headers + options + compiler identity for specialised
 * kernels, the library's device sources otherwise -- a stored profile describes this handle only if it carries the same key).
 * Further fields, in front of compiler= and code=: "flat=flat_grid_kernel<K,W>:..." and "dc=dc_origin_kernel<K,W>:..." (3-D: the flat
 * renderer's lattice pass, dual contouring's origin sweep), "image=image2_kernel<K>:..." (2-D) and "interval=<depth of the interval
 * stack>" (3-D: what the octree's limit counts beside the slots, see "Largest trees"). Last, "recip=a/b/c/d": what the lowering decided
 * about division -- a divisors that carry RN(1/d) for the exact-reciprocal form (|d| in [2^-30, 2^30]), b divisors it declined (the
 * device divides), c polygons whose every squared edge length is eligible, d polygons that are not (read-only, for tests that must
 * know which form a tree runs). Readers split at blanks and '=' and skip the fields they do not know. */
int gsdf_hip_program_kernels(const gsdf_program* p, char* dst, size_t dst_cap);
/* Host-only (run without a GPU): text of the generated evaluator, and a gfx950 hiprtc build of the specialised kernels
 * that stops before loading them. dst may be NULL to query the length. */
int gsdf_hip_specialize_source(const gsdf_tree* tree, char* dst, size_t dst_cap, size_t* len);
int gsdf_hip_specialize_check(const gsdf_tree* tree, size_t* code_object_bytes);
/* Host-only (runs without a GPU): lower a tree to the device instruction stream (gsdf_amd/csrc/dev_ops.h) for
 * inspection. code_out may be NULL to query the size. */
int gsdf_hip_lower(const gsdf_tree* tree, uint32_t* code_out, uint32_t code_cap, uint32_t* code_words, uint32_t* lds_slots);
/* Host-only test hook: the region outside which the lowering claims a positive lower bound of the subtree rooted at
 * `node` (what its skip gates test): *kind 0 = no claim, 1 = box {min xyz, max xyz}, 2 = z-axis cylinder {cx cy r z0 z1
 * rs rin} (rin > 0: an annulus -- the shape also keeps rin away from the axis); tests check the claim against the CPU
 * oracle (tests/test_gate_regions.py). */
int gsdf_hip_lower_region(const gsdf_tree* tree, uint32_t node, int* kind, float params[8]);

/* gleval.BlockCachedSDF3 (gleval/gleval.go:110-218): host-side lossy cache in front of a 3-D program, keyed by the
 * lattice cell int(mul*(p - bb.Min)), mul = 1/res per axis; misses go to the program in one batch. reset = Reset
 * (also clears the statistics), hits = CacheHits, evaluations = Evaluations (cached ones included). */
typedef struct gsdf_blockcache gsdf_blockcache;
int gsdf_hip_blockcache_create(gsdf_program* sdf, float resx, float resy, float resz, gsdf_blockcache** out);
int gsdf_hip_blockcache_reset(gsdf_blockcache* c, gsdf_program* sdf, float resx, float resy, float resz);
int gsdf_hip_blockcache_eval3(gsdf_blockcache* c, const void* pos, size_t pos_stride_bytes, size_t n_pos, float* dist, size_t n_dist);
uint64_t gsdf_hip_blockcache_hits(const gsdf_blockcache* c);
uint64_t gsdf_hip_blockcache_evaluations(const gsdf_blockcache* c);
void gsdf_hip_blockcache_destroy(gsdf_blockcache* c);

/* Host-buffer evaluation (drop-in for SDF3Compute.Evaluate). pos_stride_bytes is the distance between
 * consecutive positions: 12 for []ms3.Vec, 16 for std140 vec3 / ms3.Quat-aligned data; 8 for []ms2.Vec.
 * n_pos/n_dist are the two slice lengths (mismatch and zero are reported like the reference does). */
int gsdf_hip_eval3(gsdf_program* p, const void* pos, size_t pos_stride_bytes, size_t n_pos, float* dist, size_t n_dist);
int gsdf_hip_eval2(gsdf_program* p, const void* pos, size_t pos_stride_bytes, size_t n_pos, float* dist, size_t n_dist);
/* Thread safety of the host-buffer calls: gsdf_hip_eval3 / _eval2 may be called from several host threads on one program at
 * the same time (glrender.FlatRenderer evaluates from numParallel goroutines, flatrenderer.go:120-129): up to 4 calls are
 * in flight on their own streams and staging buffers, further callers wait for a slot. Everything else on a handle is one
 * caller at a time -- and while a background build is pending (gsdf_hip_program_specialize_async started, _poll not yet 1) not at
 * the same time as those concurrent Evaluate calls either: whichever entry point first finds the build finished swaps the
 * handle's kernels in (the Evaluate calls read theirs as one snapshot; a mesh being enqueued on another thread would not).
 * Pipelined form: submit returns at once with a ticket, wait blocks until that call's distances are in `dist` (batches of
 * up to 262144 points, any size in registered memory; at most 4 tickets outstanding per program). */
int gsdf_hip_eval3_submit(gsdf_program* p, const void* pos, size_t pos_stride_bytes, size_t n_pos, float* dist, size_t n_dist, int* ticket);
int gsdf_hip_eval_wait(gsdf_program* p, int ticket);
/* Caller buffers the GPU reaches directly. A host-buffer call whose positions AND distances lie inside memory from
 * gsdf_hip_host_alloc (pinned, device-mapped; C memory, so a Go caller may wrap it in a slice and keep it) or registered
 * with gsdf_hip_host_register (pins and maps memory the caller allocated and keeps alive, e.g. the renderer's long-lived
 * posbuf/distbuf) makes no staging copy: the kernel reads and writes the caller's memory across PCIe.
 * gsdf_hip_host_release frees / unregisters. */
void* gsdf_hip_host_alloc(size_t bytes);
int gsdf_hip_host_register(void* ptr, size_t bytes);
int gsdf_hip_host_release(void* ptr);
/* Device-resident evaluation: d_pos/d_dist are device pointers on the program's GPU; stream is a
 * hipStream_t (NULL = the program's own stream, a non-blocking one). Asynchronous either way: the kernel is enqueued and the
 * call returns; synchronise the stream you passed, or the device (hipDeviceSynchronize) when it was the program's own. */
int gsdf_hip_eval3_dev(gsdf_program* p, const void* d_pos, size_t pos_stride_bytes, float* d_dist, size_t n, void* stream);
int gsdf_hip_eval2_dev(gsdf_program* p, const void* d_pos, size_t pos_stride_bytes, float* d_dist, size_t n, void* stream);
/* Central-difference normals (not normalised), host buffers, 12-byte xyz in and out. */
int gsdf_hip_normals3(gsdf_program* p, const float* pos, float* normals, size_t n, float step);

/* ImageRendererSDF2.Render of a 2D program over its Bounds(): dist_out (w*h floats, row 0 = top) and/or rgba_out
 * (w*h*4 bytes: black inside, white outside, red for NaN/Inf -- the renderer's default conversion). */
int gsdf_hip_image2(gsdf_program* p, int w, int h, float* dist_out, uint8_t* rgba_out);

/* ---- a 2-D part's picture with the reference's colour conversions (gsdfaux.RenderPNGFile, gsdfaux/gsdfaux.go:264-296;
 *      gsdfaux/color.go) ---------------------------------------------------------------------------------------------------------
 *
 * gsdf_hip_image2_color samples the pixel lattice of gsdf_hip_image2 (the same statements, so the same distances, bit for bit)
 * and converts each distance d to RGBA8 by the conversion `conv`. The conversions are exact float32 arithmetic, which the device
 * kernel (gsdf_amd/csrc/kernels_image.h) and the CPU twin of the tests (tests/colorref.py) follow to the bit: every step ONE IEEE
 * operation rounded to nearest, never contracted, division correctly rounded, sums left to right as color.go writes them; the
 * constants are the float32 values nearest to the exact numbers Go's untyped constants denote (1.0/6 -> float32(1/6), not the
 * float32 of the float64 1/6). Helpers (u8 and friends are stated at the end):
 *   Clamp(v, lo, hi) = v < lo ? lo : (v > hi ? hi : v)  (a NaN stays NaN)        Interp(x, y, a) = x + a * (y - x)
 *   SmoothStep(e0, e1, x) = (t * t) * (3 - 2 * t), t = Clamp((x - e0) / (e1 - e0), 0, 1)
 *
 * GSDF_COLOR_DEFAULT    gsdf_hip_image2's bytes: (255,0,0,255) for NaN / +-Inf, white for d > 0, black otherwise (image.go:51-61).
 * GSDF_COLOR_IQ         ColorConversionInigoQuilez(length) (color.go:21-46). NaN -> (255,0,0,255). Otherwise inv = 1 / length;
 *                       d = d * inv; c = d > 0 ? (0.9, 0.6, 0.3) : (0.65, 0.85, 1.0); a = |d|; c *= 1 - Exp(-6 * a);
 *                       c *= 0.8 + 0.2 * Cos(150 * d); mx = 1 - SmoothStep(0, 0.01, a); c = Interp(c, 1, mx) per channel;
 *                       (u8(c.x * 255), u8(c.y * 255), u8(c.z * 255), 255). An infinite distance gives Cos(Inf) = NaN, hence
 *                       (0, 0, 0, 255).
 * GSDF_COLOR_GRADIENT   ColorConversionLinearGradient(length, c0, c1) (color.go:50-71, 104-200) for any pair but black -> white.
 *                       blend = d / length + 0.5; blend <= 0 -> c0 as stored; blend >= 1 -> c1 as stored. Otherwise (a NaN
 *                       included) (h, s, v) = hsvToRGB's inverse rgbToHSV of each end colour's r / 255, g / 255, b / 255
 *                       (colorToHSV; the >> 8 of the 16-bit values gives the stored bytes back), interpHSV (h0 += 1 if h1 - h0 >
 *                       0.5, else h1 += 1 if h1 - h0 < -0.5; then Interp of h, s, v by blend), hsvToRGB (c = s * v, x = c * (1 -
 *                       |Mod(h * 6, 2) - 1|), m = v - c; the six cases h in [0, 1/6], (1/6, 2/6], ... (5/6, 1] give (c,x,0),
 *                       (x,c,0), (0,c,x), (0,x,c), (x,0,c), (c,0,x); an h outside [0, 1], NaN included, gives (0,0,0); then + m
 *                       per channel), rgbToC (u32(Clamp(ch, 0, 1) * 255) per channel); alpha 255. rgbToHSV(r, g, b): xmax / xmin
 *                       of the three, c = xmax - xmin, v = xmax; h = 0 if c == 0, else (g - b) / (c * 6) if v == r, else 1/3 +
 *                       (b - r) / (c * 6) if v == g, else 2/3 + (r - g) / (c * 6); h += 1 if h < 0; s = xmax > 0 ? c / xmax : 0.
 *                       Mod(x, 2) is the exact remainder with the sign of x (math32.Mod).
 * GSDF_COLOR_BW_SMOOTH  ColorConversionLinearGradient(length, color.Black, color.White) (color.go:73-99). length == 0: d < 0 ->
 *                       black, anything else (NaN included) -> white. Otherwise blend = d / length + 0.5; blend <= 0 -> black;
 *                       blend >= 1 -> white; else y = u8(Clamp(blend, 0, 1) * 255) -> (y, y, y, 255) (a NaN gives y = 0).
 *
 * Pinned by this contract, not by the reference (the reference leaves them to the platform or to code outside it):
 *   Exp(x)  = float32(exp64(float64(x))), exp64 Go's portable math.Exp (exp.go: FreeBSD e_exp.c reduction k = int(Log2e x -+ 0.5),
 *             hi = x - k Ln2Hi, lo = k Ln2Lo, then expmulti and an exact Ldexp) with its special cases (NaN, +-Inf, x > 709.78...
 *             -> +Inf, x < -745.13... -> 0, |x| < 2^-28 -> 1 + x). math32.Exp has amd64 assembly of its own.
 *   Cos(x)  = float32(cos64(float64(x))), cos64 Go's math.Cos with Cody-Waite reduction (cos.go, as oracle/orc_math.h states it)
 *             at every finite argument: Go switches to Payne-Hanek at |x| >= 2^29, which this contract does not follow (at such
 *             arguments the results differ from Go's; IQ reaches them only at distances above 3.5e6 characteristic lengths).
 *             Where x (4/pi) >= 2^64 the integer part is taken as 0, as amd64's float64 -> uint64 conversion gives it.
 *   u8(v), u32(v): Go's float -> integer conversion of a value outside the target's range is implementation-specific. Stated
 *             here as amd64's truncating conversion to int64, low bits kept: NaN and |v| >= 2^63 give 0, other values
 *             trunc(v) mod 256 (u8) / mod 2^32 (u32). (Not checked against a Go toolchain.)
 *   Clamp, SmoothStep, Interp and the bounds' Diagonal (below) restate helpers of soypat/geometry (ms1, ms3, ms2), a module
 *   this project does not carry. */
enum {
  GSDF_COLOR_DEFAULT = 0,
  GSDF_COLOR_IQ = 1,
  GSDF_COLOR_GRADIENT = 2,
  GSDF_COLOR_BW_SMOOTH = 3
};
typedef struct gsdf_color2 {
  int32_t kind;        /* GSDF_COLOR_* */
  float length;        /* IQ: characteristic distance (finite, > 0); GRADIENT / BW_SMOOTH: gradient length (finite, >= 0) */
  uint8_t c0[4];       /* GRADIENT end colours, 8-bit RGBA as image.RGBA stores them (alpha-premultiplied) */
  uint8_t c1[4];
  int32_t reserved[4]; /* 0 */
} gsdf_color2;
GSDF_ABI_ASSERT(sizeof(gsdf_color2) == 32, "gsdf_color2 is 32 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_color2, kind) == 0 && offsetof(gsdf_color2, length) == 4 && offsetof(gsdf_color2, c0) == 8, "gsdf_color2 head");
GSDF_ABI_ASSERT(offsetof(gsdf_color2, c1) == 12 && offsetof(gsdf_color2, reserved) == 16, "gsdf_color2 tail");

/* RenderPNGFile's picture size (gsdfaux.go:271-274; host only, needs no device): bb = gsdf_hip_program_bounds of the part;
 * sz = (bb[3] - bb[0], bb[4] - bb[1]) in float32, pixPerUnit = float64(pic_height) / float64(sz.y), *w = int(pixPerUnit *
 * float64(sz.x)) (truncated). GSDF_ERR_BAD_ARGUMENT for non-finite bounds, sz.y <= 0, or pic_height or *w outside 1 .. 16384. */
int gsdf_hip_picture_size(const float bb[6], int pic_height, int* w);
/* ColorConversionInigoQuilez (host only): char_dist > 0 is used as given; char_dist <= 0 selects RenderPNGFile's default,
 * Diagonal() / 3 of the x, y extents (math32.Hypot in float32, then one float32 division). GSDF_ERR_BAD_ARGUMENT for non-finite
 * input or a default that comes out 0. */
int gsdf_hip_color_iq(const float bb[6], float char_dist, gsdf_color2* out);
/* ColorConversionLinearGradient(length, c0, c1) (host only): BW_SMOOTH when c0 is (0,0,0,255) and c1 (255,255,255,255), GRADIENT
 * otherwise. A byte test, not Go's: `c0 == color.Black` is an interface comparison that holds for color.Black / color.White only
 * (dynamic type Gray16), so Go sends color.RGBA{0,0,0,255} -> {255,255,255,255} down the HSV path. The two paths give the same
 * bytes for length > 0; at length 0 they differ where d == 0 or d is NaN (BW_SMOOTH: white; the HSV path: black). A caller that
 * holds Go values decides the kind by Go's own comparison (integration/go/gsdfaux/png_hip.go). GSDF_ERR_BAD_ARGUMENT for a
 * non-finite or negative length. */
int gsdf_hip_color_gradient(float length, const uint8_t c0[4], const uint8_t c1[4], gsdf_color2* out);
/* The picture of a 2-D program: rgba_out w*h*4 bytes converted by `conv`, dist_out w*h floats (gsdf_hip_image2's), row 0 = top;
 * either may be NULL. Blocking; gsdf_hip_evaluations grows by w*h. GSDF_ERR_DIMENSION for a 3-D program; GSDF_ERR_BAD_ARGUMENT
 * for a NULL or unknown conversion, a length out of its kind's range, non-zero reserved words, or w or h outside 1 .. 16384. */
int gsdf_hip_image2_color(gsdf_program* p, const gsdf_color2* conv, int w, int h, uint8_t* rgba_out, float* dist_out);

/* ---- the UI's ray-marched view of a 3-D part (gsdfaux.UI, gsdfaux/ui.go:247-355), headless ------------------------------------
 *
 * The GLSL leaves rounding to the driver; here the frame is exact float32 arithmetic, which the device kernel
 * (gsdf_amd/csrc/kernels_view.h) and the CPU twin of the tests (tests/viewref.py) follow to the bit. Every operation is ONE
 * IEEE float32 operation, rounded to nearest, never contracted; sqrt and division correctly rounded; sums left to right as the
 * shader writes them. normalize(v) = v / sqrt((x*x + y*y) + z*z), one division per component; clamp(x, a, b) = fmin(fmax(x, a), b),
 * so a NaN clamps to a.
 *
 * Pixels and samples. Output row r is GL row j = h - 1 - r (row 0 is the top, as gsdf_hip_image2); fragCoord = (i + 0.5, j + 0.5),
 * exact. For m, n in 0 .. aa-1 (m outer): o = (float(m), float(n)) / float(aa) - 0.5; p = (2 (fragCoord + o) - (w, h)) / float(h);
 * rd = normalize((p.x uu + p.y vv) + 1.5 ww).
 * Marching. tol = 1e-4f, tmax = 1.3f * char_dist, t = 0; for i < max_steps: pos = ro + t rd, d = sdf(pos); if d < tol || t > tmax
 * { hit = d < tol; stop } else t += d. A NaN distance is never a hit and marching runs on to max_steps; a field that is not
 * 1-Lipschitz overshoots as the UI's does (a view, not a guarantee).
 * Normal and colour (hit samples only). k = 0.5773f * 1e-4f; d0..d3 = sdf(pos + (k,-k,-k)), sdf(pos + (-k,-k,k)), sdf(pos + (-k,k,-k)),
 * sdf(pos + (k,k,k)); with e = (0.5773, -0.5773): nor = normalize(((e.xyy d0 + e.yyx d1) + e.yxy d2) + e.xxx d3);
 * dif = clamp((nor.x 0.57703 + nor.y 0.57703) + nor.z 0.57703, 0, 1); amb = 0.5 + 0.5 nor.y;
 * col = sqrt((0.2, 0.3, 0.4) amb + (0.8, 0.7, 0.5) dif); tot += col. After the samples tot /= float(aa * aa).
 * Outputs per pixel (each optional): RGBA8 = (uint8)(clamp(tot, 0, 1) * 255 + 0.5f), alpha 255; depth = the smallest t among the
 * pixel's hitting samples, +Inf if none hit; evals = SDF evaluations the pixel cost (march steps + 4 per hit). The program's
 * gsdf_hip_evaluations grows by the sum of evals. */
typedef struct gsdf_view {
  float ro[3];        /* camera position */
  float uu[3];        /* right */
  float vv[3];        /* up */
  float ww[3];        /* forward (unit) */
  float char_dist;    /* characteristic distance: marching gives up beyond t = 1.3 char_dist */
  int32_t aa;         /* aa x aa samples per pixel, 1 .. 8 (the UI: 1 while the mouse moves, 3 at rest) */
  int32_t max_steps;  /* march steps per sample, 0 .. 4096 (the UI: 256) */
  int32_t reserved;   /* 0 */
} gsdf_view;
GSDF_ABI_ASSERT(sizeof(gsdf_view) == 64, "gsdf_view is 64 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_view, ro) == 0 && offsetof(gsdf_view, uu) == 12 && offsetof(gsdf_view, vv) == 24 && offsetof(gsdf_view, ww) == 36, "gsdf_view basis");
GSDF_ABI_ASSERT(offsetof(gsdf_view, char_dist) == 48 && offsetof(gsdf_view, aa) == 52 && offsetof(gsdf_view, max_steps) == 56, "gsdf_view tail");

/* The UI's orbit camera (host only, needs no device): bb = gsdf_hip_program_bounds of the part; yaw, pitch in radians (pitch is
 * clamped to +-(pi/2 - 0.01)); cam_dist <= 0: the UI's default camDist = diag, the bounds' Diagonal() (Norm of the size vector by
 * nested hypot); char_dist = camDist + diag; target NULL = the origin, as ui.go. dir = (cos p sin y, sin p, cos p cos y) (trig in
 * float64, rounded once), ro = ta - dir camDist, ww = normalize(ta - ro), uu = normalize(cross(ww, (0,1,0))), vv = cross(uu, ww).
 * Sets aa = 1, max_steps = 256. GSDF_ERR_BAD_ARGUMENT for non-finite inputs or an empty camera distance. */
int gsdf_hip_view_orbit(const float bb[6], float yaw, float pitch, float cam_dist, const float target[3], gsdf_view* view);
/* One frame of a 3-D program through `view` (see gsdf_view): host outputs, each may be NULL -- rgba_out w*h*4 bytes, depth_out
 * w*h floats, evals_out w*h uint32, row 0 = top. Blocking, like gsdf_hip_image2. GSDF_ERR_DIMENSION for a 2-D program;
 * GSDF_ERR_BAD_ARGUMENT for w or h outside 1 .. 16384, aa outside 1 .. 8, max_steps outside 0 .. 4096 or a non-finite camera. */
int gsdf_hip_render3(gsdf_program* p, const gsdf_view* view, int w, int h, uint8_t* rgba_out, float* depth_out, uint32_t* evals_out);

/* gsdf_mesh_opts.prune flag: apply the reference's centre test verbatim, |d(centre)| >= size * sqrt3/2
 * (octreerenderer.go:270-273), at the tested levels, as if the field were a true distance field. */
#define GSDF_PRUNE_ASSUME_SDF (1 << 30)
typedef struct gsdf_mesh_opts {
  int prune;          /* which octree levels are centre-tested: 1 = every Level >= 3 (default), 0 = none (visit all leaves), any
                         other value = bit mask (bit L = cubes of Level L, L >= 3). The reference tests the capacity-limited
                         frontier of its DecomposeBFS buffer only (octreerenderer.go:94-105,140): a handful of upper levels.
                         The test drops a cube when the field cannot vanish inside it: the bounds of the field over the cube's
                         bounding ball, obtained by interval evaluation of the tree at the centre, exclude 0. For a true
                         distance field those bounds are d -+ size * sqrt3/2, i.e. the reference's predicate
                         |d| >= size * sqrt3/2 (:270-273); for fields that grow faster than distance (twist, screw, non-rigid
                         transform) or jump (a screw with an asymmetric thread form, across the seams of its sawtooth) they
                         are wider, so that no cube holding surface is dropped at any level: examples/fibonacci-showerhead
                         at resdiv 350 gives the reference's 309,872 triangles (README.md:152,166), where the reference's
                         predicate applied to every Level >= 3 cube gives 309,849. Or'ing GSDF_PRUNE_ASSUME_SDF in selects
                         that predicate (a few percent fewer evaluations; exact only for 1-Lipschitz fields). Sector and cell
                         seams of (circular) arrays are taken as continuous, as those nodes' own Bounds() assume. */
  int shard_rank;     /* multi-GPU: this rank ... */
  int shard_count;    /* ... of this many (1 = whole model). Bricks of 16^3 leaves go to rank gsdf_hip_brick_owner(x, y, z, count). */
  uint64_t max_tris;  /* device triangle buffer capacity; 0 = size automatically */
  void* stream;       /* hipStream_t to run on; NULL = the program's stream */
  int share_corners;  /* 0 (default): every leaf evaluates its own 8 corners like the reference (8 evals/leaf);
                         1: each bitwise-distinct lattice point of a 4x4x4-leaf brick is evaluated once (identical
                         triangles, 1.2-2.2x fewer evaluations; leaf_dense_kernel in the default two-kernel leaf phase -- it
                         gives up the column sharing of the default, so it pays where the field costs more per point than per
                         (x, y) column: threads, knurls, transformed parts);
                         2: the bitwise-distinct z rows of a brick once each (a brick's eight rows of corners are five to eight
                         distinct planes: row 2k-1 = (O + res (i-1)) + res and row 2k = O + res i are the same float on most planes)
                         -- the default's kernels, a quarter fewer evaluations, identical distances, records and triangles.
                         stats.evals then counts the evaluations performed, not the reference's 8 per leaf: for 2, distinct rows
                         x 64 lanes (a second pass rounds the rows it executes up to its width: lane slots that repeat a row
                         are not counted; 1 counts every lane slot of its passes);
                         3: 1 or 2, chosen by how much of the tree's work depends on x and y alone (threads, knurls, transformed
                         parts: 1; mostly axisymmetric parts: 2). */
  int host_output;    /* 1: the triangle buffer is pinned, device-mapped HOST memory and the mesher writes it across PCIe
                         while it runs (gsdf_hip_mesh_host_tris then returns that buffer: mesh + transfer 4.x ms instead
                         of 1.7 + 4.4 ms at npt-flange resdiv 1600). For results that are consumed on the host only:
                         device-side consumers (gsdf_hip_mesh_stl, RCCL gathers) would read back over PCIe. */
  int payload;        /* what the mesh holds when the call returns: GSDF_PAYLOAD_TRIANGLES (0, default), or GSDF_PAYLOAD_RECORDS:
                         the 40-byte records of the leaves the surface cuts (8 corner distances, leaf coordinates, marching-cubes
                         case), packed, and no triangles yet -- the form a rank hands to gsdf_hip_mesh_gatherv_start, which then
                         moves 20 bytes per triangle instead of 36 and runs marching cubes on the receiving ranks, over everybody's
                         records. gsdf_hip_mesh_march turns such a mesh into triangles where it is. Same triangles either way. */
  int reserved;       /* 0 */
} gsdf_mesh_opts;
#define GSDF_PAYLOAD_TRIANGLES 0
#define GSDF_PAYLOAD_RECORDS 1

typedef struct gsdf_mesh_stats {
  uint64_t n_tris;
  uint64_t evals;          /* SDF evaluations performed on device for this mesh */
  uint64_t pruned_leaves;  /* leaf cubes skipped by pruning (Octree.TotalPruned) */
  uint64_t leaf_cubes;     /* leaf cubes visited */
  uint64_t active_leaves;  /* leaf cubes that passed the |d(corner0)| <= 2*sqrt3*res test */
  int levels;              /* octree levels (makeICube) */
  float origin[3];         /* lattice origin (scaled bounds min) */
  float res;
  double ms_total;         /* device time for the whole mesh, HIP events */
  double ms_prune;         /* pruning levels */
  double ms_leaf;          /* leaf phase */
  double ms_march;         /* dominant kernel alone, HIP events: leaf_eval_kernel (the 8 corner evaluations of every leaf) */
  uint64_t evals_prune;    /* evaluations done by the pruning levels (cube centres) */
  uint64_t evals_leaf;     /* evaluations done by the leaf phase (leaf corners) */
  double ms_emit;          /* march_records_kernel: marching cubes over the cut-leaf records */
  uint64_t cut_leaves;     /* leaves the surface cuts = 40-byte records handed from leaf_eval_kernel to march_records_kernel */
} gsdf_mesh_stats;

GSDF_ABI_ASSERT(sizeof(gsdf_mesh_opts) == 48, "gsdf_mesh_opts is 48 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_mesh_opts, prune) == 0 && offsetof(gsdf_mesh_opts, shard_rank) == 4 && offsetof(gsdf_mesh_opts, shard_count) == 8, "gsdf_mesh_opts head");
GSDF_ABI_ASSERT(offsetof(gsdf_mesh_opts, max_tris) == 16 && offsetof(gsdf_mesh_opts, stream) == 24, "gsdf_mesh_opts middle");
GSDF_ABI_ASSERT(offsetof(gsdf_mesh_opts, share_corners) == 32 && offsetof(gsdf_mesh_opts, host_output) == 36 && offsetof(gsdf_mesh_opts, payload) == 40, "gsdf_mesh_opts tail");
GSDF_ABI_ASSERT(sizeof(gsdf_mesh_stats) == 128, "gsdf_mesh_stats is 128 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_mesh_stats, n_tris) == 0 && offsetof(gsdf_mesh_stats, evals) == 8 && offsetof(gsdf_mesh_stats, pruned_leaves) == 16, "gsdf_mesh_stats counters");
GSDF_ABI_ASSERT(offsetof(gsdf_mesh_stats, leaf_cubes) == 24 && offsetof(gsdf_mesh_stats, active_leaves) == 32 && offsetof(gsdf_mesh_stats, levels) == 40, "gsdf_mesh_stats counters 2");
GSDF_ABI_ASSERT(offsetof(gsdf_mesh_stats, origin) == 44 && offsetof(gsdf_mesh_stats, res) == 56 && offsetof(gsdf_mesh_stats, ms_total) == 64, "gsdf_mesh_stats lattice");
GSDF_ABI_ASSERT(offsetof(gsdf_mesh_stats, ms_prune) == 72 && offsetof(gsdf_mesh_stats, ms_leaf) == 80 && offsetof(gsdf_mesh_stats, ms_march) == 88, "gsdf_mesh_stats times");
GSDF_ABI_ASSERT(offsetof(gsdf_mesh_stats, evals_prune) == 96 && offsetof(gsdf_mesh_stats, evals_leaf) == 104 && offsetof(gsdf_mesh_stats, ms_emit) == 112 && offsetof(gsdf_mesh_stats, cut_leaves) == 120, "gsdf_mesh_stats tail");
GSDF_ABI_ASSERT(GSDF_ERR_EMPTY_BUFFERS == -1 && GSDF_ERR_LENGTH_MISMATCH == -2 && GSDF_ERR_SHORT_BUFFER == -9 && GSDF_ERR_CAPACITY == -10, "status codes are part of the ABI");

int gsdf_hip_mesh_octree(gsdf_program* p, float res, const gsdf_mesh_opts* opts, gsdf_mesh** out);
/* The same in two halves, for a caller with several meshes to make (a part at several resolutions, a batch of parts on one
 * program): _start enqueues the whole chain of kernels and returns; _wait blocks until that mesh is complete. Up to three meshes
 * of a program may be in flight, each with a workspace and a stream of its own (opts.stream, if given, takes them all): the ~30 us a
 * blocking call spends between a mesh's last kernel and the next mesh's first (completion wake-up, the caller's bookkeeping,
 * launch latency) pass under a busy GPU, and the latency-bound top and tail of one mesh (centre tests, marching cubes over the
 * records) run beside the others' evaluating kernel: 0.34 ms per mesh with three in flight, 0.37 with two, 0.45 one at a time
 * (npt-flange resdiv 1600).
 * gsdf_hip_mesh_octree is _start followed by _wait. No other mesher call on the program while a job is in flight. */
typedef struct gsdf_mesh_job gsdf_mesh_job;
int gsdf_hip_mesh_octree_start(gsdf_program* p, float res, const gsdf_mesh_opts* opts, gsdf_mesh_job** job);
int gsdf_hip_mesh_octree_wait(gsdf_mesh_job* job, gsdf_mesh** out);
/* Dual contouring (least-squares vertex placement; chiseled = DualContourLeastSquares.Chiseled). The result is a
 * gsdf_mesh like the octree mesher's (stats: leaf_cubes = kept cubes, active_leaves = active edges; evals = the evaluations
 * performed -- fewer than the reference's: lattice blocks an interval evaluation proves empty are not swept, and a kept cube's own
 * origin is evaluated once, by the sweep, not again with its three edge ends). Multi-GPU: rank
 * shard_rank of shard_count emits the quads of its z-slab of the lattice (one-cube halo recomputed, nothing exchanged). */
int gsdf_hip_mesh_dualcontour(gsdf_program* p, float res, int chiseled, int shard_rank, int shard_count, void* stream,
                              gsdf_mesh** out);
/* glrender.FlatRenderer (glrender/flatrenderer.go:36-256; the renderer gsdfaux.RenderShader3D picks for CPU runs,
 * gsdfaux/gsdfaux.go:160-168): the SDF on every corner of the ceil(size/res)+1 lattice of the 1.01-scaled bounds into a
 * device-resident grid, then marching cubes of every cube whose first corner passes |d| <= 2*sqrt3*res. Same triangle
 * set as the reference's ReadTriangles loop (order differs). Stats: evals = lattice corners (FlatRenderer.Evaluations),
 * leaf_cubes = cubes, active_leaves = cubes passing the first-corner test, ms_leaf = lattice pass, ms_march = marching
 * pass, levels = 0. Multi-GPU: rank shard_rank of shard_count takes a z-slab of cubes (the reference's goroutine split,
 * :120-122), nothing exchanged. */
int gsdf_hip_mesh_flat(gsdf_program* p, float res, int shard_rank, int shard_count, void* stream, gsdf_mesh** out);
/* minecraftRender (glrender/dual_contour.go:297-403; unexported there, exercised by glrender_test.go:55-81): every level-1 cube of the
 * top cube over Bounds() has its origin and its +x, +y, +z edge ends evaluated; an edge whose ends differ in sign contributes the
 * square face across it, two triangles wound by which end is inside. Triangles in no particular order (the reference's is the order of
 * its breadth-first decomposition); stats: n_tris, evals = 4 per cube, levels. At most 9 levels (every cube is evaluated). */
int gsdf_hip_mesh_minecraft(gsdf_program* p, float res, void* stream, gsdf_mesh** out);
int gsdf_hip_mesh_stats_get(const gsdf_mesh* m, gsdf_mesh_stats* st);
/* Device time of the mesher's stages, where it records them (dual contouring: dc_origin, dc_edges, dc_normals, dc_place, dc_quads;
 * HIP events between the stages): *n = number of stages, ms / names (optional, cap entries) = milliseconds and kernel names. */
int gsdf_hip_mesh_stage_ms(const gsdf_mesh* m, double* ms, const char** names, int cap, int* n);
/* What the mesh holds: GSDF_PAYLOAD_TRIANGLES or GSDF_PAYLOAD_RECORDS (gsdf_mesh_opts.payload); *n_records / *payload_bytes
 * (optional) = its cut-leaf records and the size of their packed form (0 for a mesh of triangles). */
int gsdf_hip_mesh_payload(const gsdf_mesh* m, uint64_t* n_records, uint64_t* payload_bytes);
/* Host copy of a records mesh's cut-leaf records, in the order marching cubes takes them: 10 words each -- the 8 corner distances
 * (float32 bits, Box.Vertices order), lx | ly << 16, lz | case << 16 (the leaf's integer coordinates and its marching-cubes case).
 * Works while the mesh holds records, and after gsdf_hip_mesh_march on a mesh gsdf_hip_mesh_weld accepts. *n_records optional;
 * dst NULL to query it. */
int gsdf_hip_mesh_read_records(const gsdf_mesh* m, uint32_t* dst, uint64_t dst_records, uint64_t* n_records);
/* Marching cubes over a mesh's packed records, in place: afterwards it holds triangles (stats.n_tris was known before) and
 * every accessor below works. No-op on a mesh of triangles. glrender/marchcubes.go:14-98. */
int gsdf_hip_mesh_march(gsdf_mesh* m);
/* Copy triangles [first, first+count) to host memory: 9 floats (36 B) each = ms3.Triangle. */
int gsdf_hip_mesh_read(const gsdf_mesh* m, uint64_t first, uint64_t count, float* dst);
/* Device pointer to the triangle array (for RCCL gathers / further device work). */
const float* gsdf_hip_mesh_dev_tris(const gsdf_mesh* m);
/* Binary STL (84 + 50*n bytes) built on device into dst (host). dst_cap must be >= that size. A zero-area triangle's normal is
 * NaN in all three components (Inf * 0, as glrender/stl.go computes it), with unspecified sign and payload: the reference's own
 * differ between amd64 and arm64. Vertex bytes and the attribute word are the reference's for every triangle. */
int gsdf_hip_mesh_stl(const gsdf_mesh* m, uint8_t* dst, size_t dst_cap);
/* Zero-copy result views (no reference counterpart: the reference drains a renderer through ReadTriangles into a
 * 4096-triangle buffer and appends, glrender/glrender.go:20-36, and WriteBinarySTL issues one Write per triangle,
 * glrender/stl.go:40-58). The whole result is moved once, by DMA, into pinned host memory owned by the mesh: *tris is
 * n_tris x 9 floats = []ms3.Triangle, *stl the complete binary STL file (84 + 50 n bytes, records built on device).
 * Valid until gsdf_hip_mesh_destroy; repeated calls return the same memory. */
int gsdf_hip_mesh_host_tris(gsdf_mesh* m, const float** tris);
int gsdf_hip_mesh_host_stl(gsdf_mesh* m, const uint8_t** stl, size_t* len);
/* Releases the mesh. Its device buffers go to a per-process pool that the next meshes (and gathers) draw from -- up to 16 idle
 * buffers are kept (environment: GSDF_HIP_POOL_MAX), beyond that the smallest is freed. */
void gsdf_hip_mesh_destroy(gsdf_mesh* m);

/* ---- indexed meshes: the marching-cubes vertices welded on device (no reference counterpart: the reference's mesh is a triangle
 *      list, SURVEY.md "no vertex welding") ---------------------------------------------------------------------------------------
 *
 * The two to four copies of a vertex that neighbouring cubes emit differ in their last bits (a leaf's corner is (O + res (i-1)) + res
 * seen from one leaf and O + res i from the next; half the marching-cubes edge pairs run against their axis), so they cannot be
 * merged by comparing floats. The cut-leaf records carry the leaves' integer coordinates: vertices are welded by the LATTICE EDGE
 * (or lattice point) they sit on, which is exact.
 *
 * Soup slot. Slot s = 3 t + c is corner c of triangle t, in the order gsdf_hip_mesh_march produces for the same mesh.
 * Key. One uint64 per slot: ix | iy << 20 | iz << 40 | kind << 60. Let v1, v2 be the corner distances at the two ends p1, p2 of the
 *   cube edge mcInterpolate (marchcubes.go:76-98) is called on for that slot. If it returns p1 or p2 unchanged -- exactly one of
 *   |v1|, |v2| is below 1e-12 -- the key names that LATTICE POINT: kind 3, (ix, iy, iz) = the leaf's integer coordinates + that
 *   corner's offset (0 or 1 per axis). Otherwise (both or neither below 1e-12, a NaN included: the comparison is false) it names the
 *   LATTICE EDGE: kind = the axis the edge runs along (0 x, 1 y, 2 z), (ix, iy, iz) = the leaf's coordinates + the offset of the
 *   edge's lower end. The leaf's coordinates are those of its cut-leaf record (0 .. 2^(levels-1) - 1).
 * Vertices. A vertex is the set of slots with one key. Vertices are numbered by the smallest slot they contain, in increasing order;
 *   a vertex's position is the position that smallest slot has in the marched soup, bit for bit. (The other slots of the vertex
 *   lie within a few ulp of it: far below res / 64 per coordinate at the 17 levels the mesher allows.)
 * Faces. idx[s] is the number of slot s's vertex. All F triangles are kept, degenerate ones included: F == stats.n_tris.
 * Determinism. The result is a function of the records alone, not of the order in which threads arrive.
 *
 * gsdf_hip_mesh_weld takes a mesh of the octree mesher made with payload = GSDF_PAYLOAD_RECORDS and shard_count == 1, marched
 * in place already (gsdf_hip_mesh_march: the mesh keeps its records for this) or not (the mesh stays as it is). Every other mesh
 * -- triangle payload, flat, dual contouring, minecraft, gathered, sharded -- is refused with GSDF_ERR_BAD_ARGUMENT and a text that
 * says what is required; a mesh with 3 F >= 2^32 with GSDF_ERR_CAPACITY; an empty one with GSDF_ERR_EMPTY_BUFFERS. The result is
 * independent of the mesh afterwards. Kernels: gsdf_amd/csrc/kernels_weld.h, launched by abi_indexed.hip. */
typedef struct gsdf_indexed gsdf_indexed; /* welded mesh, resident in HBM */
typedef struct gsdf_indexed_stats {
  double ms_keys;        /* device time, HIP events: the slots' keys from the records */
  double ms_insert;      /* the hash table (all attempts) */
  double ms_number;      /* owner lookup, vertex numbering, position gather, index write */
  double ms_ply;         /* the last PLY pack (0 before gsdf_hip_indexed_ply / _host_ply) */
  uint64_t probes;       /* table cells inspected by the inserting pass that succeeded */
  uint64_t table_cells;  /* its capacity (a power of two, >= 2 V) */
  int32_t attempts;      /* inserting passes run: 1 unless the table had to grow */
  int32_t has_normals;
} gsdf_indexed_stats;
GSDF_ABI_ASSERT(sizeof(gsdf_indexed_stats) == 56, "gsdf_indexed_stats is 56 bytes");
int gsdf_hip_mesh_weld(const gsdf_mesh* m, gsdf_indexed** out);
/* Each output optional. ms_device: device time of the whole weld (keys + table + numbering), HIP events. */
int gsdf_hip_indexed_counts(const gsdf_indexed* ix, uint64_t* n_verts, uint64_t* n_tris, double* ms_device);
int gsdf_hip_indexed_stats_get(const gsdf_indexed* ix, gsdf_indexed_stats* st);
/* Host copies, each optional: verts 3 V floats, idx 3 F vertex numbers, keys V (the key of each vertex: what a later weld across
 * shards would match on). */
int gsdf_hip_indexed_read(const gsdf_indexed* ix, float* verts, uint32_t* idx, uint64_t* keys);
/* gleval.NormalsCentralDiff (gleval/gleval.go:53-108; not normalised) of program p at the welded vertices, kept on device: the
 * values gsdf_hip_normals3 gives at the same points with the same step. The PLY carries them from then on; _read_normals copies
 * them out (3 V floats). */
int gsdf_hip_indexed_normals(gsdf_indexed* ix, gsdf_program* p, float step);
int gsdf_hip_indexed_read_normals(const gsdf_indexed* ix, float* normals);
/* Binary PLY, packed on device and moved by one DMA. The file: the header lines "ply", "format binary_little_endian 1.0", one
 * "comment gsdf" line padded with spaces so that the header's length is a multiple of 4, "element vertex V", "property float x" /
 * y / z (and nx / ny / nz once normals were asked for), "element face F", "property list uchar int vertex_indices", "end_header",
 * each ended by '\n'; then V records of 3 (6) little-endian floats; then F records of one byte 3 and three little-endian int32.
 * _ply copies it into dst (*len = its size; dst NULL or cap short: GSDF_ERR_SHORT_BUFFER with *len set); _host_ply returns a view
 * of pinned host memory the handle owns, valid until the next gsdf_hip_indexed_normals or gsdf_hip_indexed_destroy. */
int gsdf_hip_indexed_ply(gsdf_indexed* ix, uint8_t* dst, size_t cap, size_t* len);
int gsdf_hip_indexed_host_ply(gsdf_indexed* ix, const uint8_t** ply, size_t* len);
void gsdf_hip_indexed_destroy(gsdf_indexed* ix);

/* ---- indexed meshes: report and extract (no reference counterpart) --------------------------------------------------------------
 *
 * What one asks of a mesh before it goes to a slicer: is it watertight and consistently oriented, how many shells has it, what are
 * their volume, area and centre of mass, and the mesh without some of them. All of it is computed on the device from the handle's
 * vertices and faces; the counts are functions of the faces alone, the measures of faces and positions, NONE of the order in which
 * threads arrive or of the order of the faces (Determinism below). Kernels: gsdf_amd/csrc/kernels_topo.h (abi_indexed.hip); a numpy restatement:
 * tests/toporef.py.
 *
 * Faces. A face with two equal indices is DEGENERATE: counted, and otherwise absent from everything below. A non-degenerate face
 *   with a NaN or infinite coordinate is NONFINITE: it takes part in the topology (pairs, shells, counts) and not in the measures
 *   (area, volume, centroid, bbox). A vertex is USED if a non-degenerate face names it.
 * Pairs. Over the non-degenerate faces (a, b, c), the directed edges (a, b), (b, c), (c, a); per UNORDERED pair {p, q}, p < q,
 *   f = its uses as (p, q) and r = its uses as (q, p). edges = distinct pairs; a pair is a BOUNDARY edge if f + r == 1, NON-MANIFOLD
 *   if f + r > 2, MISORIENTED if f + r == 2 and f != 1. euler = used_verts - edges + (n_tris - degenerate).
 *   closed_oriented = degenerate == 0 and no boundary, non-manifold or misoriented edge: every directed edge used once each way.
 * Shells. The connected components of the graph whose nodes are the used vertices and whose edges are the pairs. A shell's LABEL is
 *   its smallest vertex number; shells are numbered 0 .. n_shells - 1 in increasing order of their labels. A face belongs to the
 *   shell of its vertices, a pair to the shell of its vertices. Per shell: the same counts, euler = n_verts - edges + n_tris
 *   (n_tris: its non-degenerate faces), and the same measures.
 * Measures, per FINITE non-degenerate face with corner positions a, b, c, each coordinate taken as (double)float32 (exact); every
 *   operation below is one IEEE float64 operation, in this order, none contracted (the library is built with -ffp-contract=off and
 *   these kernels are never part of a per-tree fast-math build):
 *     u = b - a, w = c - a;  n = (u.y w.z - u.z w.y, u.z w.x - u.x w.z, u.x w.y - u.y w.x)
 *     area term   = 0.5 * sqrt((n.x n.x + n.y n.y) + n.z n.z)                       (correctly rounded square root)
 *     m = (b.y c.z - b.z c.y, b.z c.x - b.x c.z, b.x c.y - b.y c.x);  det = (a.x m.x + a.y m.y) + a.z m.z
 *     volume term = det / 6;   moment term k = (det * ((a_k + b_k) + c_k)) / 24     (k = x, y, z)
 *   bbox = min / max of the corner coordinates, compared as order-preserving float32 bits (-0 below +0); with no finite face
 *   min = +inf, max = -inf.
 * Determinism. Let e (`exponent`) be the smallest integer >= -125 with |x| < 2^e for every FINITE coordinate x of the handle's V
 *   vertices (from the largest |bits|: e = max(biased exponent, 1) - 126; -125 for a mesh of zeros). Then area term < 2^(2e+3),
 *   |volume term| < 2^(3e), |moment term| < 2^(4e). Each term is multiplied by the power of two 2^(59-2e), 2^(62-3e), 2^(62-4e)
 *   (exact), rounded to the nearest integer, ties to even: |q| <= 2^62. The q are summed as INTEGERS (on the device: q's low 32 bits
 *   and its arithmetic-shifted rest in separate 64-bit words, which the 2^31 faces a handle can hold cannot overflow; sum = rest
 *   sum * 2^32 + low sum), so any reduction tree and any order of atomics give the same sum. The result is that integer, converted to
 *   float64 with ONE rounding (to nearest even), times the inverse power of two (exact: never subnormal). A mesh's sums are the sums
 *   of its shells' integers. centroid_k = moment_k / volume, one float64 division; the quiet NaN 0x7ff8000000000000 where volume == 0.
 *   Error of the quantisation: at most n_tris / 2 units of 2^(3e-62) for the volume, i.e. n_tris * 2^-66 of the volume of the cube
 *   [-2^e, 2^e]^3 that holds the mesh (< 2^-35 of it at 2^31 faces); likewise n_tris / 2 units of 2^(2e-59) for the area, i.e. n_tris * 2^-62 of that cube's face 2^(2e+2): both far
 *   below what float32 positions carry (2^-24 relative per coordinate). Derived, not measured.
 *
 * gsdf_hip_indexed_create uploads a host mesh (a PLY read back, or any mesh): verts 3 V floats, idx 3 F vertex numbers, keys V or
 *   NULL (then they read back as 0). The device of the calling thread (gsdf_hip_init). An index >= n_verts: GSDF_ERR_BAD_ARGUMENT,
 *   the text names the face and the index; n_tris == 0 or n_verts == 0: GSDF_ERR_EMPTY_BUFFERS; 3 F >= 2^32 or V >= 2^32:
 *   GSDF_ERR_CAPACITY. Every accessor above works on the result (its gsdf_indexed_stats times are 0).
 * gsdf_hip_indexed_report computes the report once per handle (later calls return the same bytes). Bytes 0 .. 159 of the struct
 *   (n_verts .. exponent) are a function of the mesh alone; the rest says what this run cost. GSDF_HIP_TOPO_CELLS_MIN (environment)
 *   lowers the edge table's first size so that tests can drive the grow-and-repeat path, as GSDF_HIP_WELD_CELLS_MIN does.
 * gsdf_hip_indexed_shells: one record per shell, in shell order. dst NULL: *n = n_shells; cap < n_shells: GSDF_ERR_SHORT_BUFFER with
 *   *n set.
 * gsdf_hip_indexed_read_shell_of: each optional; the shell NUMBER of every vertex (V) and face (F), 0xffffffff for a vertex that is
 *   not used / a degenerate face.
 * gsdf_hip_indexed_extract: a new, independent handle with the faces of the kept shells (keep_shell: n_shells bytes, non-zero =
 *   keep; NULL = all) in their original order; degenerate faces are kept only if drop_degenerate == 0 and keep_shell == NULL.
 *   Vertices are renumbered by the smallest slot 3 g + c (g: position among the kept faces) that names them, in increasing order --
 *   the weld's own rule; positions, keys and, if present, normals are carried bit for bit. Nothing kept: GSDF_ERR_EMPTY_BUFFERS. */
typedef struct gsdf_indexed_report {
  uint64_t n_verts, n_tris;
  uint64_t degenerate, nonfinite, used_verts;
  uint64_t edges, boundary_edges, nonmanifold_edges, misoriented_edges;
  uint64_t n_shells;
  int64_t euler;
  double area, volume, centroid[3];
  float bbox[6];            /* min x y z, max x y z */
  int32_t closed_oriented;  /* 0 / 1 */
  int32_t exponent;         /* e of the contract */
  double ms_edges;          /* device time, HIP events: exponent scan + edge table (all attempts) */
  double ms_shells;         /* union-find, roots, numbering */
  double ms_measure;        /* face measures + pair classes */
  uint64_t probes;          /* table cells inspected by the inserting pass that succeeded */
  uint64_t table_cells;     /* its capacity (a power of two, >= 2 edges) */
  int32_t attempts;         /* inserting passes run */
  int32_t reserved;
} gsdf_indexed_report;
GSDF_ABI_ASSERT(sizeof(gsdf_indexed_report) == 208, "gsdf_indexed_report is 208 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_indexed_report, degenerate) == 16 && offsetof(gsdf_indexed_report, edges) == 40 && offsetof(gsdf_indexed_report, n_shells) == 72, "gsdf_indexed_report counts");
GSDF_ABI_ASSERT(offsetof(gsdf_indexed_report, euler) == 80 && offsetof(gsdf_indexed_report, area) == 88 && offsetof(gsdf_indexed_report, centroid) == 104, "gsdf_indexed_report measures");
GSDF_ABI_ASSERT(offsetof(gsdf_indexed_report, bbox) == 128 && offsetof(gsdf_indexed_report, closed_oriented) == 152 && offsetof(gsdf_indexed_report, exponent) == 156, "gsdf_indexed_report box");
GSDF_ABI_ASSERT(offsetof(gsdf_indexed_report, ms_edges) == 160 && offsetof(gsdf_indexed_report, probes) == 184 && offsetof(gsdf_indexed_report, attempts) == 200, "gsdf_indexed_report cost");
typedef struct gsdf_shell {
  uint64_t n_verts, n_tris; /* n_tris: non-degenerate faces, nonfinite ones included */
  uint64_t nonfinite;
  uint64_t edges, boundary_edges, nonmanifold_edges, misoriented_edges;
  int64_t euler;
  double area, volume, centroid[3];
  float bbox[6];
  uint32_t label;           /* the shell's smallest vertex number */
  uint32_t reserved;
} gsdf_shell;
GSDF_ABI_ASSERT(sizeof(gsdf_shell) == 136, "gsdf_shell is 136 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_shell, nonfinite) == 16 && offsetof(gsdf_shell, edges) == 24 && offsetof(gsdf_shell, euler) == 56, "gsdf_shell counts");
GSDF_ABI_ASSERT(offsetof(gsdf_shell, area) == 64 && offsetof(gsdf_shell, centroid) == 80 && offsetof(gsdf_shell, bbox) == 104 && offsetof(gsdf_shell, label) == 128, "gsdf_shell measures");
int gsdf_hip_indexed_create(const float* verts, uint64_t n_verts, const uint32_t* idx, uint64_t n_tris, const uint64_t* keys, gsdf_indexed** out);
int gsdf_hip_indexed_report(gsdf_indexed* ix, gsdf_indexed_report* rep);
int gsdf_hip_indexed_shells(gsdf_indexed* ix, gsdf_shell* dst, uint64_t cap, uint64_t* n);
int gsdf_hip_indexed_read_shell_of(gsdf_indexed* ix, uint32_t* shell_of_vertex, uint32_t* shell_of_face);
int gsdf_hip_indexed_extract(gsdf_indexed* ix, const uint8_t* keep_shell, int drop_degenerate, gsdf_indexed** out);

/* ---- indexed meshes: mass properties (no reference counterpart) -------------------------------------------------------------------
 *
 * One polynomial degree above the report: the second moments of the solid a mesh bounds, per shell and for the mesh, and from them
 * the inertia tensor about the centre of mass and its principal axes. Computed on the device by the scheme of "report and extract"
 * above, with its exponent e, its shells and its faces (degenerate and NONFINITE faces are absent), so order-independent to the bit.
 * Kernel: gsdf_amd/csrc/kernels_mass.h (abi_indexed.hip); host arithmetic: gsdf_amd/csrc/mass_host.h; a numpy / Python-integer
 * restatement: tests/massref.py.
 *
 * Terms, per FINITE non-degenerate face with corners a, b, c as (double)float32 and the report's det (the same operations in the
 *   same order: the volume and first-moment integers of a shell ARE the report's). Let s_k = (a_k + b_k) + c_k. For the six pairs
 *   (i, j) = xx, yy, zz, xy, xz, yz, in this order everywhere below:
 *     second term ij = (det * ((((a_i a_j) + (b_i b_j)) + (c_i c_j)) + (s_i s_j))) / 120
 *   every operation one IEEE float64 operation, none contracted: the integral of x_i x_j over the tetrahedron (0, a, b, c), signed
 *   as its volume is.
 * Bound (derived, not measured). |det| < 6 2^(3e) (six products of three coordinates), the bracket < 12 2^(2e) (|s_k| < 3 2^e), so
 *   |term| < 72 / 120 2^(5e) = 0.6 2^(5e). The term is multiplied by the power of two 2^(62-5e) (exact; for e = -125 .. 128 a normal
 *   double between 2^-578 and 2^687), rounded to the nearest integer, ties to even: |q| < 2^62. The q are summed as the report's are
 *   (low 32 bits and arithmetic-shifted rest in separate 64-bit words). second_ij = that integer converted to float64 with ONE
 *   rounding, times 2^(5e-62) (exact: never subnormal). Error of the quantisation: at most n_tris / 2 units of 2^(5e-62), i.e.
 *   n_tris 2^-68 of 2^(5e+5), the second moment of the cube [-2^e, 2^e]^3 that holds the mesh about its own centre being 2^(5e+3) / 3.
 * The record. volume and first[k] (the report's moment sums: first_k = the integral of x_k, so that the report's centroid_k =
 *   first_k / volume) come from the report's integers, second[6] from the sums above. Derived, on the host, one float64 operation
 *   each, in this order:
 *     centroid_k = first_k / volume                                              (the report's bytes)
 *     C_ij       = second_ij - ((first_i * first_j) / volume)                    (central second moments)
 *     inertia    = (C_yy + C_zz, C_xx + C_zz, C_xx + C_yy, -C_xy, -C_xz, -C_yz)  (xx, yy, zz, xy, xz, yz; unit density)
 *   With volume == 0 every centroid and inertia entry is the quiet NaN 0x7ff8000000000000. A mesh's integers are the sums of its
 *   shells' integers (label 0xffffffff); a cavity's shell has negative volume and moments, so that the sums are the material's.
 *   C cancels for a part far from the origin: the raw sums stay exact to the quantisation above whatever the position, while
 *   centroid and inertia of a part of size d at distance D lose about 2 log2(D / d) bits -- on top of what float32 positions
 *   carry (2^-24 of D per coordinate). Translate the part to the origin first if that matters. The derived values are what IEEE
 *   arithmetic gives in the order stated: first_i * first_j is formed before the division, so at the very ends of the range of
 *   e it can overflow to infinity (first moments near 2^512: an off-centre part at e = 128) or lose bits to a subnormal
 *   product (below 2^-511: a small part at e near -125) where the raw sums are still exact. exponent = e.
 * gsdf_hip_indexed_mass: total, shells and n are each optional, but shells needs n (a short buffer is reported through it) and
 *   at least one of the three must be given: otherwise GSDF_ERR_BAD_ARGUMENT, before the device is touched. shells NULL: *n =
 *   n_shells; cap < n_shells: GSDF_ERR_SHORT_BUFFER with *n set (total, if given, is filled). Runs the report if the handle has
 *   none; computed once per handle, later calls return the same bytes. gsdf_hip_indexed_mass_ms: the device time (HIP events) of
 *   the pass that made the records the calling thread's last successful gsdf_hip_indexed_mass returned; 0 before the first, and
 *   after a call that failed.
 * gsdf_hip_inertia_principal (host only, no GPU): the eigenvalues of the symmetric tensor I (inertia[6] in the order above:
 *   A00 A11 A22 A01 A02 A12) in ascending order, and a right-handed frame of unit row vectors (axes[3 k + i] = component i of axis
 *   k; unit to rounding), by the cyclic Jacobi iteration, float64, one operation at a time:
 *     A = I, V = identity. Up to 32 sweeps; a sweep begins by the stop rule: A01 == 0 and A02 == 0 and A12 == 0 ends the iteration
 *     (after 32 sweeps A is taken as it is). A sweep visits the pairs (p, q) = (0, 1), (0, 2), (1, 2), r the third index:
 *       g = A_pq; g == 0: next pair.  |A_pp| + |g| == |A_pp| and |A_qq| + |g| == |A_qq|: A_pq = A_qp = 0, next pair.
 *       theta = (A_qq - A_pp) / (2 g);  t = sgn / (|theta| + sqrt((theta theta) + 1)), sgn = 1 if theta >= 0 else -1
 *       c = 1 / sqrt((t t) + 1);  s = t c;  h = t g;  A_pp = A_pp - h;  A_qq = A_qq + h;  A_pq = A_qp = 0
 *       (x, y) = (A_rp, A_rq):  A_rp = A_pr = (c x) - (s y);  A_rq = A_qr = (s x) + (c y)
 *       for i = 0, 1, 2, (x, y) = (V_ip, V_iq):  V_ip = (c x) - (s y);  V_iq = (s x) + (c y)
 *     Order: positions (0, 1, 2) of the diagonal are sorted by compare-and-swap of positions (0, 1), (1, 2), (0, 1), swapping
 *     when the first is GREATER (equal moments keep their order). moments[k] = the k-th diagonal entry, axis k = that column of V.
 *     Sign: of axes 0 and 1, the component of largest magnitude (ties: the lowest index) is made positive by negating the axis;
 *     axis 2 = axis 0 x axis 1 = ((x1 y2) - (x2 y1), (x2 y0) - (x0 y2), (x0 y1) - (x1 y0)).
 *   An entry dropped by the second rule is below 2^-53 of both diagonal entries beside it. GSDF_ERR_BAD_ARGUMENT: a NULL pointer,
 *   a NaN or infinite entry. */
typedef struct gsdf_mass {
  double volume, first[3], second[6]; /* second: xx yy zz xy xz yz, about the origin */
  double centroid[3], inertia[6];     /* inertia: xx yy zz xy xz yz, about the centroid, unit density */
  int32_t exponent;                   /* e of the contract */
  uint32_t label;                     /* the shell's label; 0xffffffff: the whole mesh */
} gsdf_mass;
GSDF_ABI_ASSERT(sizeof(gsdf_mass) == 160, "gsdf_mass is 160 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_mass, first) == 8 && offsetof(gsdf_mass, second) == 32 && offsetof(gsdf_mass, centroid) == 80, "gsdf_mass sums");
GSDF_ABI_ASSERT(offsetof(gsdf_mass, inertia) == 104 && offsetof(gsdf_mass, exponent) == 152 && offsetof(gsdf_mass, label) == 156, "gsdf_mass derived values");
int gsdf_hip_indexed_mass(gsdf_indexed* ix, gsdf_mass* total, gsdf_mass* shells, uint64_t cap, uint64_t* n);
double gsdf_hip_indexed_mass_ms(void);
int gsdf_hip_inertia_principal(const double inertia[6], double moments[3], double axes[9]);

/* ---- indexed meshes: simplify (no reference counterpart) --------------------------------------------------------------------------
 *
 * A smaller mesh by VERTEX CLUSTERING: the used vertices fall into the cells of a cubic grid, the vertices of one cell become one
 * vertex at their mean, and the faces that still have three distinct corners are kept. Marching cubes tessellates a flat face as
 * finely as a thread flank and its vertices sit on lattice edges (features are bevelled at the scale of res already), so cells of
 * a few res are the natural first simplifier for these meshes. The result is a function of the mesh and the options alone, to the
 * bit: not of the order in which threads arrive, and (as a set of keyed vertices and of faces over keys) not of the order of the
 * faces or the numbering of the vertices. Kernels: gsdf_amd/csrc/kernels_simplify.h (abi_indexed.hip); a numpy restatement:
 * tests/simplifyref.py.
 *
 * Input. Any gsdf_indexed handle (welded, extracted, or uploaded with gsdf_hip_indexed_create) and gsdf_simplify_opts: cell > 0 and
 *   finite, origin finite, flags == 0 -- anything else is GSDF_ERR_BAD_ARGUMENT, checked before the handle is looked at.
 *   For a WELDED mesh choose an origin off the lattice planes, such as the lattice origin minus res / 2 with a cell of K res
 *   (examples/render_ply.py does): two of a marching-cubes vertex's three coordinates lie on lattice planes, in floats whose last bits
 *   depend on which leaf's copy the weld kept, i.e. on the mesher's record order, which differs from run to run. With cell faces on
 *   those planes these bits would decide the cell -- exactly as the contract says, and differently for the next run's mesh.
 * Used vertices. A vertex is USED if a non-degenerate face names it; a face is DEGENERATE if two of its indices are equal (the
 *   report's definitions). Only used vertices take part.
 * Non-finite coordinates. A used vertex with a NaN or infinite coordinate: GSDF_ERR_BAD_ARGUMENT, the text gives the number of such
 *   vertices. (A non-finite vertex that no non-degenerate face names is ignored.)
 * Cell of a vertex. Per coordinate k, c_k = floor(((double)x_k - (double)origin_k) / (double)cell): two IEEE float64 operations and
 *   a floor, nothing contracted. Some |c_k| >= 2^19: GSDF_ERR_RESOLUTION, the text names the smallest such vertex.
 * Key. (c_x + 2^19) | (c_y + 2^19) << 20 | (c_z + 2^19) << 40 | 4 << 60: kind 4, after the weld's kinds 0 .. 3. Its top four bits
 *   are 0100, so it is never the hash table's empty value (all ones).
 * Clusters. A cluster is the set of used vertices with one key; n its size. n == 1: the cluster's position is that vertex's, bit for
 *   bit. n > 1: with e the report's `exponent` (over ALL finite coordinates of the handle's V vertices, used or not),
 *     q_k = rint((double)x_k * 2^(30-e))                 exact scaling, ties to even; |q_k| <= 2^30
 *     S_k = the INTEGER sum of q_k over the cluster      |S_k| <= 2^62 for V < 2^32: an int64
 *     position_k = (float)(((double)S_k / (double)n) * 2^(e-30))
 *   -- one conversion of S_k to float64, one division, an exact scaling, one rounding to float32. The sums being integer sums, any
 *   order of atomics and any reduction tree give the same bytes. Error of the quantisation: |q_k 2^(e-30) - x_k| <= 2^(e-31) per
 *   member, hence at most 2^(e-31) for the mean per coordinate: 1/128 of a float32 ulp at magnitude 2^e (ulp 2^(e-24) in
 *   [2^(e-1), 2^e)). Derived, not measured.
 * Faces. Degenerate input faces are dropped. A non-degenerate face whose three vertices fall into fewer than three distinct clusters
 *   is COLLAPSED and dropped. Every other face is kept, in the original order, each corner replaced by its cluster. Clustering can
 *   make two kept faces equal or opposite (a thin wall inside one layer of cells): such faces are KEPT, nothing is deduplicated,
 *   and gsdf_hip_indexed_report on the result tells the truth about them (non-manifold / misoriented edges).
 * Vertices of the result. The clusters a kept face names, numbered by the smallest slot 3 g + c (g: the face's position among the
 *   kept faces) that names them, in increasing order -- the weld's and extract's rule. A vertex's key is its cluster's key. Normals
 *   are not carried (has_normals == 0): ask for them again on the result. Unlike extract, positions are new, so the result's own
 *   exponent may be smaller than the input's.
 * Nothing kept: GSDF_ERR_EMPTY_BUFFERS.
 *
 * gsdf_hip_indexed_simplify(ix, o, out, st): *out = a new, independent handle; st (optional) = the stats. out == NULL with st != NULL
 *   is a DRY RUN: the same stats, no handle built, GSDF_OK with n_tris == 0 where nothing would be kept; it costs the clustering and
 *   one counting pass over the faces. Both NULL: GSDF_ERR_BAD_ARGUMENT. On an error *out is NULL and *st is not written.
 * gsdf_simplify_stats. Bytes 0 .. 79 (n_verts_in .. reserved) are a function of the mesh and the options alone; the rest says what
 *   this run cost. GSDF_HIP_SIMPLIFY_CELLS_MIN (environment) lowers the cluster table's first size so that tests can drive the
 *   grow-and-repeat path, as GSDF_HIP_TOPO_CELLS_MIN does.
 * Not done here: quadric edge-collapse, QEF placement of the representative. (Removing duplicate or opposite faces:
 *   "indexed meshes: clean", below. Adaptive
 *   simplification, by error-bounded clustering over nested cells: "indexed meshes: adaptive simplify", below. Projecting the
 *   representatives back onto the field: gsdf_hip_indexed_project, below.) */
typedef struct gsdf_simplify_opts {
  float cell;        /* cell edge, > 0 and finite */
  float origin[3];   /* where cell (0, 0, 0) starts; finite */
  uint32_t flags;    /* 0; others refused */
  uint32_t reserved[3];
} gsdf_simplify_opts;
GSDF_ABI_ASSERT(sizeof(gsdf_simplify_opts) == 32, "gsdf_simplify_opts is 32 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_simplify_opts, origin) == 4 && offsetof(gsdf_simplify_opts, flags) == 16, "gsdf_simplify_opts fields");
typedef struct gsdf_simplify_stats {
  uint64_t n_verts_in, n_tris_in;
  uint64_t used_verts_in, degenerate_in;
  uint64_t cells;          /* clusters: distinct keys of the used vertices */
  uint64_t collapsed;      /* non-degenerate faces with fewer than three distinct clusters */
  uint64_t n_verts, n_tris; /* of the result: clusters a kept face names; n_tris_in - degenerate_in - collapsed */
  uint64_t largest_cell;   /* the largest n */
  int32_t exponent;        /* e of the contract */
  int32_t reserved;
  double ms_cells;         /* device time, HIP events: used marks, exponent, cluster table (all attempts), sums */
  double ms_faces;         /* face pass, positions; compaction, numbering, remap (not in a dry run) */
  uint64_t probes;         /* table cells inspected by the inserting pass that succeeded */
  uint64_t table_cells;    /* its capacity (a power of two, >= 2 cells) */
  int32_t attempts;        /* inserting passes run */
  int32_t reserved2;
} gsdf_simplify_stats;
GSDF_ABI_ASSERT(sizeof(gsdf_simplify_stats) == 120, "gsdf_simplify_stats is 120 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_simplify_stats, cells) == 32 && offsetof(gsdf_simplify_stats, n_verts) == 48, "gsdf_simplify_stats counts");
GSDF_ABI_ASSERT(offsetof(gsdf_simplify_stats, exponent) == 72 && offsetof(gsdf_simplify_stats, ms_cells) == 80, "gsdf_simplify_stats cost");
int gsdf_hip_indexed_simplify(gsdf_indexed* ix, const gsdf_simplify_opts* o, gsdf_indexed** out, gsdf_simplify_stats* st);

/* ---- indexed meshes: adaptive simplify (no reference counterpart) -----------------------------------------------------------------
 *
 * A smaller mesh by ERROR-BOUNDED CLUSTERING over nested grids: where the uniform simplifier above has one cell size for the whole
 * part, this one merges the vertices of the COARSEST cell, out of `levels` nested ones, whose mean stays within `tol` of the plane
 * of every face that touches the cell. A flat face collapses into cells of 2^(levels-1) finest cells; a thread flank keeps the
 * finest cells, or its vertices. Like every stage here, and unlike edge-collapse, the result is a function of the mesh and the
 * options alone, to the bit: integer sums, minima and maxima only. Kernels: gsdf_amd/csrc/kernels_simplify_adaptive.h
 * (abi_indexed.hip); a numpy restatement: tests/adaptiveref.py.
 *
 * Input. Any gsdf_indexed handle and gsdf_adaptive_opts: cell (the FINEST cell's edge) > 0 and finite, origin finite, tol >= 0 and
 *   finite, levels 1 .. 16, flags == 0 -- anything else is GSDF_ERR_BAD_ARGUMENT, checked before the handle is looked at. Used
 *   vertices, degenerate faces and non-finite used vertices (GSDF_ERR_BAD_ARGUMENT): as in "simplify". The advice on the origin for a
 *   welded mesh holds here too.
 * Nested cells. The level-0 cell of a vertex is c_k of "simplify", computed exactly so (two float64 operations and a floor). Some
 *   |c_k| >= 2^17: GSDF_ERR_RESOLUTION, the text names the smallest such vertex. Its level-l cell is c_k >> l, an ARITHMETIC shift
 *   (floor of c_k / 2^l), l = 0 .. levels-1: a level-(l+1) cell is the union of 8 level-l cells, exactly.
 * Key of a cell. ((c_x >> l) + 2^17) | ((c_y >> l) + 2^17) << 18 | ((c_z >> l) + 2^17) << 36 | l << 54 | 6 << 60: kind 6, after the
 *   weld's kinds 0 .. 3, the simplifier's 4 and dual contouring's 5. Its top four bits are 0110: never the hash table's empty value.
 * Position of a cell, at every level: the "simplify" formula over the used vertices in the cell, verbatim. n == 1: that vertex's
 *   bits. n > 1: q_k = rint((double)x_k * 2^(30-e)), S_k their integer sum, position_k = (float)(((double)S_k / (double)n) * 2^(e-30)),
 *   e the report's exponent of the input.
 * Error of a cell. The largest distance from the cell's position r (float32, widened) to the plane of a NON-DEGENERATE face that has
 *   a corner in the cell -- in float64, nothing contracted, from the float32 vertices pa, pb, pc of the face widened:
 *     u = pb - pa, w = pc - pa                                     (one float64 subtraction per coordinate)
 *     n = (u_y w_z - u_z w_y, u_z w_x - u_x w_z, u_x w_y - u_y w_x)
 *     L = sqrt((n_x n_x + n_y n_y) + n_z n_z)                      a face with !(L > 0) has no plane and contributes nothing
 *     g = r - pa
 *     t = |(n_x g_x + n_y g_y) + n_z g_z| / L
 *     err(cell) = max t over the (face, corner) pairs whose corner's vertex is in the cell; 0 where there is none
 *   No intermediate overflows: |x| < 2^128 for a finite float32, so |u_k|, |w_k|, |g_k| < 2^129, a product < 2^258, |n_k| < 2^259,
 *   n_k n_k < 2^518, their sum < 2^520, L < 2^260, |n . g| < 3 * 2^388 < 2^390 -- all far below 2^1024. Squares may UNDERFLOW:
 *   a sliver's L is then 0 (the face has no plane) or, if positive, at least 2^-537 (the root of the smallest subnormal), so the
 *   quotient t stays below 2^390 * 2^537 = 2^927: finite.
 *   The maximum is order-independent: non-negative float64 order as their bit patterns, so a 64-bit unsigned maximum gives the same
 *   bytes in any order of arrival.
 * Choice. A cell is ACCEPTED iff err <= (double)tol. A vertex's cluster is its ancestor cell (its own cells at levels 0 .. levels-1)
 *   at the LARGEST accepted level; the cells below it need not be accepted. A vertex with no accepted ancestor, or whose cluster has
 *   n == 1, is SINGLE: it keeps its position bits and its INPUT key (the handle's key of that vertex). The grids nest, so all
 *   vertices of a chosen cell choose it: the clusters and the singles are a partition of the used vertices. Raising tol or levels
 *   only coarsens the partition (every cluster of the finer one lies inside one cluster of the coarser one): an accepted cell stays
 *   accepted under a larger tol, and a new level only adds candidates above the old ones. Hence n_verts and n_tris do not increase
 *   along either.
 * Faces, vertices of the result, nothing kept: as in "simplify", with the cluster or the single where it has the cluster. Degenerate
 *   and collapsed faces are dropped, the rest stay in order; result vertices are numbered by the smallest kept slot; nothing is
 *   deduplicated and the report of the result tells the truth; has_normals == 0. Nothing kept: GSDF_ERR_EMPTY_BUFFERS.
 * With levels == 1 and a tol no error exceeds, positions, faces and numbering are those of "simplify" with the same cell and origin.
 * An accepted cell that spans a wall thinner than 2 tol collapses the wall, as a uniform cell does.
 *
 * gsdf_hip_indexed_simplify_adaptive(ix, o, out, st): as gsdf_hip_indexed_simplify; out == NULL with st != NULL is a DRY RUN with the
 *   same leading stats, GSDF_OK with n_tris == 0 where nothing would be kept. Both NULL: GSDF_ERR_BAD_ARGUMENT.
 * gsdf_adaptive_stats. Bytes 0 .. 223 (n_verts_in .. reserved) are a function of the mesh and the options alone; the rest says what
 *   this run cost. Only an accepted cell's error is complete (the kernel stops raising a cell's word once it is beyond tol), and
 *   only those reach max_err. GSDF_HIP_SIMPLIFY_CELLS_MIN lowers this table's first size too.
 * Run to run. A welded mesh's last bits vary with the mesher's record order (see "simplify"), and here they can also flip an
 *   err <= tol decision, so two welds of one part may differ in a few clusters. A handle from gsdf_hip_mesh_dualcontour_indexed
 *   does not vary, so its adaptive result is reproducible byte for byte.
 * Not done here: edge-collapse, QEF placement, un-flipping folded faces. (Removing duplicate or opposite faces: "indexed meshes:
 *   clean", below.) */
typedef struct gsdf_adaptive_opts {
  float cell;        /* the finest cell's edge, > 0 and finite */
  float origin[3];   /* where cell (0, 0, 0) of every level starts; finite */
  float tol;         /* the largest accepted error, >= 0 and finite */
  uint32_t levels;   /* 1 .. 16 nested grids: cells of 1, 2, .. 2^(levels-1) finest cells */
  uint32_t flags;    /* 0; others refused */
  uint32_t reserved;
} gsdf_adaptive_opts;
GSDF_ABI_ASSERT(sizeof(gsdf_adaptive_opts) == 32, "gsdf_adaptive_opts is 32 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_adaptive_opts, origin) == 4 && offsetof(gsdf_adaptive_opts, tol) == 16 && offsetof(gsdf_adaptive_opts, levels) == 20 &&
                offsetof(gsdf_adaptive_opts, flags) == 24, "gsdf_adaptive_opts fields");
typedef struct gsdf_adaptive_stats {
  uint64_t n_verts_in, n_tris_in;
  uint64_t used_verts_in, degenerate_in;
  uint64_t cells;            /* distinct cells of the used vertices, over all levels */
  uint64_t chosen[16];       /* chosen clusters of more than one vertex, per level */
  uint64_t singles;          /* used vertices that stay alone */
  uint64_t collapsed;        /* non-degenerate faces with fewer than three distinct clusters */
  uint64_t n_verts, n_tris;  /* of the result: clusters and singles a kept face names; n_tris_in - degenerate_in - collapsed */
  uint64_t largest_cluster;  /* the largest n chosen (1 where every used vertex stays alone, 0 where none is used) */
  double max_err;            /* the largest error of a chosen cluster of more than one vertex; 0 where there is none */
  int32_t exponent;          /* e of the contract */
  int32_t reserved;
  double ms_cells;           /* device time, HIP events: used marks, exponent, table (all attempts), sums, positions */
  double ms_error;           /* the cells' errors, the choice */
  double ms_faces;           /* face pass; compaction, numbering, remap (not in a dry run) */
  uint64_t probes;           /* table cells inspected by the inserting pass that succeeded */
  uint64_t table_cells;      /* its capacity (a power of two, >= 2 cells) */
  int32_t attempts;          /* inserting passes run */
  int32_t reserved2;
} gsdf_adaptive_stats;
GSDF_ABI_ASSERT(sizeof(gsdf_adaptive_stats) == 272, "gsdf_adaptive_stats is 272 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_adaptive_stats, cells) == 32 && offsetof(gsdf_adaptive_stats, chosen) == 40 && offsetof(gsdf_adaptive_stats, singles) == 168,
                "gsdf_adaptive_stats counts");
GSDF_ABI_ASSERT(offsetof(gsdf_adaptive_stats, n_verts) == 184 && offsetof(gsdf_adaptive_stats, max_err) == 208 && offsetof(gsdf_adaptive_stats, exponent) == 216 &&
                offsetof(gsdf_adaptive_stats, ms_cells) == 224, "gsdf_adaptive_stats result and cost");
int gsdf_hip_indexed_simplify_adaptive(gsdf_indexed* ix, const gsdf_adaptive_opts* o, gsdf_indexed** out, gsdf_adaptive_stats* st);

/* ---- indexed meshes: clean (no reference counterpart) ------------------------------------------------------------------------------
 *
 * Vertices with EQUAL positions merged, degenerate faces dropped, and of the faces over one set of three vertices at most one kept:
 * what joins a triangle soup uploaded with gsdf_hip_indexed_create (an STL read back, any triangle list whose shared corners are
 * the same floats) into an indexed mesh, and what removes the equal and opposite faces that clustering leaves where a wall is thinner
 * than a cell ("simplify", "adaptive simplify"). All of it is integer work: the result is a function of the mesh and the flags
 * alone, to the byte, under any order of arrival. Kernels: gsdf_amd/csrc/kernels_clean.h (abi_indexed.hip); a numpy restatement:
 * tests/cleanref.py.
 *
 * Input. Any gsdf_indexed handle and gsdf_clean_opts: flags a non-empty subset of GSDF_CLEAN_MERGE_POSITIONS | GSDF_CLEAN_FACES, the
 *   reserved words 0 -- anything else (flags == 0, an unknown bit, a non-zero reserved word) is GSDF_ERR_BAD_ARGUMENT, checked before
 *   the handle is looked at.
 * 1. Merge (only with GSDF_CLEAN_MERGE_POSITIONS). A vertex's POSITION KEY is its three float32 bit patterns, with 0x80000000 (-0)
 *   replaced by 0. A vertex with a NaN or infinite coordinate is never merged: it is a class of its own. ALL vertices take part, used
 *   or not. The vertices with one key form a CLASS, and every index that names a member is replaced by the class's SMALLEST vertex
 *   number. merged_verts = the sum of (members - 1) over the classes. Without the flag every vertex is its own class, merged_verts 0.
 * 2. Degenerate faces. After step 1 a face with two equal indices is DEGENERATE (the report's definition), counted in `degenerate`
 *   -- the faces that were degenerate on input included -- and dropped.
 * 3. Face sets (only with GSDF_CLEAN_FACES). Of a non-degenerate face (a, b, c), after step 1: its SET is the sorted triple
 *   lo < mid < hi; its ORIENTATION is + if (a, b, c) is a rotation of (lo, mid, hi) and - if it is a rotation of (lo, hi, mid). Per
 *   set, f = the number of its + faces and r = the number of its - faces. The rule, the whole of it:
 *     f == r: every face of the set is dropped. The set is CANCELLED, and all f + r faces count as opposite_faces.
 *     f != r: exactly ONE face is kept, the smallest-numbered face of the majority orientation, its corners in the order it has them
 *             (not rotated). Of the dropped ones 2 min(f, r) count as opposite_faces and the other |f - r| - 1 as duplicate_faces.
 *   face_sets = the distinct sets, cancelled_sets = those with f == r, largest_set = the largest f + r (0 where there is no set).
 *   Without the flag every non-degenerate face is kept, and face_sets, cancelled_sets, duplicate_faces, opposite_faces and
 *   largest_set are 0.
 * 4. Result. The kept faces in their original order. Its vertices are the classes a kept face names, numbered by the smallest slot
 *   3 g + c (g: the face's position among the kept faces) that names them, in increasing order -- the weld's, extract's and
 *   simplify's rule. Position, key and normal (has_normals carries over as in extract: positions do not change) are those of the
 *   class's smallest-numbered member, bit for bit: the -0 of the position key is for grouping only, the stored bits are the
 *   member's own. n_verts, n_tris: of the result. Nothing kept: GSDF_ERR_EMPTY_BUFFERS.
 * 5. Derived guarantees (tests/test_clean_ref.py holds the restatement to them by brute force).
 *   (i)   Idempotent: cleaning the result with the same flags drops nothing and returns the same bytes. (Smallest members have
 *         distinct keys; a kept face is alone in its set.)
 *   (ii)  After GSDF_CLEAN_FACES no two faces of the result have one set.
 *   (iii) Removing one + and one - face of a set removes each of its three vertex pairs once in each direction. So where
 *         duplicate_faces == 0, every pair {p, q} of vertices has the same f - r (the report's uses as (p, q) minus its uses as
 *         (q, p)) before and after, over the classes of step 1. In particular a mesh in which every pair has f == r (no boundary,
 *         no misoriented edge; non-manifold edges allowed) keeps that property, and its non-manifold edges at cancelled sheets fall
 *         from 2 + 2 uses to 1 + 1.
 *   (iv)  With duplicate_faces > 0 signed volume and edge balance may change: the stats say so, and gsdf_hip_indexed_report of the
 *         result tells the truth, as everywhere else.
 *   NOT promised: that the result is closed; hole filling; re-orienting shells; merging vertices that are merely CLOSE -- the
 *   copies of a corner that neighbouring cubes of a mesher emit differ in their last bits (see "indexed meshes", the weld; the
 *   minecraft mesher's faces too: a corner is origin + res i + res in one cube and origin + res (i + 1) in the next): weld
 *   marching-cubes meshes from records, or cluster with "simplify".
 * Limits. 3 F < 2^32 and V < 2^32, as gsdf_hip_indexed_create enforces.
 *
 * gsdf_hip_indexed_clean(ix, o, out, st): as gsdf_hip_indexed_simplify. *out = a new, independent handle; st (optional) = the stats.
 *   out == NULL with st != NULL is a DRY RUN: the same stats, no handle built, GSDF_OK with n_tris == 0 where nothing would be kept.
 *   Both NULL: GSDF_ERR_BAD_ARGUMENT. On an error *out is NULL and *st is not written.
 * gsdf_clean_stats. Bytes 0 .. 87 (n_verts_in .. n_tris) are a function of the mesh and the flags alone, and
 *   n_tris == n_tris_in - degenerate - duplicate_faces - opposite_faces; the rest says what this run cost, per table (0 for a table
 *   the flags do not ask for). GSDF_HIP_CLEAN_CELLS_MIN (environment) lowers both tables' first size so that tests can drive the
 *   grow-and-repeat path, as GSDF_HIP_SIMPLIFY_CELLS_MIN does. */
#define GSDF_CLEAN_MERGE_POSITIONS 1u
#define GSDF_CLEAN_FACES 2u
typedef struct gsdf_clean_opts {
  uint32_t flags;    /* GSDF_CLEAN_MERGE_POSITIONS | GSDF_CLEAN_FACES, not 0; others refused */
  uint32_t reserved[3];
} gsdf_clean_opts;
GSDF_ABI_ASSERT(sizeof(gsdf_clean_opts) == 16, "gsdf_clean_opts is 16 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_clean_opts, flags) == 0 && offsetof(gsdf_clean_opts, reserved) == 4, "gsdf_clean_opts fields");
typedef struct gsdf_clean_stats {
  uint64_t n_verts_in, n_tris_in;
  uint64_t merged_verts;      /* sum over the classes of (members - 1) */
  uint64_t degenerate;        /* faces with two equal indices after the merge */
  uint64_t face_sets;         /* distinct sets of the non-degenerate faces */
  uint64_t cancelled_sets;    /* sets with f == r */
  uint64_t duplicate_faces;   /* dropped faces of a kept face's own orientation beyond the opposite pairs */
  uint64_t opposite_faces;    /* dropped faces that pair up, one + with one -: even */
  uint64_t largest_set;       /* the largest f + r */
  uint64_t n_verts, n_tris;   /* of the result */
  double ms_merge;            /* device time, HIP events: vertex table (all attempts), classes, the merged faces */
  double ms_faces;            /* face table (all attempts), the rule, the named classes */
  double ms_result;           /* compaction, numbering, remap (0 in a dry run) */
  uint64_t vert_probes;       /* vertex table: cells inspected by the inserting pass that succeeded */
  uint64_t vert_table_cells;  /* its capacity (a power of two, >= 2 classes of finite vertices) */
  uint64_t face_probes;       /* face table: the same */
  uint64_t face_table_cells;  /* its capacity (a power of two, >= 2 face_sets) */
  int32_t vert_attempts;      /* inserting passes run, per table */
  int32_t face_attempts;
} gsdf_clean_stats;
GSDF_ABI_ASSERT(sizeof(gsdf_clean_stats) == 152, "gsdf_clean_stats is 152 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_clean_stats, merged_verts) == 16 && offsetof(gsdf_clean_stats, face_sets) == 32 && offsetof(gsdf_clean_stats, duplicate_faces) == 48,
                "gsdf_clean_stats counts");
GSDF_ABI_ASSERT(offsetof(gsdf_clean_stats, largest_set) == 64 && offsetof(gsdf_clean_stats, n_verts) == 72 && offsetof(gsdf_clean_stats, n_tris) == 80,
                "gsdf_clean_stats result");
GSDF_ABI_ASSERT(offsetof(gsdf_clean_stats, ms_merge) == 88 && offsetof(gsdf_clean_stats, vert_probes) == 112 && offsetof(gsdf_clean_stats, vert_attempts) == 144,
                "gsdf_clean_stats cost");
int gsdf_hip_indexed_clean(gsdf_indexed* ix, const gsdf_clean_opts* o, gsdf_indexed** out, gsdf_clean_stats* st);

/* ---- indexed meshes: project onto the field (no reference counterpart) -------------------------------------------------------------
 *
 * The vertices of an indexed mesh moved onto the zero set of a 3-D program by Newton steps along its central-difference gradient,
 * and, as the dry run with no step, the DEVIATION of a mesh from the part: how far its vertices are from the surface. A cluster's
 * mean (simplify) lies inside every convex part and outside every concave one, by up to about cell^2 / (8 radius of curvature); a
 * marching-cubes vertex is itself only the linear interpolate along a lattice edge. The result is a function of the mesh, the
 * program and the options alone, to the bit. Kernel: gsdf_amd/csrc/kernels_project.h (abi_eval.hip: project_dev); a numpy
 * restatement: tests/projectref.py.
 *
 * Options. step, tol, max_move finite, step > 0, tol >= 0, max_move >= 0, 0 <= max_iters <= 64, flags == 0 -- anything else is
 *   GSDF_ERR_BAD_ARGUMENT, checked before the handle is looked at. A 2-D program: GSDF_ERR_DIMENSION. A program on another device
 *   than the handle's: GSDF_ERR_BAD_ARGUMENT. h = step * 0.5f, as gsdf_hip_normals3.
 * Arithmetic. Every operation below is ONE IEEE float32 operation, never contracted; the division is correctly rounded; comparisons
 *   are IEEE (false on a NaN operand). sdf() is the program's distance, gsdf_hip_eval3's.
 * Who takes part. All V vertices, used by a face or not. A vertex with a NaN or infinite coordinate is SKIPPED: not evaluated, its
 *   position carried bit for bit, d_before and d_after the quiet NaN 0x7fc00000.
 * Per vertex. x = x0, the vertex; then for it = 0 .. max_iters:
 *   1. d = sdf(x)  (one evaluation). On it == 0, d_before = d. If d is NaN on it == 0: status NONFINITE, stop. If NOT (|d| > tol):
 *      stop, status ON when it == 0, else CONVERGED. If it == max_iters: stop, status ITERS.
 *   2. g_k = sdf(x + h e_k) - sdf(x - h e_k), k = x, y, z  (six evaluations; gsdf_hip_normals3's points and subtraction).
 *   3. s = (g.x g.x + g.y g.y) + g.z g.z. If NOT (s > 0): stop, status FLAT.
 *   4. t = (d * (h + h)) / s;  x'_k = x_k - t * g_k: the Newton step along the central-difference gradient g / 2h.
 *   5. u = x' - x0;  r = (u.x u.x + u.y u.y) + u.z u.z. If NOT (r <= max_move * max_move): stop, status CLAMPED, x stays.
 *      Otherwise x = x' (an ACCEPTED step).
 * The end. d_after is the last d of step 1: it was evaluated at the final x (a vertex that stopped at 3 or 5 evaluated d at its x
 *   in step 1 of that trip). For every vertex that is neither SKIPPED nor NONFINITE: if d_after is NaN or |d_after| > |d_before|,
 *   the status becomes REVERTED, the position is x0 bit for bit and d_after = d_before; otherwise the position is x. (A NONFINITE
 *   vertex keeps its status, its position and d_after = d_before.) So no vertex is further from the surface than it was, and none
 *   leaves the ball of radius max_move about where it started.
 * Status. One byte per vertex: GSDF_PROJECT_SKIPPED 0, _ON 1, _CONVERGED 2, _ITERS 3, _FLAT 4, _CLAMPED 5, _NONFINITE 6, _REVERTED 7.
 * Evaluations. One per step 1 reached plus six per step 2 reached; their sum is st->evals, and gsdf_hip_evaluations(p) grows by
 *   exactly that (padding lanes and finished lanes do not count, as in gsdf_hip_render3).
 *
 * gsdf_hip_indexed_project(ix, p, o, out, st): *out = a new, independent handle with the faces and the keys of ix byte for byte and
 *   the new positions; normals are not carried (has_normals == 0), the report is computed afresh on demand. The handle keeps
 *   d_before, d_after and the status per vertex for gsdf_hip_indexed_read_fit (each output optional; a handle not made by
 *   gsdf_hip_indexed_project: GSDF_ERR_BAD_ARGUMENT); extract and simplify of the result do not carry them. out == NULL with
 *   st != NULL is a DRY RUN: the same stats, no handle built; with max_iters == 0 it costs one evaluation per vertex and is the
 *   deviation report. Both NULL: GSDF_ERR_BAD_ARGUMENT. On an error *out is NULL and *st is not written. (A handle always has
 *   vertices: every call that makes one refuses an empty mesh with GSDF_ERR_EMPTY_BUFFERS.)
 * gsdf_project_stats. Bytes 0 .. 111 (n_verts .. reserved) are a function of the mesh, the program and the options alone; ms_device
 *   says what this run cost. count[k]: vertices of status k. over_tol_before / _after: vertices that took part with |d| > tol or a
 *   NaN d. max_abs_before / _after: the largest non-NaN |d| of a vertex that took part, 0 if none. steps_max: the most accepted steps
 *   of any vertex (a REVERTED vertex's count too). Every one is an integer sum or an integer maximum (|d|'s bits order as unsigned
 *   integers), so any order of atomics gives the same bytes.
 * Not done here: re-meshing, feature-preserving (QEF) placement, un-flipping faces a projection folds over (the report of the result
 *   counts misoriented edges), 2-D. */
enum { GSDF_PROJECT_SKIPPED = 0, GSDF_PROJECT_ON = 1, GSDF_PROJECT_CONVERGED = 2, GSDF_PROJECT_ITERS = 3, GSDF_PROJECT_FLAT = 4,
       GSDF_PROJECT_CLAMPED = 5, GSDF_PROJECT_NONFINITE = 6, GSDF_PROJECT_REVERTED = 7 };
typedef struct gsdf_project_opts {
  float step;         /* central-difference step, > 0 and finite: h = step / 2 */
  float tol;          /* a vertex is on the surface when NOT (|d| > tol); >= 0 and finite */
  float max_move;     /* no vertex ends further than this from where it started; >= 0 and finite */
  int32_t max_iters;  /* 0 .. 64 */
  uint32_t flags;     /* 0; others refused */
  uint32_t reserved[3];
} gsdf_project_opts;
GSDF_ABI_ASSERT(sizeof(gsdf_project_opts) == 32, "gsdf_project_opts is 32 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_project_opts, tol) == 4 && offsetof(gsdf_project_opts, max_move) == 8 && offsetof(gsdf_project_opts, max_iters) == 12 && offsetof(gsdf_project_opts, flags) == 16, "gsdf_project_opts fields");
typedef struct gsdf_project_stats {
  uint64_t n_verts;
  uint64_t count[8];        /* vertices per status */
  uint64_t evals;
  uint64_t over_tol_before, over_tol_after;
  float max_abs_before, max_abs_after;
  uint32_t steps_max;
  uint32_t reserved;
  double ms_device;         /* device time of the kernel, HIP events */
} gsdf_project_stats;
GSDF_ABI_ASSERT(sizeof(gsdf_project_stats) == 120, "gsdf_project_stats is 120 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_project_stats, count) == 8 && offsetof(gsdf_project_stats, evals) == 72 && offsetof(gsdf_project_stats, over_tol_before) == 80, "gsdf_project_stats counts");
GSDF_ABI_ASSERT(offsetof(gsdf_project_stats, max_abs_before) == 96 && offsetof(gsdf_project_stats, steps_max) == 104 && offsetof(gsdf_project_stats, ms_device) == 112, "gsdf_project_stats maxima and cost");
int gsdf_hip_indexed_project(gsdf_indexed* ix, gsdf_program* p, const gsdf_project_opts* o, gsdf_indexed** out, gsdf_project_stats* st);
int gsdf_hip_indexed_read_fit(const gsdf_indexed* ix, float* dist_before, float* dist_after, uint8_t* status);

/* ---- rays (no reference counterpart) --------------------------------------------------------------------------------------------
 *
 * "What does this ray hit, and how far away?": a batch of the caller's own rays sphere-traced through the field of a 3-D program,
 * from outside or from inside the part (picking, line of sight, drop to the surface), and, with the rays built from the vertices of
 * an indexed mesh along their inward normals, the WALL THICKNESS of that mesh. The result is a function of the rays (the mesh), the
 * program and the options alone, to the bit. Kernel: gsdf_amd/csrc/kernels_ray.h (abi_eval.hip: ray_dev); a numpy restatement:
 * tests/rayref.py.
 *
 * A ray is 24 bytes: the origin o[3], then the direction r[3], used as given: r is NOT normalised, so t is in units of |r|.
 *   pos(t) = (o.x + t * r.x, o.y + t * r.y, o.z + t * r.z).
 * Options (gsdf_ray_opts). t0 finite and >= 0 (a t0 of -0 is taken as +0); tmax >= t0, +Inf allowed; tol and min_step finite and
 *   >= 0; 1 <= max_steps <= 4096; 0 <= refine <= 32; flags == 0 and reserved == 0 -- anything else is GSDF_ERR_BAD_ARGUMENT.
 * Arithmetic. Every operation below is ONE IEEE float32 operation, round to nearest, never contracted; sqrt and the division are
 *   correctly rounded; comparisons are IEEE (false on a NaN operand); "d is NaN" is a test of d's bit pattern. sdf() is the program's
 *   distance, gsdf_hip_eval3's. signbit(d) is d's sign bit (set for -0).
 * Marching one ray.
 *   1. If a component of o or r is NaN or infinite: status SKIPPED, nothing is evaluated, t and d are the quiet NaN 0x7fc00000.
 *   2. t = t0, d = sdf(pos(t))  (march evaluation 1). If d is NaN: status NONFINITE. If NOT (|d| > tol): status HIT. Otherwise
 *      inside = signbit(d).
 *   3. Loop. If the march evaluations so far >= max_steps: status STEPS, reporting the last t and d. tp = t, dp = d. s = |d|; if
 *      s < min_step then s = min_step. t = tp + s. If t > tmax: status MISS, reporting tp and dp. d = sdf(pos(t))  (a march
 *      evaluation). If d is NaN: status NONFINITE. If NOT (|d| > tol): status HIT. If signbit(d) != inside: status CROSSED with the
 *      bracket a = tp, b = t, db = d, on to 4. Otherwise repeat.
 *   4. Refinement, for a CROSSED ray, up to `refine` times: m = a + (b - a) * 0.5f. Stop if NOT (m > a AND m < b). dm = sdf(pos(m))
 *      (a refine evaluation). Stop if dm is NaN. If NOT (|dm| > tol): b = m, db = dm, stop. If signbit(dm) == inside: a = m;
 *      otherwise b = m, db = dm. A CROSSED ray reports t = b, d = db: the nearest point known to lie on the far side.
 *   HIT, STEPS and NONFINITE report the t of their last evaluation; HIT and STEPS its d; NONFINITE the quiet NaN 0x7fc00000 for d.
 * Outputs per ray, each optional: t and d (floats), status (one byte, GSDF_RAY_*), steps (uint16: march plus refine evaluations).
 * Status. GSDF_RAY_SKIPPED 0, _HIT 1, _CROSSED 2, _MISS 3, _STEPS 4, _NONFINITE 5, _FLAT 6 (thickness only).
 * A query, not a guarantee. As for gsdf_hip_render3: a field that is not 1-Lipschitz (twist, a scaled part, a shell of one), or a
 *   min_step larger than a wall, can step over a wall. The sign test catches a single crossing inside a step; a double crossing --
 *   into a wall and out of it again in one step -- is missed, and the ray goes on as if the wall were not there.
 * gsdf_ray_stats. Bytes 0 .. 103 (n .. below) are a function of the inputs alone, byte for byte; ms_device says what this run cost.
 *   count[k]: rays of status k. evals: every evaluation (thickness: the six taps of every vertex that reached them too);
 *   gsdf_hip_evaluations(p) grows by exactly that (padding lanes and finished lanes do not count). steps_max: the most march plus
 *   refine evaluations of any ray. t_min, t_max: the smallest and the largest t over the HIT and CROSSED rays (+Inf and 0 when
 *   there is none). below: the HIT and CROSSED rays with t < thin (a NaN thin counts none). Every one is an integer sum, maximum or
 *   minimum (t >= 0 there, so its bits order as unsigned integers): any order of atomics gives the same bytes.
 *
 * gsdf_hip_raycast3(p, rays, n, o, thin, t_out, d_out, status_out, steps_out, st): host buffers, blocking, on the path
 *   gsdf_hip_normals3 takes. A 2-D program: GSDF_ERR_DIMENSION. n == 0: GSDF_ERR_EMPTY_BUFFERS. n >= 2^32: GSDF_ERR_CAPACITY. Bad
 *   options, a null p, rays or o, or all five outputs NULL: GSDF_ERR_BAD_ARGUMENT. On an error nothing is written.
 *
 * gsdf_hip_indexed_thickness(ix, p, o, thickness_out, status_out, st): the RAY definition of wall thickness -- per vertex, the
 *   distance to the opposite wall along the inward normal, marched through the exact field and not through triangles. At a sharp
 *   convex edge it is legitimately small. gsdf_thickness_opts is a gsdf_ray_opts plus step (the central-difference step, finite and
 *   > 0: h = step * 0.5f, as gsdf_hip_indexed_project's step 2) and thin. Per vertex x (all V of them, used by a face or not):
 *   a NaN or infinite coordinate: SKIPPED. Otherwise g_k = sdf(x + h e_k) - sdf(x - h e_k), k = x, y, z (six evaluations;
 *   gsdf_hip_normals3's points and subtraction); s = (g.x g.x + g.y g.y) + g.z g.z; if NOT (s > 0): status FLAT. len = sqrt(s);
 *   r = (-(g.x / len), -(g.y / len), -(g.z / len)); o = x; then the march above from t0. The caller picks t0 > tol so that the march
 *   does not stop on the wall it starts from. thickness[v] is t for HIT and CROSSED, +Inf for MISS and the quiet NaN 0x7fc00000
 *   otherwise. The same limits as gsdf_hip_indexed_project (80 slots; a program on another device: GSDF_ERR_BAD_ARGUMENT; 2-D:
 *   GSDF_ERR_DIMENSION). Both outputs NULL with st != NULL is the DRY report; all three NULL: GSDF_ERR_BAD_ARGUMENT.
 * Not done here: sphere-definition (medial) thickness, rays against meshes, 2-D rays, the normal at the hit (run gsdf_hip_normals3 on
 *   pos(t)), interval-guarded marching that would make the query a guarantee, sorting rays for coherence. */
enum { GSDF_RAY_SKIPPED = 0, GSDF_RAY_HIT = 1, GSDF_RAY_CROSSED = 2, GSDF_RAY_MISS = 3, GSDF_RAY_STEPS = 4, GSDF_RAY_NONFINITE = 5,
       GSDF_RAY_FLAT = 6 };
typedef struct gsdf_ray_opts {
  float t0;           /* where the march starts; finite, >= 0 */
  float tmax;         /* a step that would pass it is a MISS; >= t0, +Inf allowed */
  float tol;          /* a ray has hit when NOT (|d| > tol); finite, >= 0 */
  float min_step;     /* no step is shorter; finite, >= 0 */
  int32_t max_steps;  /* march evaluations per ray, 1 .. 4096 */
  int32_t refine;     /* bisections of a crossing's bracket, 0 .. 32 */
  uint32_t flags;     /* 0; others refused */
  uint32_t reserved;  /* 0; others refused */
} gsdf_ray_opts;
GSDF_ABI_ASSERT(sizeof(gsdf_ray_opts) == 32, "gsdf_ray_opts is 32 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_ray_opts, tmax) == 4 && offsetof(gsdf_ray_opts, tol) == 8 && offsetof(gsdf_ray_opts, min_step) == 12 && offsetof(gsdf_ray_opts, max_steps) == 16 && offsetof(gsdf_ray_opts, refine) == 20 && offsetof(gsdf_ray_opts, flags) == 24, "gsdf_ray_opts fields");
typedef struct gsdf_thickness_opts {
  gsdf_ray_opts ray;
  float step;            /* central-difference step, > 0 and finite: h = step / 2 */
  float thin;            /* st->below counts the vertices thinner than this */
  uint32_t reserved[2];  /* 0; others refused */
} gsdf_thickness_opts;
GSDF_ABI_ASSERT(sizeof(gsdf_thickness_opts) == 48, "gsdf_thickness_opts is 48 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_thickness_opts, step) == 32 && offsetof(gsdf_thickness_opts, thin) == 36, "gsdf_thickness_opts fields");
typedef struct gsdf_ray_stats {
  uint64_t n;
  uint64_t count[8];   /* rays per status */
  uint64_t evals;
  uint32_t steps_max;
  float t_min, t_max;  /* over the HIT and CROSSED rays; +Inf and 0 when there is none */
  uint32_t reserved;
  uint64_t below;      /* HIT and CROSSED rays with t < thin */
  double ms_device;    /* device time of the kernel, HIP events */
} gsdf_ray_stats;
GSDF_ABI_ASSERT(sizeof(gsdf_ray_stats) == 112, "gsdf_ray_stats is 112 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_ray_stats, count) == 8 && offsetof(gsdf_ray_stats, evals) == 72 && offsetof(gsdf_ray_stats, steps_max) == 80 && offsetof(gsdf_ray_stats, t_min) == 84, "gsdf_ray_stats counts");
GSDF_ABI_ASSERT(offsetof(gsdf_ray_stats, t_max) == 88 && offsetof(gsdf_ray_stats, below) == 96 && offsetof(gsdf_ray_stats, ms_device) == 104, "gsdf_ray_stats extremes and cost");
int gsdf_hip_raycast3(gsdf_program* p, const float* rays, size_t n, const gsdf_ray_opts* o, float thin, float* t_out, float* d_out, uint8_t* status_out, uint16_t* steps_out, gsdf_ray_stats* st);
int gsdf_hip_indexed_thickness(gsdf_indexed* ix, gsdf_program* p, const gsdf_thickness_opts* o, float* thickness_out, uint8_t* status_out, gsdf_ray_stats* st);

/* ---- indexed meshes: dual contouring (no reference counterpart: the reference's dual-contouring mesh is a triangle list too) -------
 *
 * Dual contouring is the one mesher here whose native output IS an indexed mesh: one vertex per kept cube, one quad per active
 * lattice edge. gsdf_hip_mesh_dualcontour_indexed runs the stages of gsdf_hip_mesh_dualcontour up to the vertex placement and then,
 * instead of copying the quads' corners into a soup, hands out the cubes' indices as an ordinary gsdf_indexed handle: every accessor
 * and pass above works on it unchanged (counts, read, normals, PLY, report, shells, extract, simplify, project). Same arguments
 * and the same checks as gsdf_hip_mesh_dualcontour (2-D program: GSDF_ERR_DIMENSION; bad res or more than 12 levels:
 * GSDF_ERR_RESOLUTION; an octree mesh of the program in flight: GSDF_ERR_BAD_ARGUMENT); unsharded only.
 *
 * Quads. Those of glrender/dual_contour.go:143-219 (oracle/orc_render.c: orc_render_dualcontour restates them): a kept cube
 *   (x, y, z) whose edge from its origin along axis a (0 x, 1 y, 2 z) is ACTIVE -- the sign bit of the distance at the edge's end
 *   differs from that of the distance at the origin -- yields a quad if the four cubes of EdgeNeighborsX/Y/Z (:271-287) around that
 *   edge are all kept: q0 .. q3 in that order, reversed (q3, q2, q1, q0) when d_end - d_origin < 0.
 * Order. Quads are ordered by (z, y, x, a), increasing: the order the reference emits them in. Quad g is the faces
 *   2 g = (q0, q1, q2) and 2 g + 1 = (q2, q3, q0). Slot s = 3 t + c is corner c of face t, as in the weld. The order is part of the
 *   contract, not an accident of scheduling.
 * Key. The key of a slot is its cube: ix | iy << 20 | iz << 40 | 5 << 60, the cube's lattice coordinates (0 .. 2^(levels-1) - 1).
 *   Kind 5, after the weld's 0 .. 3 and the simplifier's 4; its top bits are 0101, so it is never the tables' empty value.
 * Vertices. A vertex is the set of slots with one key. Vertices are numbered by the smallest slot that names them, in increasing
 *   order (the weld's and extract's rule); a vertex's position is the cube's placed vertex, bit for bit -- the value every copy of it
 *   has in gsdf_hip_mesh_dualcontour's soup -- and keys[v] is the cube's key. has_normals == 0. A kept cube that no quad names is
 *   not a vertex.
 * Faces. F = 2 x quads; idx[s] is the number of slot s's vertex. All faces are kept, degenerate ones included. verts[idx] is the
 *   reference's triangle list in the reference's order.
 * Determinism. The result is a function of the program, res and chiseled alone, to the byte: it does not depend on the order in
 *   which threads arrive, on the capacity-retry loop, or on whether the interpreter or the per-tree kernels evaluated.
 * Errors. 3 F >= 2^32: GSDF_ERR_CAPACITY. No quad: GSDF_ERR_EMPTY_BUFFERS.
 * st (optional): what gsdf_hip_mesh_dualcontour reports for the same call -- n_tris, evals, leaf_cubes, active_leaves, levels,
 *   origin, res, ms_total. Here ms_total runs from the first stage to the end of the ordering of the quads and is NOT pure device time,
 *   unlike gsdf_hip_mesh_dualcontour's: the ordering waits once for the host in its middle (the quad count comes back with the
 *   counters and sizes the index array), and that wait is inside the interval. The numbering follows it and is the handle's
 *   ms_number; ms_keys and ms_number are device time alone. The handle's gsdf_indexed_stats: ms_keys = the ordering of the
 *   quads, ms_number = owners, numbering, position gather and index write; ms_insert = 0, probes = table_cells = 0, attempts = 0
 *   (there is no hash table: a cube's index is its vertex's identity).
 * Workspace. Beside dual contouring's own, the program handle keeps (grow-only, like the rest) 60 bytes per cube of LIST CAPACITY
 *   (20 per possible edge: a quad's four cubes and its place) + 8 bytes per lattice row (n^2) + 8 per quad of the last mesh: 63 MB at
 *   the smallest capacity (2^20 cubes), 0.76 GB for a first mesh at 11 levels (12 n^2 cubes), 3 GB at 12. The soup's triangle
 *   buffer (216 bytes per cube of capacity) is not allocated by this entry.
 * The result is finished inside the call (the cubes and their vertices live in the program handle's workspace, which the next mesh
 * overwrites) and independent of the program afterwards. Kernels: gsdf_amd/csrc/kernels_dc_indexed.h (abi_mesh.hip) and
 * kernels_topo.h: cube_first_kernel, cube_number_kernel (abi_indexed.hip); a numpy restatement: tests/dcref.py. */
int gsdf_hip_mesh_dualcontour_indexed(gsdf_program* p, float res, int chiseled, void* stream, gsdf_indexed** out, gsdf_mesh_stats* st /* optional */);

/* ---- contours: a 2-D part's outline and a 3-D part's z-slices as ordered closed loops (no reference counterpart: the reference's
 * only 2-D output is a picture) ---------------------------------------------------------------------------------------------------
 *
 * gsdf_hip_contour2 traces the zero set of a 2-D program on a square lattice of spacing res; gsdf_hip_slice3 does the same for a 3-D
 * program in the planes z = z[k], one LAYER per z, each traced independently of the others on the same xy lattice. The result is a
 * gsdf_contour handle: closed polygons (loops) whose vertices lie on lattice edges, each loop in order of travel with the part on its
 * left (outer boundaries counter-clockwise, holes clockwise). All arithmetic below is float32, every operation rounded once (fl), never
 * fused; the result is a function of the program, res and the z list alone, to the byte -- not of thread order, of the chunking
 * (max_nodes) or of whether the interpreter or the per-tree kernels evaluated.
 *
 * Lattice. bb = the program's bounds. x0 = fl(bb.min.x - res); nx = int(floor(fl(fl(bb.max.x - bb.min.x) / res))) + 4;
 *   x_i = fl(x0 + fl(float(i) res)), i = 0 .. nx - 1; y likewise. The last node lies more than res beyond bb.max: a full ring of
 *   cells outside the bounds on every side. A box that is empty or inverted along an axis (size 0 or the quotient not >= 0) has
 *   4 nodes along it: no loops, no error. GSDF_ERR_BAD_ARGUMENT: res not finite or <= 0, x or y bounds not finite,
 *   a quotient >= 2^31, nx ny >= 2^31 -- all refused before anything is allocated. Node (i, j) of layer k is evaluated at
 *   (x_i, y_j) or (x_i, y_j, z[k]) by the program's ordinary Evaluate: d.
 * Inside. A node is inside iff d < 0 and it is not on the lattice border (i = 0, nx - 1 or j = 0, ny - 1). NaN and both zeros are
 *   outside; -Inf is inside. A border node with d < 0 is forced outside and counted in border_inside: every loop closes, whatever the
 *   field does. nonfinite_nodes counts the nodes (border included) whose d is NaN or +-Inf.
 * Vertices. A lattice edge is cut iff its two nodes differ in the inside test. Its key is 2 (j nx + i) + axis, (i, j) its lower node,
 *   axis 0 along x, 1 along y. With d_lo, d_hi the distances at the lower and the higher node: t = fl(d_lo / fl(d_lo - d_hi)) if both
 *   are finite and the OUTSIDE node has d >= 0 (it has not where the border rule forced it outside), else t = 0.5. The division is the
 *   correctly rounded one. The cut coordinate is fl(c_lo + fl(t res)), c_lo the lower node's; the other coordinate is the node's own.
 * Segments. A cell (i, j), i < nx - 1, j < ny - 1, has corners c0 (i, j), c1 (i+1, j), c2 (i+1, j+1), c3 (i, j+1), case = the sum of
 *   2^c over its inside corners, and edges B (bottom, key(i, j, 0)), R (key(i+1, j, 1)), T (key(i, j+1, 0)), L (key(i, j, 1)).
 *   Oriented segments tail -> head, the part on the left:  1 B>L  2 R>B  3 R>L  4 T>R  6 T>B  7 T>L  8 L>T  9 B>T  11 R>T  12 L>R
 *   13 B>R  14 L>B;  the saddles 5: B>L and T>R, 10: R>B and L>T (the two inside corners are never joined: a fixed rule, no extra
 *   evaluation; saddle_cells counts them);  0 and 15: none. Every cut edge is the tail of exactly one segment and the head of exactly
 *   one: succ (tail -> head) is a permutation of the cut edges of a layer and its cycles are the loops.
 * Order. A loop's leader is its smallest key. Loops are ordered by (layer, leader), increasing; a loop's vertices start at its leader
 *   and follow succ. (A leader is always an axis-1 edge.) loop_start[q] is the first vertex of loop q, loop_start[n_loops] = n_verts;
 *   loop_layer[q] its layer (an index into z; 0 for gsdf_hip_contour2); keys[v] the edge key of vertex v within its layer;
 *   xy[2 v], xy[2 v + 1] its coordinates. Areas are the caller's (a shoelace sum over this order); not part of the contract.
 * Chunks. The layers are evaluated and traced in chunks of whole layers of at most max_nodes lattice nodes (0: the default below;
 *   always at least one layer), so that a tall stack does not hold every layer's workspace (24 bytes per node) at once. The result
 *   and the integer statistics do not depend on it.
 * Statistics. rank_rounds = ceil(log2(the largest number of vertices in one layer)) (0 for none): the rounds of pointer jumping that
 *   layer needs, once for the leaders and once for the ranks; a chunk runs the rounds of its own largest layer, one launch per round,
 *   no host round trip inside. evals = nx ny n_layers, by which the program's evaluation count grows. ms_eval = device time of the
 *   lattice positions and the Evaluate, ms_trace = device time of everything behind it (intervals between the host's waits, which
 *   are left out), ms_device = their sum. Bytes 0 .. 63 of the record are a function of the inputs alone.
 * Errors. GSDF_ERR_DIMENSION: gsdf_hip_contour2 on a 3-D program, gsdf_hip_slice3 on a 2-D one. GSDF_ERR_BAD_ARGUMENT: the lattice
 *   rules above, n_z == 0, a null z. GSDF_ERR_CAPACITY: 2^32 vertices or more. Blocking; the handle is independent of the program
 *   afterwards. Out of scope: DXF / G-code, arc fitting, tool offsets inside the tracer (Offset2D in the tree is exact for a 2-D
 *   program; in-plane offsets of any handle: "contours: offset" below), sharded or gathered contours, a fused lattice kernel,
 *   asymptotic-decider saddles. (Simplification and the loops' areas on the device: the next section; infill: "contours: hatch
 *   fill" below.)
 * Kernels: gsdf_amd/csrc/kernels_contour.h (abi_contour.hip); a numpy restatement over the oracle: tests/contourref.py. */
typedef struct gsdf_contour gsdf_contour; /* loops, resident in HBM */
#define GSDF_CONTOUR_DEFAULT_MAX_NODES 16777216 /* 2^24 nodes: 0.4 GB of workspace */
typedef struct gsdf_contour_opts {
  uint64_t max_nodes; /* lattice nodes per chunk of whole layers; 0 = GSDF_CONTOUR_DEFAULT_MAX_NODES */
} gsdf_contour_opts;
typedef struct gsdf_contour_stats {
  uint64_t n_verts, n_loops, border_inside, nonfinite_nodes, saddle_cells, evals;
  uint32_t nx, ny, n_layers, rank_rounds;
  double ms_device, ms_eval, ms_trace;
} gsdf_contour_stats;
int gsdf_hip_contour2(gsdf_program* p2d, float res, const gsdf_contour_opts* o /* optional */, gsdf_contour** out);
int gsdf_hip_slice3(gsdf_program* p3d, float res, const float* z, uint32_t n_z, const gsdf_contour_opts* o /* optional */, gsdf_contour** out);
int gsdf_hip_contour_counts(const gsdf_contour* c, uint32_t* n_layers, uint64_t* n_loops, uint64_t* n_verts); /* each optional */
/* xy 2 n_verts floats, keys n_verts, loop_start n_loops + 1, loop_layer n_loops; any pointer may be NULL */
int gsdf_hip_contour_read(const gsdf_contour* c, float* xy, uint32_t* keys, uint32_t* loop_start, uint32_t* loop_layer);
int gsdf_hip_contour_stats_get(const gsdf_contour* c, gsdf_contour_stats* st);
void gsdf_hip_contour_destroy(gsdf_contour* c);

/* ---- contours: simplify and measures (no reference counterpart) -------------------------------------------------------------------
 *
 * The tracer returns one vertex per cut lattice edge: a straight side is hundreds of collinear points. What a cutter or a slicer asks
 * of loops before it takes them: fewer vertices within a stated deviation, and each loop's area, length and box. All of it runs on the
 * device, on any gsdf_contour handle (traced, uploaded or simplified), and is a function of the handle's arrays and the options alone,
 * to the byte: NOT of the order in which threads arrive. Kernels: gsdf_amd/csrc/kernels_contour_simplify.h (abi_contour.hip); a numpy
 * restatement: tests/contoursimpref.py.
 *
 * gsdf_hip_contour_create uploads host loops (an SVG read back, or any polygons): xy 2 n_verts floats, loop_start n_loops + 1 (loop q
 *   is the vertices loop_start[q] .. loop_start[q + 1] - 1, in order), loop_layer n_loops or NULL (all 0), keys n_verts or NULL (then
 *   they read back as 0). The device of the calling thread (gsdf_hip_init). GSDF_ERR_BAD_ARGUMENT, refused before anything is
 *   allocated, the text names the loop or the vertex: loop_start[0] != 0; loop_start[n_loops] != n_verts; a loop of fewer than 3
 *   vertices; loop_layer decreasing, or >= n_layers (so n_layers == 0); a NaN or infinite coordinate. n_loops == 0 or n_verts == 0:
 *   GSDF_ERR_EMPTY_BUFFERS; n_verts >= 2^32: GSDF_ERR_CAPACITY. Every accessor above works on the result; its gsdf_contour_stats has
 *   n_verts, n_loops and n_layers set, every other integer 0, the times 0. The same holds for a handle gsdf_hip_contour_simplify made.
 *   Every coordinate of every handle is finite (the tracer makes no other, this call takes no other).
 *
 * gsdf_hip_contour_simplify: dyadic chord simplification. tol in the coordinates' unit, levels 1 .. 16 (0: 8), passes 1 .. 8 (0: 1).
 * One pass, per loop. The loop's vertices are p_0 .. p_(n-1), p_0 its leader (first vertex); read it as the open polyline p_0 .. p_n
 *   with p_n = p_0. kmax = the largest k <= levels with 3 2^k <= n (0 for n < 6: such a loop is unchanged). For k = 1 .. kmax and
 *   m = 0, 1, ..., the SPAN (k, m) runs from s = m 2^k to e = min(s + 2^k, n); a span with e - s < 2 has no interior and does not
 *   count. A span is ACCEPTABLE iff every interior vertex p_j (s < j < e) has q2(p_s, p_e, p_j) <= tol2, tol2 = (double)tol (double)tol.
 * The distance q2(a, b, p): every coordinate taken as (double)float32 (exact); every operation below is one IEEE float64 operation,
 *   in this order, none contracted (the library is built with -ffp-contract=off):
 *     u = b - a;  dd = u.x u.x + u.y u.y;  w = p - a;  t = w.x u.x + w.y u.y
 *     if dd == 0 or t <= 0:  q2 = w.x w.x + w.y w.y
 *     else if t >= dd:       v = p - b,  q2 = v.x v.x + v.y v.y
 *     else:                  cr = w.x u.y - w.y u.x,  q2 = (cr cr) / dd
 *   the squared distance of p to the SEGMENT a b (not to the line). A comparison with a NaN is false (no finite input makes one).
 * Dropping and keeping. Vertex j is DROPPED iff it is interior to some acceptable span of its loop; every other vertex is KEPT. The
 *   output has the same loops, in the same order and in the same layers, each its kept vertices in order, their coordinate bits and
 *   keys carried over; loop_start is recomputed. Position 0 is interior to no span: leaders stay, and so does the loop order.
 * Guarantees (derived; tests/test_contour_simplify_ref.py holds the restatement to them). Vertices m 2^kmax are interior to no span:
 *   every loop keeps at least ceil(n / 2^kmax) >= 3 vertices. Dyadic spans nest (two of them are disjoint inside or one holds the
 *   other), so the kept neighbours of a dropped vertex are exactly the ends of the MAXIMAL acceptable span around it (the acceptable
 *   span no acceptable span contains), and the vertex lies within tol of the segment that replaces it. The tol-neighbourhood of a
 *   segment is convex: the Hausdorff distance between the old and the new loop is <= tol both ways, and |area change| <= tol x (old
 *   perimeter). Raising tol or levels only drops more vertices.
 * passes repeats the rule on the previous pass's result with the same tol; the deviations add: <= passes tol to the original. A second
 *   pass removes what the dyadic alignment keeps (a rectangle with 37 and 41 collinear vertices per side, 156 in all, keeps 19
 *   after one pass at tol 0, 10 after two, 6 after three).
 * NOT promised: that the result is free of self-intersections; that two loops closer than 2 tol stay apart. Out of scope: arc
 *   fitting, DXF / G-code, optimal (Douglas-Peucker / Imai-Iri) vertex counts.
 * Statistics. Bytes 0 .. 183 (n_verts_in .. max_dev) are a function of the inputs alone: n_verts_out of the last pass; loops_changed
 *   = loops that lost a vertex, summed over passes; spans[k] = maximal acceptable spans of level k, summed over passes; max_level =
 *   the largest k with spans[k] > 0 (0: none); max_dev = the correctly rounded float64 square root of the largest q2 of any dropped
 *   vertex against the chord of its maximal span, over all passes (on the device an unsigned 64-bit maximum over the bit patterns
 *   of non-negative doubles, as the adaptive simplification's max_err), 0 if nothing was dropped. ms_device: HIP events around the
 *   kernels of every pass (the host's waits between them left out).
 * dry != 0 fills the statistics and builds no handle: out may be NULL, and is set to NULL if it is not.
 * Errors. GSDF_ERR_BAD_ARGUMENT: tol NaN or < 0 (+Inf is allowed: every span is acceptable); levels > 16; passes > 8; out NULL
 *   without dry. A handle without loops gives a handle without loops.
 *
 * gsdf_hip_contour_measures: per loop (loops: n_loops records, loop order, or NULL) and per layer (layers: n_layers records, or NULL)
 *   the signed area (the part on the left: outer boundaries > 0, holes < 0), the length and the box, order-independent to the bit by
 *   the scheme of "report and extract" above. e = the smallest integer >= -125 with |x| < 2^e for every coordinate of the handle (from
 *   the largest |bits|: e = max(biased exponent, 1) - 126). Per vertex j of a loop, with its successor j+1 (the leader behind the last),
 *   coordinates as (double)float32, one IEEE float64 operation each, none contracted:
 *     area term   = x_j y_(j+1) - x_(j+1) y_j       (both products are exact: 24 x 24 bits; ONE rounded subtraction)
 *     length term = sqrt(dx dx + dy dy), dx = x_(j+1) - x_j, dy likewise   (correctly rounded square root)
 *   |area term| < 2^(2e+1) and length term < 2^(e+3/2) (|dx|, |dy| < 2^(e+1)). Each term is multiplied by the power of two 2^(61-2e)
 *   resp. 2^(60-e) (exact), rounded to the nearest integer, ties to even: |q| < 2^62 resp. < 2^61.5. The q are summed as INTEGERS
 *   (on the device: q's low 32 bits and its arithmetic-shifted rest in separate 64-bit words, which the 2^32 vertices a handle can
 *   hold cannot overflow). The result is that integer converted to float64 with ONE rounding (to nearest even) times the inverse
 *   power of two (exact: never subnormal); area = that / 2 (exact). A layer's sums are the integer sums of its loops, converted
 *   likewise. bbox = min x, min y, max x, max y of the vertices, compared as order-preserving float32 bits (-0 below +0); a layer
 *   without a loop has min = +inf, max = -inf, sums 0. Error of the quantisation: at most n / 2 units of 2^(2e-62) for the area of
 *   n vertices, i.e. n 2^-65 of the square [-2^e, 2^e]^2 that holds them, and n / 2 units of 2^(e-60) for the length: far below what
 *   float32 coordinates carry. Derived, not measured. gsdf_hip_contour_measures_ms: the device time (HIP events) of the calling
 *   thread's last gsdf_hip_contour_measures, 0 before the first. */
typedef struct gsdf_contour_simplify_opts {
  float tol;       /* >= 0, +Inf allowed */
  uint32_t levels; /* 1 .. 16; 0 = 8 */
  uint32_t passes; /* 1 .. 8; 0 = 1 */
  uint32_t dry;    /* non-zero: statistics only */
} gsdf_contour_simplify_opts;
GSDF_ABI_ASSERT(sizeof(gsdf_contour_simplify_opts) == 16, "gsdf_contour_simplify_opts is 16 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_contour_simplify_opts, levels) == 4 && offsetof(gsdf_contour_simplify_opts, passes) == 8 && offsetof(gsdf_contour_simplify_opts, dry) == 12, "gsdf_contour_simplify_opts fields");
typedef struct gsdf_contour_simplify_stats {
  uint64_t n_verts_in, n_verts_out, n_loops, loops_changed;
  uint64_t spans[17]; /* [k]: maximal acceptable spans of level k ([0] stays 0) */
  uint32_t max_level, reserved;
  double max_dev;
  double ms_device;
} gsdf_contour_simplify_stats;
GSDF_ABI_ASSERT(sizeof(gsdf_contour_simplify_stats) == 192, "gsdf_contour_simplify_stats is 192 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_contour_simplify_stats, n_loops) == 16 && offsetof(gsdf_contour_simplify_stats, spans) == 32 && offsetof(gsdf_contour_simplify_stats, max_level) == 168, "gsdf_contour_simplify_stats counts");
GSDF_ABI_ASSERT(offsetof(gsdf_contour_simplify_stats, max_dev) == 176 && offsetof(gsdf_contour_simplify_stats, ms_device) == 184, "gsdf_contour_simplify_stats deviation and cost");
typedef struct gsdf_loop_measure {
  double area, length;
  float bbox[4]; /* min x y, max x y */
  uint32_t n_verts, layer;
} gsdf_loop_measure;
GSDF_ABI_ASSERT(sizeof(gsdf_loop_measure) == 40, "gsdf_loop_measure is 40 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_loop_measure, length) == 8 && offsetof(gsdf_loop_measure, bbox) == 16 && offsetof(gsdf_loop_measure, n_verts) == 32 && offsetof(gsdf_loop_measure, layer) == 36, "gsdf_loop_measure fields");
typedef struct gsdf_layer_measure {
  double area, length;
  float bbox[4];
  uint32_t n_loops, n_verts;
} gsdf_layer_measure;
GSDF_ABI_ASSERT(sizeof(gsdf_layer_measure) == 40, "gsdf_layer_measure is 40 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_layer_measure, length) == 8 && offsetof(gsdf_layer_measure, bbox) == 16 && offsetof(gsdf_layer_measure, n_loops) == 32 && offsetof(gsdf_layer_measure, n_verts) == 36, "gsdf_layer_measure fields");
int gsdf_hip_contour_create(const float* xy, uint64_t n_verts, const uint32_t* loop_start, uint64_t n_loops, const uint32_t* loop_layer /* NULL: all 0 */,
                            uint32_t n_layers, const uint32_t* keys /* NULL: read back as 0 */, gsdf_contour** out);
int gsdf_hip_contour_simplify(const gsdf_contour* c, const gsdf_contour_simplify_opts* o, gsdf_contour** out /* NULL allowed iff dry */,
                              gsdf_contour_simplify_stats* st /* optional */);
int gsdf_hip_contour_measures(const gsdf_contour* c, gsdf_loop_measure* loops /* n_loops or NULL */, gsdf_layer_measure* layers /* n_layers or NULL */);
double gsdf_hip_contour_measures_ms(void);

/* ---- contours: section properties (no reference counterpart) -----------------------------------------------------------------------
 *
 * What a beam calculation asks of a cross-section: its centroid and its second moments of area, per loop and per layer, by the
 * scheme of gsdf_hip_contour_measures above and with its exponent e. Kernel: gsdf_amd/csrc/kernels_mass.h (abi_contour.hip); host
 * arithmetic: gsdf_amd/csrc/mass_host.h; restated in tests/massref.py.
 *
 * Terms, per vertex j of a loop with its successor j+1 (the leader behind the last), coordinates as (double)float32, one IEEE
 *   float64 operation each, none contracted; cross = x_j y_(j+1) - x_(j+1) y_j is the measures' area term:
 *     first_x term = (cross * (x_j + x_(j+1))) / 6                                  and first_y likewise with y
 *     xx term      = (cross * (((x_j x_j) + (x_j x_(j+1))) + (x_(j+1) x_(j+1)))) / 12     and yy likewise with y
 *     xy term      = (cross * ((((x_j y_(j+1)) + (x_(j+1) y_j)) + 2 (x_j y_j)) + 2 (x_(j+1) y_(j+1)))) / 24
 *   (2 (u v): the product, then doubled; every product of two coordinates is exact.) first_x is the integral of x over the part on
 *   the left of the loop, xx of x^2, yy of y^2, xy of x y. The signs follow the area's: a hole's sums are negative, so a layer's
 *   sums are those of the material.
 * Bounds (derived). |cross| < 2^(2e+1); |x_j + x_(j+1)| < 2^(e+1): |first term| < 2^(3e+2) / 6 < 2^(3e), scale 2^(62-3e). The
 *   brackets of xx and yy are < 3 2^(2e), that of xy < 6 2^(2e): |second term| < 2^(4e-1), scale 2^(62-4e). Scaled (exact), rounded
 *   to the nearest integer, ties to even, |q| < 2^62, summed as integers as the measures' terms are, converted with ONE rounding,
 *   times the inverse power of two (exact). A layer's integers are the sums of its loops' integers. Error of the quantisation: at
 *   most n / 2 units of 2^(3e-62) resp. 2^(4e-62) for n vertices.
 * The record. area has the bytes of gsdf_hip_contour_measures' area; first = (x, y); second = (xx, yy, xy), about the origin. Derived
 *   on the host, one float64 operation each, in this order:
 *     centroid_k = first_k / area
 *     central    = (xx - ((first_x * first_x) / area), yy - ((first_y * first_y) / area), xy - ((first_x * first_y) / area))
 *   With area == 0 (a layer without a loop among them) centroid and central are the quiet NaN 0x7ff8000000000000. central cancels
 *   for a section far from the origin, as the inertia of a mesh does. n_verts: the loop's, or the layer's; layer_or_n_loops: the
 *   loop's layer in a loop record, the number of loops in a layer record.
 * gsdf_hip_contour_sections: loops (n_loops records, loop order) and layers (n_layers records), either may be NULL.
 *   gsdf_hip_contour_sections_ms: the device time (HIP events) of the calling thread's last gsdf_hip_contour_sections, 0 before the
 *   first. */
typedef struct gsdf_section {
  double area, first[2], second[3];  /* second: xx yy xy, about the origin */
  double centroid[2], central[3];    /* central: xx yy xy, about the centroid */
  uint32_t n_verts, layer_or_n_loops;
} gsdf_section;
GSDF_ABI_ASSERT(sizeof(gsdf_section) == 96, "gsdf_section is 96 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_section, first) == 8 && offsetof(gsdf_section, second) == 24 && offsetof(gsdf_section, centroid) == 48, "gsdf_section sums");
GSDF_ABI_ASSERT(offsetof(gsdf_section, central) == 64 && offsetof(gsdf_section, n_verts) == 88 && offsetof(gsdf_section, layer_or_n_loops) == 92, "gsdf_section derived values");
int gsdf_hip_contour_sections(const gsdf_contour* c, gsdf_section* loops /* n_loops or NULL */, gsdf_section* layers /* n_layers or NULL */);
double gsdf_hip_contour_sections_ms(void);

/* ---- contours: hatch fill (no reference counterpart) ---------------------------------------------------------------------------------
 *
 * The step between closed loops and something a printer, a laser or a plotter can follow: for every layer of a gsdf_contour handle
 * (traced, uploaded or simplified), the segments of a family of parallel lines that lie inside the material. All of it runs on the
 * device and is a function of the handle's arrays and the options alone, to the byte: NOT of the order in which threads arrive.
 * Kernels: gsdf_amd/csrc/kernels_hatch.h (abi_contour.hip); a numpy restatement: tests/hatchref.py.
 *
 * Coordinates are taken as (double)float32 (exact), so are spacing, offset and dir. Every operation below is one IEEE float64
 *   operation, in the order written, none contracted (the library is built with -ffp-contract=off).
 * Vertex values. (dx, dy) = dir[l % n_dirs] is the direction of the vertex's layer l.
 *     s = ((-dy) x) + (dx y)        u = (dx x) + (dy y)
 *   All four products are exact (24 x 24 bits): one rounded addition each. s is the coordinate across the lines, u along them.
 * Lines. Line k (an integer) of a layer is the set s = c_k, c_k = offset + ((double)k spacing). The product is exact while
 *   |k| < 2^29; the addition's rounding is monotone, so c_k is non-decreasing in k. With a unit dir neighbouring lines are spacing apart.
 * Crossings. The edge from vertex j to its successor in the loop (the leader follows the last vertex), a and b, crosses line k iff
 *     (s_a < c_k) != (s_b < c_k)
 *   A vertex exactly on a line counts as above it; an edge lying on a line does not cross it; every closed loop crosses every line an
 *   even number of times (the predicate is a function of the vertex alone, and a closed walk changes sides an even number of times).
 *     t   = (c_k - s_a) / (s_b - s_a)      (the divisor is not 0 at a crossing; 0 <= t <= 1; -0.0 occurs and is allowed)
 *     u_c = u_a + (t (u_b - u_a))
 *     x_c = (float)(x_a + (t (x_b - x_a)))   and y_c likewise: float64 arithmetic, rounded once to float32
 *   How the candidate k of an edge are found is the implementation's business (here: floor((s - offset) / spacing), corrected with
 *   the predicate); the predicate alone is the contract.
 * Segments. The crossings of one (layer, k) are ordered by (u_c, j), increasing: u_c compared as doubles (-0 == +0), j, the global
 *   vertex number of the edge's tail, breaks ties (an edge crosses a line once: the order is total). Consecutive pairs (0, 1),
 *   (2, 3), ... are the segments: the even-odd rule, which is the material for the tracer's loops (outer boundaries counter-clockwise,
 *   holes clockwise, properly nested). A segment runs from the lower to the higher u_c (x0 y0, then x1 y1). Segments are ordered by
 *   (layer, k, position); layer_start[l] is the first segment of layer l, layer_start[n_layers] = n_segments. Nothing is dropped:
 *   zero_length counts the segments whose two float32 end points are equal bit for bit.
 * Lengths. A segment's term is u_c1 - u_c0, in units of |dir|. Bound (derived): with e the handle's exponent as in
 *   gsdf_hip_contour_measures, |x|, |y| <= 2^e (1 - 2^-24) and |dx|, |dy| <= 1, so |s|, |u| <= 2^(e+1) (1 - 2^-24) before and after
 *   their one rounding; t lies in [0, 1], so |u_c| < 2^(e+1) (1 + 2^-50) and |term| < 2^(e+2) (1 + 2^-50). Scaled by 2^(58-e)
 *   (exact) the term is below 2^60 (1 + 2^-50): inside the |q| <= 2^62 the measures' scheme needs, with room to spare, so the
 *   exponent stays 58 - e. Rounded to the nearest integer, ties to even, summed as INTEGERS (on the device: the low 32 bits and the
 *   arithmetic-shifted rest in separate 64-bit words, which 2^31 segments cannot overflow), converted to float64 with ONE rounding,
 *   times 2^(e-58) (exact). Error of the quantisation: at most n / 2 units of 2^(e-58) for n segments.
 *   gsdf_hatch_layer: the layer's length, its n_segments, k_min and k_max = the smallest and the largest k with a crossing; a layer
 *   without one has k_min = 0, k_max = -1, length 0. The statistics' length is the sum of the layers' integers, converted likewise.
 * Statistics. Everything before ms_device is a function of the inputs alone. n_crossings = 2 n_segments; n_lines = the (layer, k)
 *   with a crossing; max_line_crossings = the most crossings on one of them: the rank pass compares every crossing of a line with
 *   every other one, so its cost grows with the square of this number. ms_device: HIP events around the kernels (the host's waits
 *   between them left out). gsdf_hip_hatch_rank_ms: of that, the rank pass of the calling thread's last gsdf_hip_contour_hatch.
 * dry != 0 fills the statistics and builds no handle: out may be NULL, and is set to NULL if it is not.
 * Errors. GSDF_ERR_BAD_ARGUMENT: spacing not finite or <= 0; offset not finite; n_dirs 0 or > 4; a dir (of the first n_dirs) with a
 *   non-finite component, |dx| or |dy| > 1, or both 0; out NULL without dry; (2^(e+1) + |offset|) / spacing >= 2^29, decided on the
 *   host in float64 before any workspace but the exponent's one word is allocated: the text says that spacing is too small for these
 *   coordinates. (|s| < 2^(e+1): every k that can cross has |k| < 2^29 + 2, and its product with spacing is exact.) GSDF_ERR_CAPACITY:
 *   2^32 crossings or more, or 2^31 line slots (the sum over the layers of k_max - k_min + 1) or more. A handle without loops gives
 *   a handle without segments and no error. Blocking; the result is independent of c afterwards.
 * Out of scope: joining segments into zig-zag paths, travel ordering, concentric or gyroid patterns, dropping short segments,
 *   clipping against anything but the handle's own loops (against the neighbouring layers: the next section), a segmented sort for
 *   lines with thousands of crossings. */
typedef struct gsdf_hatch gsdf_hatch; /* segments, resident in HBM */
typedef struct gsdf_hatch_opts {
  float spacing;   /* > 0, finite */
  float offset;    /* finite */
  uint32_t n_dirs; /* 1 .. 4; layer l uses dir[l % n_dirs] */
  uint32_t dry;    /* non-zero: statistics only */
  float dir[4][2]; /* (dx, dy); both finite, |dx|, |dy| <= 1, not both 0. The caller's unit vector: float32(cos), float32(sin) */
} gsdf_hatch_opts;
GSDF_ABI_ASSERT(sizeof(gsdf_hatch_opts) == 48, "gsdf_hatch_opts is 48 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_hatch_opts, offset) == 4 && offsetof(gsdf_hatch_opts, n_dirs) == 8 && offsetof(gsdf_hatch_opts, dry) == 12 && offsetof(gsdf_hatch_opts, dir) == 16, "gsdf_hatch_opts fields");
typedef struct gsdf_hatch_layer {
  double length;
  uint64_t n_segments;
  int32_t k_min, k_max;
} gsdf_hatch_layer;
GSDF_ABI_ASSERT(sizeof(gsdf_hatch_layer) == 24, "gsdf_hatch_layer is 24 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_hatch_layer, n_segments) == 8 && offsetof(gsdf_hatch_layer, k_min) == 16 && offsetof(gsdf_hatch_layer, k_max) == 20, "gsdf_hatch_layer fields");
typedef struct gsdf_hatch_stats {
  uint64_t n_segments, n_crossings, n_lines /* (layer, k) pairs with a crossing */, max_line_crossings, zero_length;
  uint32_t n_layers, reserved;
  double length;    /* all layers */
  double ms_device; /* last: everything before it is a function of the inputs alone */
} gsdf_hatch_stats;
GSDF_ABI_ASSERT(sizeof(gsdf_hatch_stats) == 64, "gsdf_hatch_stats is 64 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_hatch_stats, zero_length) == 32 && offsetof(gsdf_hatch_stats, n_layers) == 40 && offsetof(gsdf_hatch_stats, length) == 48 && offsetof(gsdf_hatch_stats, ms_device) == 56, "gsdf_hatch_stats fields");
int gsdf_hip_contour_hatch(const gsdf_contour* c, const gsdf_hatch_opts* o, gsdf_hatch** out /* NULL allowed iff dry */, gsdf_hatch_stats* st /* optional */);
int gsdf_hip_hatch_counts(const gsdf_hatch* h, uint32_t* n_layers, uint64_t* n_segments); /* each optional */
/* seg 4 n_segments floats (x0 y0 x1 y1), line n_segments (k), layer_start n_layers + 1, layers n_layers; any pointer may be NULL */
int gsdf_hip_hatch_read(const gsdf_hatch* h, float* seg, int32_t* line, uint32_t* layer_start, gsdf_hatch_layer* layers);
double gsdf_hip_hatch_rank_ms(void);
void gsdf_hip_hatch_destroy(gsdf_hatch* h);

/* ---- contours: skin classification of the hatch (no reference counterpart) -----------------------------------------------------------
 *
 * What a layer's fill must be depends on its neighbours: where the layer above lacks material the surface is exposed (top skin),
 * where the layer below lacks it the fill hangs in the air (bottom skin: an overhang or a bridge), the rest may be filled sparsely.
 * gsdf_hip_contour_hatch_skin hatches every layer as the section above does and cuts each hatch line against the loops of the
 * `below` layers under and the `above` layers over it: the pieces carry a class, 0 inner, 1 bottom, 2 top, 3 both. On the device, a
 * function of the handle's arrays and the options alone, to the byte. Kernels: gsdf_amd/csrc/kernels_skin.h (abi_contour.hip); a
 * numpy restatement: tests/skinref.py. Every operation is one IEEE float64 operation, uncontracted; s, u, c_k, the crossing predicate,
 * t, u_c, x_c, y_c, the exponent e and the quantisation are the hatch section's, by name.
 *
 * Lines and sources. Target layer l of L uses the direction D_l = dir[l % n_dirs] and the hatch's lines c_k. Its sources are numbered
 *   r: r = 0 is layer l itself, r = i is layer l - i (i = 1 .. below), r = below + i is layer l + i (i = 1 .. above). A source whose
 *   layer index falls outside 0 .. L-1 is MISSING.
 * Crossings. Every edge of every present source layer is crossed with the lines of D_l -- s and u of its ends under the TARGET's
 *   direction, not the source layer's own -- with exactly the hatch's predicate and its formulas for t, u_c, x_c and y_c. A crossing is
 *   (l, k, r, j), j the global vertex number of the edge's tail.
 * Lines that count. Only lines (l, k) that carry at least one crossing of source 0 exist; crossings on other lines are counted
 *   nowhere. Each closed loop crosses a line an even number of times, so every source's count on a line is even.
 * Values and gaps. The distinct u_c on a line, v_0 < v_1 < ... (compared as doubles, -0 == +0). On the open gap (v_i, v_i+1) source r
 *   is PRESENT iff the number of its crossings with u_c <= v_i is odd.
 * Class of a gap. OUTSIDE if source 0 is not present. Otherwise bit 0 (value 1, bottom) is set iff below > 0 and some source
 *   1 .. below is missing or not present; bit 1 (value 2, top) iff above > 0 and some source below+1 .. below+above is missing or not
 *   present. Missing layers count as empty: the first `below` layers are bottom skin and the last `above` layers top skin throughout,
 *   as a slicer's "N solid layers" means.
 * Pieces. A maximal run of consecutive gaps of one line with the same class, not OUTSIDE, is one segment from the run's first value
 *   to its last. The float32 end points are the (x_c, y_c) of the first crossing at that value under the order (r, j): a tie between
 *   layers makes no sliver, and where an own-layer crossing has the value it decides the coordinates. Segments are ordered by (layer,
 *   k, start value); layer_start and line are the hatch's; cls[i] is 0 .. 3. Nothing is dropped: zero_length counts the pieces whose
 *   two float32 end points are equal bit for bit. (An own-layer pair of crossings with ONE value encloses no gap and makes no piece,
 *   where the hatch makes a segment of length 0; on other inputs below = above = 0 gives the hatch's segments.)
 * Lengths. A piece's term is (end value - start value), quantised with the hatch's scale 2^(58-e) -- u_c under any of the
 *   directions obeys the hatch's bound, which applies unchanged -- and summed as split integers per (layer, class).
 *   gsdf_skin_layer: the layer's length and pieces by class. The gsdf_hatch_layer of such a handle is the layer's total: the sum of
 *   the four class INTEGERS converted once, n_segments summed, k_min and k_max over the pieces (0, -1: none). stats.length[c] is the
 *   sum of the layers' integers of class c, converted likewise.
 * Statistics. Bytes 0 .. 127 are a function of the inputs alone. n_own_crossings: the crossings of source 0 (the hatch's
 *   n_crossings); n_crossings: all crossings on existing lines; n_lines: the existing lines; max_line_crossings: the most crossings,
 *   of all sources, on one of them. The rank pass compares every crossing of a line with every other one: its cost grows with the
 *   square of max_line_crossings, that is with about (1 + below + above)^2. ms_device as in the hatch; gsdf_hip_skin_rank_ms: of
 *   that, the rank and parity pass of the calling thread's last gsdf_hip_contour_hatch_skin.
 * The result is a gsdf_hatch: gsdf_hip_hatch_counts, _read and _destroy work on it unchanged. gsdf_hip_hatch_read_skin on a handle
 *   made by gsdf_hip_contour_hatch fails with GSDF_ERR_BAD_ARGUMENT (this handle has no classes). dry as in the hatch.
 * Errors. The hatch's checks of o, with its codes; a null k, below or above > 8: GSDF_ERR_BAD_ARGUMENT. GSDF_ERR_CAPACITY: 2^32
 *   crossings or more -- of source 0, or of all sources inside the layers' own line ranges k_min .. k_max (counted before the lines
 *   without an own crossing are left out) -- 2^32 (edge, source) pairs n_verts (1 + below + above) or more, or 2^31 line slots or more
 *   (the hatch's sum); all refused from counts, before anything of that size is allocated. A handle without loops gives a handle
 *   without segments and no error. Blocking; the result is independent of c afterwards.
 * Out of scope: dropping short pieces, widening skin by an overhang angle, joining pieces into paths, support generation, a
 *   segmented sort for lines with thousands of crossings. */
typedef struct gsdf_skin_opts {
  uint32_t below, above; /* 0 .. 8 each: the layers under and over a layer that must cover it */
} gsdf_skin_opts;
GSDF_ABI_ASSERT(sizeof(gsdf_skin_opts) == 8, "gsdf_skin_opts is 8 bytes");
typedef struct gsdf_skin_layer {
  double length[4];       /* by class: 0 inner, 1 bottom, 2 top, 3 both */
  uint64_t n_segments[4];
} gsdf_skin_layer;
GSDF_ABI_ASSERT(sizeof(gsdf_skin_layer) == 64, "gsdf_skin_layer is 64 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_skin_layer, n_segments) == 32, "gsdf_skin_layer fields");
typedef struct gsdf_skin_stats {
  uint64_t n_segments, n_crossings, n_own_crossings, n_lines, max_line_crossings, zero_length;
  uint64_t n_class[4]; /* pieces by class */
  double length[4];    /* all layers, by class */
  uint32_t n_layers, below, above, reserved;
  double ms_device;    /* last: bytes 0 .. 127 are a function of the inputs alone */
} gsdf_skin_stats;
GSDF_ABI_ASSERT(sizeof(gsdf_skin_stats) == 136, "gsdf_skin_stats is 136 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_skin_stats, zero_length) == 40 && offsetof(gsdf_skin_stats, n_class) == 48 && offsetof(gsdf_skin_stats, length) == 80, "gsdf_skin_stats sums");
GSDF_ABI_ASSERT(offsetof(gsdf_skin_stats, n_layers) == 112 && offsetof(gsdf_skin_stats, above) == 120 && offsetof(gsdf_skin_stats, ms_device) == 128, "gsdf_skin_stats fields");
int gsdf_hip_contour_hatch_skin(const gsdf_contour* c, const gsdf_hatch_opts* o, const gsdf_skin_opts* k, gsdf_hatch** out /* NULL allowed iff o->dry */, gsdf_skin_stats* st /* optional */);
/* cls n_segments bytes (0 .. 3), layers n_layers records; either may be NULL */
int gsdf_hip_hatch_read_skin(const gsdf_hatch* h, uint8_t* cls, gsdf_skin_layer* layers);
double gsdf_hip_skin_rank_ms(void);

/* ---- contours: offset (no reference counterpart) ---------------------------------------------------------------------------------------
 *
 * The step every consumer of loops takes first: move a boundary sideways by a stated in-plane distance -- a printer's walls at half a
 * bead, one and a half beads, ... inside the outline, the fill stopped a wall-stack short of it, a laser's kerf or a mill's radius in
 * either direction. Offset2D in a 2-D program is exact, but offsetting a 3-D field and slicing it is NOT an in-plane offset (the 3-D
 * distance is the shorter wherever the surface leans), and an uploaded or simplified handle has no field at all: the only correct
 * source is the stack of loops itself. gsdf_hip_contour_offset computes, for every layer of a gsdf_contour handle (traced, uploaded,
 * simplified, or itself an offset), the signed in-plane distance D of a lattice to the layer's own edges and traces the zero sets of
 * D + inset[i] with the tracer of the section "contours". The result is an ordinary gsdf_contour: simplify, measures, sections, hatch,
 * skin, read, counts and destroy work on it unchanged. Input layer l with inset i is output layer l n_insets + i (n_layers out =
 * n_layers in x n_insets): with n_insets = 1 the layers keep their numbers, and the hatch's direction l % n_dirs and the skin's
 * neighbours mean what they meant. gsdf_hip_contour_distance copies out D of ONE input layer (nx ny floats, row j behind row j - 1; nx
 * and ny from a dry offset call with the same options): an in-plane distance map of a slice, on exactly the lattice the offset call
 * uses. On the device, a function of the handle's arrays and the options alone, to the byte -- not of thread order, of the chunking,
 * or of which edges the kernel culls. Kernels: gsdf_amd/csrc/kernels_offset.h (abi_contour.hip); a numpy restatement over every edge:
 * tests/offsetref.py.
 *
 * Coordinates are taken as (double)float32 (exact). Every operation below is one IEEE float64 operation, in the order written, none
 *   contracted, unless marked fl: float32, rounded once.
 * Lattice. One lattice serves every layer and every inset of the call. xmin, ymin, xmax, ymax are the exact minima and maxima of
 *   the handle's vertices (all layers; a handle without vertices: all four 0). g = max(0, max_i(-inset[i])) (float32, exact). The box
 *   is fl(xmin - g), fl(ymin - g), fl(xmax + g), fl(ymax + g), and the paragraph "Lattice" of the section "contours" is applied to that
 *   box with res, by name: the same x0, nx, x_i and the same refusals (a box that is not finite among them), and one more:
 *   nx ny n_insets >= 2^31.
 * Edges. An edge runs from a vertex to its successor in the loop; the leader follows the last vertex: the hatch's edges.
 * Distance of node p = (x_i, y_j) to the edge a -> b.
 *     ex = bx - ax    ey = by - ay    wx = px - ax    wy = py - ay    ee = (ex ex) + (ey ey)
 *     h  = ee > 0 ? min(max(((wx ex) + (wy ey)) / ee, 0), 1) : 0
 *     qx = wx - (h ex)    qy = wy - (h ey)    d2 = (qx qx) + (qy qy)
 *   m2 = the minimum of d2 over the edges of the node's layer; +inf for a layer without loops. (A minimum does not depend on order.)
 * Band. band = fl(fl(max_i |inset[i]|) + fl(2 res)); a = min(sqrt(m2), (double)band), the square root correctly rounded. The clamp is
 *   what makes culling legal: an edge no nearer than band to a node cannot change that node's value.
 * Sign. The node is INSIDE iff an odd number of its layer's edges satisfy (ay < py) != (by < py) and x_c > px, with
 *     t = (py - ay) / (by - ay)    x_c = ax + (t (bx - ax))
 *   the hatch's crossing predicate and formula for the direction (1, 0): the even-odd rule. A count: it does not depend on order.
 * Field. D = fl(INSIDE ? -a : a) (float64 to float32, once); f_i = fl(D + inset[i]). inset > 0 moves the boundary INTO the material,
 *   < 0 grows the part, 0 re-traces it on the lattice. The lattice f_i of input layer l is traced as output layer l n_insets + i by the
 *   tracer's paragraphs "Inside", "Vertices", "Segments" and "Order", verbatim: zero is outside, a border node with f < 0 is forced
 *   outside and counted, keys and loop order as there.
 * Derived. |a| is 1-Lipschitz up to rounding, so a cut edge has both ends within |inset| + res of the loops: the clamp (band is 2 res
 *   beyond the largest |inset|) never touches a node that decides a vertex, and the loops are those of the unclamped distance. Every
 *   output vertex v has | dist(v, source loops) - |inset| | <= res plus rounding (the linear interpolation of a 1-Lipschitz function
 *   over one lattice edge). A distance offset ROUNDS outward corners. A remainder thinner than res fragments into small loops or
 *   vanishes (n_loops and saddle_cells show it); not an error. Where the field is exactly 0 (the medial line of a strip of width
 *   2 inset) the node is outside.
 * Chunks. Like the tracer's: a chunk holds whole input layers, each with all its insets, of at most max_nodes lattice nodes (always
 *   at least one input layer). The result and the integer statistics do not depend on it. On the HOST the call holds one word per
 *   input layer (the layers' edge ranges) and per output layer of a chunk, as the hatch holds its layer_start: a handle uploaded
 *   with 2^29 declared layers costs 2 GB there before the device sees any work. The layers are the caller's to keep sensible.
 * Statistics. inside_nodes and band_nodes count, over the input layers, the nodes that are INSIDE and the nodes with a < band;
 *   border_inside, saddle_cells, n_verts and n_loops cover the output (the tracer's counts). x0, y0, band, res: the lattice's. ms_field:
 *   device time of the distance and field kernels, ms_trace: of the tracer's steps, ms_device their sum. Bytes 0 .. 79 are a function of
 *   the inputs alone. gsdf_hip_contour_distance fills the lattice's fields, n_layers_in, n_insets and the two node counts of its one
 *   layer; the output's counts are 0. The result handle's own gsdf_contour_stats carries the tracer's fields with evals = 0 and
 *   ms_eval = ms_field.
 * dry != 0 fills the statistics and builds no handle: out may be NULL, and is set to NULL if it is not.
 * Errors. The lattice's refusals above; GSDF_ERR_BAD_ARGUMENT: n_insets 0 or > 8, a non-finite inset (of the first n_insets),
 *   reserved != 0, out NULL without dry, a NULL d_out, layer >= n_layers (the distance call). GSDF_ERR_CAPACITY: 2^32 output layers or
 *   vertices or more. A handle without loops gives a handle without loops. Blocking; the result is independent of c afterwards.
 * Out of scope: mitred or sharp outward corners (a distance offset rounds them), medial-axis gap fill, variable bead width, joining
 *   walls into one path, travel order. */
typedef struct gsdf_offset_opts {
  float res;          /* lattice spacing, finite, > 0 */
  uint32_t n_insets;  /* 1 .. 8 */
  uint32_t dry;       /* non-zero: statistics only */
  uint32_t reserved;  /* 0 */
  uint64_t max_nodes; /* lattice nodes per chunk; 0 = GSDF_CONTOUR_DEFAULT_MAX_NODES */
  float inset[8];     /* finite; > 0 moves the boundary INTO the material, < 0 grows the part, 0 re-traces it */
} gsdf_offset_opts;
GSDF_ABI_ASSERT(sizeof(gsdf_offset_opts) == 56, "gsdf_offset_opts is 56 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_offset_opts, n_insets) == 4 && offsetof(gsdf_offset_opts, dry) == 8 && offsetof(gsdf_offset_opts, reserved) == 12 && offsetof(gsdf_offset_opts, max_nodes) == 16 && offsetof(gsdf_offset_opts, inset) == 24, "gsdf_offset_opts fields");
typedef struct gsdf_offset_stats {
  uint64_t n_verts, n_loops, border_inside, saddle_cells, inside_nodes, band_nodes;
  uint32_t nx, ny, n_layers_in, n_insets;
  float x0, y0, band, res;
  double ms_field, ms_trace, ms_device; /* last: bytes 0 .. 79 are a function of the inputs alone */
} gsdf_offset_stats;
GSDF_ABI_ASSERT(sizeof(gsdf_offset_stats) == 104, "gsdf_offset_stats is 104 bytes");
GSDF_ABI_ASSERT(offsetof(gsdf_offset_stats, band_nodes) == 40 && offsetof(gsdf_offset_stats, nx) == 48 && offsetof(gsdf_offset_stats, n_insets) == 60 && offsetof(gsdf_offset_stats, x0) == 64 && offsetof(gsdf_offset_stats, res) == 76 && offsetof(gsdf_offset_stats, ms_field) == 80, "gsdf_offset_stats fields");
int gsdf_hip_contour_offset(const gsdf_contour* c, const gsdf_offset_opts* o, gsdf_contour** out /* NULL allowed iff dry */, gsdf_offset_stats* st /* optional */);
int gsdf_hip_contour_distance(const gsdf_contour* c, const gsdf_offset_opts* o, uint32_t layer, float* d_out /* nx ny floats, host */, gsdf_offset_stats* st /* optional */);

/* ---- multi-GPU (one process per GPU). The meshers shard with NO data-path collective (shard_rank / shard_count above); the
 * one exchange is the final variable-length gather of the ranks' results, over xGMI, inside this library: a Go caller needs no
 * Python for it. Replaces nothing in the reference (single device; its analogue of the split is the goroutine split of
 * glrender/flatrenderer.go:120-122); SURVEY.md section 8(e).
 *   rank 0: gsdf_hip_comm_unique_id(id) -> ship the 128 bytes to the other ranks by any means (file, socket, MPI, env)
 *   every rank (after gsdf_hip_init(device)): gsdf_hip_comm_create(id, rank, world, &comm)            [collective]
 *   per mesh: gsdf_hip_mesh_gatherv(local_mesh, comm, &all, counts)                                   [collective]
 * A gather = an all-gather of four counts per rank, then the transfers gsdf_hip_gather_plan lists for those counts as ONE group
 * of point-to-point sends / receives (ncclSend / ncclRecv: xGMI is one link per peer, every rank feeds all its links at once),
 * every rank's payload landing at offset sum(bytes of the ranks before it): no padding, no staging copies. What moves is the
 * meshes' payload (gsdf_mesh_opts.payload): triangles, or packed cut-leaf records -- 20 instead of 36 bytes per triangle on the
 * wire -- which the receiving ranks march into triangles behind the transfer. The result is a gsdf_mesh holding the triangles of
 * ALL ranks in rank order (device resident; every mesh accessor works on it). librccl is loaded at first use; without it these
 * calls fail with GSDF_ERR_HIP and everything else works. GSDF_HIP_COMM=loopback (environment, read by gsdf_hip_comm_unique_id)
 * selects an in-process transport instead -- the ranks are threads of one process on one GPU, a transfer is a device copy
 * ordered by events -- with which the whole path runs at any world size on a one-GPU box (the tests use it). World size <= 64. */
typedef struct gsdf_comm gsdf_comm;
#define GSDF_COMM_ID_BYTES 128
int gsdf_hip_comm_unique_id(uint8_t id[GSDF_COMM_ID_BYTES]);
int gsdf_hip_comm_create(const uint8_t id[GSDF_COMM_ID_BYTES], int rank, int world, gsdf_comm** out);
int gsdf_hip_comm_rank(const gsdf_comm* c);
int gsdf_hip_comm_world(const gsdf_comm* c);
const char* gsdf_hip_comm_transport(const gsdf_comm* c); /* "rccl" or "loopback" */
/* Sum over all ranks, in place, of n host values (Evaluations(), TotalPruned(), triangle totals). Collective. */
int gsdf_hip_comm_allreduce_sum_u64(gsdf_comm* c, uint64_t* vals, size_t n);
/* counts (optional): world entries, triangles contributed by each rank. */
int gsdf_hip_mesh_gatherv(const gsdf_mesh* m, gsdf_comm* c, gsdf_mesh** out, uint64_t* counts);
/* The same with a choice of who receives, and in two halves so that the payload can move while the caller meshes its next
 * part. Every rank of an all-gather INGESTS (world-1)/world of the whole mesh over its xGMI links -- several times what a rank
 * takes to mesh its share -- so the gather, not the meshing, bounds a step that ends in one (DESIGN.md section 7 has the numbers):
 *   GSDF_GATHER_ALL   every rank gets everything;
 *   GSDF_GATHER_ROOT  only `root` does (the other ranks' links carry their own shard only);
 *   GSDF_GATHER_NONE  counts only: every rank keeps its shard where it is.
 * _start: collective; returns when the counts are exchanged and the payload (and, for records, the marching pass behind it) is
 * enqueued on the communicator's own stream. `m` may be destroyed right away: its buffers are kept until the payload has moved.
 * _wait: blocks until the result is complete; *out = the gathered mesh (NULL on ranks that receive nothing), counts[world]
 * (triangles per rank), st (all optional). */
enum { GSDF_GATHER_ALL = 0, GSDF_GATHER_ROOT = 1, GSDF_GATHER_NONE = 2 };
typedef struct gsdf_gather gsdf_gather;
typedef struct gsdf_gather_stats {
  double ms_counts;         /* the counts exchange (all-gather of four u64 + readback), HIP events on the communicator's stream */
  double ms_payload;        /* the payload, first byte enqueued to last byte arrived */
  uint64_t bytes_sent;      /* of this rank's own payload, over all its links */
  uint64_t bytes_received;  /* of the other ranks' payloads */
  double ms_march;          /* records payload: marching cubes over the gathered records (0 for triangles) */
} gsdf_gather_stats;
GSDF_ABI_ASSERT(sizeof(gsdf_gather_stats) == 40, "gsdf_gather_stats is 40 bytes");
int gsdf_hip_mesh_gatherv_start(const gsdf_mesh* m, gsdf_comm* c, int mode, int root, gsdf_gather** pending);
int gsdf_hip_mesh_gatherv_wait(gsdf_gather* pending, gsdf_mesh** out, uint64_t* counts, gsdf_gather_stats* st);
void gsdf_hip_comm_destroy(gsdf_comm* c);

/* Host-only (runs without a GPU), pure: the transfers rank `rank` of `world` performs in a gather of payloads of
 * bytes_per_rank[r] bytes -- what gsdf_hip_mesh_gatherv_start executes as one group. Layout of the gathered buffer: rank-major,
 * payload r at offset sum(bytes_per_rank[< r]). ops (ops_cap entries; NULL to count) receives
 *   GSDF_GOP_COPY  this rank's own payload [src_off, +bytes) -> gathered buffer at dst_off   (a device copy)
 *   GSDF_GOP_SEND  this rank's own payload [src_off, +bytes) -> rank `peer`
 *   GSDF_GOP_RECV  bytes from rank `peer` -> gathered buffer at dst_off
 * in an order in which, executed entry by entry with non-blocking sends, the ranks' lists match up (peers are visited in
 * rotated order: rank+1, rank+2, ...). Ranks with nothing to contribute appear in nobody's list. *total_bytes = size of this
 * rank's gathered buffer (0 if it receives nothing). tests/test_gather_gloo.py runs these lists with gloo on CPU. */
enum { GSDF_GOP_COPY = 0, GSDF_GOP_SEND = 1, GSDF_GOP_RECV = 2 };
typedef struct gsdf_gather_op {
  int32_t kind;
  int32_t peer;
  uint64_t src_off;
  uint64_t dst_off;
  uint64_t bytes;
} gsdf_gather_op;
GSDF_ABI_ASSERT(sizeof(gsdf_gather_op) == 32, "gsdf_gather_op is 32 bytes");
int gsdf_hip_gather_plan(const uint64_t* bytes_per_rank, int world, int rank, int mode, int root, gsdf_gather_op* ops, size_t ops_cap,
                         size_t* n_ops, uint64_t* total_bytes);

/* Host-only helper (runs without a GPU): owner rank of octree brick (x,y,z) under the multi-GPU partition
 * gsdf_hip_mesh_octree applies on device -- a pure function of the coordinates, so ranks never communicate. */
uint32_t gsdf_hip_brick_owner(uint32_t x, uint32_t y, uint32_t z, uint32_t count);
/* Host-only helper: the z-slab [*lo, *hi) of n lattice planes owned by rank `rank` of `count` in gsdf_hip_mesh_flat (cube
 * planes) and gsdf_hip_mesh_dualcontour (cell planes): contiguous, disjoint, covering [0, n) -- the reference's goroutine
 * split of the flat lattice (flatrenderer.go:120-122). */
void gsdf_hip_slab_range(uint32_t n, uint32_t rank, uint32_t count, uint32_t* lo, uint32_t* hi);

#ifdef __cplusplus
}
#endif
#endif
