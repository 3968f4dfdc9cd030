// kernels_view.h -- the UI's ray-marched view of a 3-D part (gsdfaux.UI's fragment shader, gsdfaux/ui.go:247-355), headless:
// view_kernel. The frame's exact float32 arithmetic is stated in include/gsdf_hip.h (gsdf_view); tests/viewref.py is its CPU twin.
//
// Not part of kernels.h: the whole-set builds compile what they compiled before; abi_eval.hip includes this header for the
// ahead-of-time (interpreter) kernels, and a specialised handle builds view_kernel in a module of its own on its first frame
// (abi_eval.hip: spec_view; specialize.cpp: spec_includes).
//
// Each lane runs ONE pixel as a small state machine -- sample index, phase (march, or normal tap 0..3), step, t, rd, the running
// colour sum -- and every trip through the wave's loop builds one position per lane from that state and makes ONE sdf_eval call
// with all 64 lanes active (the evaluator's control flow is wave-uniform and each lane owns an LDS column). A lane without a pixel
// evaluates the camera position and its result and count are dropped. A pixel's samples run one after another in its lane, so the
// colour sums in the contract's order whatever lane or wave ran it.
//   REFILL = true   persistent waves: a lane whose pixel is done writes it out and claims the next one (wave_append on a
//                   per-launch counter), in 8 x 8 screen tiles so that a wave's rays stay close together; the loop runs while any
//                   lane of the wave has work.
//   REFILL = false  the plain form: one pixel per lane (one tile per wave), the wave runs until its slowest lane is done.
// Both give the same bytes. The plain form is the default: it measured 1.3-2x faster; GSDF_HIP_VIEW_REFILL=1
// selects the other. The wave's evaluation count leaves with one 64-bit atomic.
#pragma once
#include "kernels_common.h"

#define VIEW_TILE 8  // screen tiles of VIEW_TILE x VIEW_TILE pixels: one wave's worth of claims

// The camera as the kernel takes it (filled by abi_eval.hip: gsdf_hip_render3 from a gsdf_view)
struct ViewCam {
  float ro[3], uu[3], vv[3], ww[3];
  float tmax;           // 1.3f * char_dist
  int aa, max_steps, w, h;
  unsigned tiles_x;     // ceil(w / VIEW_TILE)
  unsigned n_claims;    // tiles_x * tiles_y * VIEW_TILE^2: claim c -> tile c / 64, pixel c % 64 of it (row-major)
};

namespace view {
// NaN by its bits: the specialised kernels are built with -fno-honor-nans, under which a comparison with a NaN operand is
// whatever is cheapest (kernels_common.h: nb). An integer test says what IEEE says in every build.
__device__ __forceinline__ bool is_nan(float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ bool lt(float a, float b) { return !is_nan(a) && !is_nan(b) && a < b; }
__device__ __forceinline__ bool gt(float a, float b) { return !is_nan(a) && !is_nan(b) && a > b; }
// clamp(x, 0, 1) = fmin(fmax(x, 0), 1): a NaN gives 0
__device__ __forceinline__ float clamp01(float x) { return is_nan(x) ? 0.f : (x < 0.f ? 0.f : (x > 1.f ? 1.f : x)); }
__device__ __forceinline__ uint32_t to_byte(float c) { return (uint32_t)(clamp01(c) * 255.f + 0.5f); }

constexpr float kTol = 1e-4f;
constexpr float kE = 0.5773f;           // calcNormal's e = (1, -1) * 0.5773
constexpr float kK = 0.5773f * 1e-4f;   // e.x * eps: the tap offset
constexpr float kL = 0.57703f;          // the light direction's components
}  // namespace view

template <bool REFILL>
__global__ void __launch_bounds__(BLOCK, 4) view_kernel(const uint32_t* __restrict__ code_g, ViewCam cam, uint32_t* __restrict__ rgba,
                                                        float* __restrict__ depth, uint32_t* __restrict__ evals,
                                                        unsigned long long* __restrict__ ctr /* [0] claims, [1] evaluations */) {
  using namespace view;
  code_ptr code = as_code(code_g);
  float* lds = g_smem + threadIdx.x;
  const int nsamp = cam.aa * cam.aa;
  const float fa = (float)cam.aa, fw = (float)cam.w, fh = (float)cam.h;
  // the lane's pixel: index into the outputs (-1: none), fragCoord, and its state
  int pix = -1;
  float fx = 0.f, fy = 0.f;
  int s = 0, ph = 0, st = 0;  // sample, phase (0 march, 1..4 after normal tap 0..3), march steps
  float t = 0.f, rx = 0.f, ry = 0.f, rz = 0.f;
  float nx = 0.f, ny = 0.f, nz = 0.f;  // the normal's sums, one tap at a time, left to right
  float tr = 0.f, tg = 0.f, tb = 0.f, dep = __builtin_inff();
  uint32_t ev = 0;         // evaluations of the lane's current pixel
  uint32_t lane_ev = 0;    // ... of every pixel the lane ran
  bool more = REFILL;      // the lane may still claim

  auto start_sample = [&]() {  // o, p, rd of sample s (ui.go:313-318)
    const int m = s / cam.aa, n = s - m * cam.aa;
    const float ox = (float)m / fa - 0.5f, oy = (float)n / fa - 0.5f;
    const float px = (2.f * (fx + ox) - fw) / fh, py = (2.f * (fy + oy) - fh) / fh;
    const float ax = (px * cam.uu[0] + py * cam.vv[0]) + 1.5f * cam.ww[0];
    const float ay = (px * cam.uu[1] + py * cam.vv[1]) + 1.5f * cam.ww[1];
    const float az = (px * cam.uu[2] + py * cam.vv[2]) + 1.5f * cam.ww[2];
    const float len = __builtin_sqrtf((ax * ax + ay * ay) + az * az);
    rx = ax / len; ry = ay / len; rz = az / len;
    t = 0.f; st = 0; ph = 0;
  };
  auto begin_pixel = [&](unsigned c) {  // claim c -> pixel (tile-major); a claim off the image's edge leaves the lane free
    const unsigned tile = c / (VIEW_TILE * VIEW_TILE), in = c % (VIEW_TILE * VIEW_TILE);
    const unsigned i = (tile % cam.tiles_x) * VIEW_TILE + in % VIEW_TILE, r = (tile / cam.tiles_x) * VIEW_TILE + in / VIEW_TILE;
    if (i >= (unsigned)cam.w || r >= (unsigned)cam.h) return;
    pix = (int)(r * (unsigned)cam.w + i);
    fx = (float)i + 0.5f;
    fy = (float)(cam.h - 1 - (int)r) + 0.5f;  // output row r is GL row h - 1 - r
    s = 0; ev = 0;
    tr = tg = tb = 0.f;
    dep = __builtin_inff();
    start_sample();
  };

  if (!REFILL) {
    const unsigned c = blockIdx.x * BLOCK + threadIdx.x;
    if (c < cam.n_claims) begin_pixel(c);
  }
#pragma unroll 1
  for (;;) {
    if (REFILL) {
#pragma unroll 1
      for (;;) {  // free lanes claim until every lane has a pixel or the frame is handed out (wave-uniform trip count)
        const bool need = pix < 0 && more;
        if (__ballot(need) == 0ull) break;
        const unsigned long long c = wave_append(need, &ctr[0]);
        if (need) {
          if (c >= (unsigned long long)cam.n_claims) more = false;
          else begin_pixel((unsigned)c);
        }
      }
    }
    if (!dm::wave_any(pix >= 0)) break;
    const bool act = pix >= 0;
    // pos = ro + t rd; the normal's taps at the hit position (ui.go:324,338-339,254-260)
    const float hx = cam.ro[0] + t * rx, hy = cam.ro[1] + t * ry, hz = cam.ro[2] + t * rz;
    const float ox = (ph == 1 || ph == 4) ? kK : -kK;
    const float oy = (ph == 3 || ph == 4) ? kK : -kK;
    const float oz = (ph == 2 || ph == 4) ? kK : -kK;
    P3 p[1];
    p[0] = ph == 0 ? P3{hx, hy, hz} : P3{hx + ox, hy + oy, hz + oz};
    if (!act) p[0] = P3{cam.ro[0], cam.ro[1], cam.ro[2]};
    float d[1];
    gsdf_dev::sdf_eval<1>(code, p, d, lds, BLOCK);
    if (!act) continue;
    const float dv = d[0];
    ev++;
    lane_ev++;
    bool done = false;
    if (ph == 0) {  // ui.go:322-331
      st++;
      const bool hit = lt(dv, kTol);
      if (hit) {
        ph = 1;
        if (lt(t, dep)) dep = t;
      } else if (gt(t, cam.tmax)) {
        done = true;
      } else {
        t = t + dv;
        done = st >= cam.max_steps;
      }
    } else {  // normal tap ph - 1: nor += e.??? * d (ui.go:256-260)
      const float a = (ph == 1 || ph == 4) ? kE : -kE;  // e.xyy, e.yyx, e.yxy, e.xxx
      const float b = (ph == 3 || ph == 4) ? kE : -kE;
      const float cz = (ph == 2 || ph == 4) ? kE : -kE;
      if (ph == 1) { nx = a * dv; ny = b * dv; nz = cz * dv; }
      else { nx = nx + a * dv; ny = ny + b * dv; nz = nz + cz * dv; }
      ph++;
      if (ph == 5) {  // shading (ui.go:336-344)
        const float len = __builtin_sqrtf((nx * nx + ny * ny) + nz * nz);
        const float ux = nx / len, uy = ny / len, uz = nz / len;
        const float dif = clamp01((ux * kL + uy * kL) + uz * kL);
        const float amb = 0.5f + 0.5f * uy;
        tr = tr + __builtin_sqrtf(0.2f * amb + 0.8f * dif);
        tg = tg + __builtin_sqrtf(0.3f * amb + 0.7f * dif);
        tb = tb + __builtin_sqrtf(0.4f * amb + 0.5f * dif);
        done = true;
      }
    }
    if (done) {
      if (++s < nsamp) {
        start_sample();
      } else {  // tot /= float(uAA*uAA); the pixel goes out and the lane is free
        const float fs = (float)nsamp;
        rgba[pix] = to_byte(tr / fs) | (to_byte(tg / fs) << 8) | (to_byte(tb / fs) << 16) | 0xff000000u;
        depth[pix] = dep;
        evals[pix] = ev;
        pix = -1;
      }
    }
  }
  unsigned long long v = lane_ev;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63u) == 0u && v) atomicAdd(&ctr[1], v);
}
