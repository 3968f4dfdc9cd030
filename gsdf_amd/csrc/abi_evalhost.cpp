// abi_evalhost.cpp -- C ABI (include/gsdf_hip.h), the evaluator side's entry points that run on the host alone: the lowering of a tree
// for inspection, the UI's orbit camera, the picture size and colour conversions of a 2-D part, and gleval.BlockCachedSDF3 over a
// program. No device code and no program handle: what the block cache needs of a program it asks through the public ABI.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <new>
#include <unordered_map>
#include <vector>

#include "abi_host.h"
#include "compile.h"

// Lower a tree to the device instruction stream, for inspection/tests.
extern "C" int gsdf_hip_lower(const gsdf_tree* tree, uint32_t* code_out, uint32_t code_cap, uint32_t* code_words, uint32_t* lds_slots) {
  if (!tree) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  try {
    gsdf_dev::Program pr = gsdf_dev::compile(*tree);
    if (code_words) *code_words = (uint32_t)pr.code.size();
    if (lds_slots) *lds_slots = (uint32_t)pr.nslots;
    if (code_out) {
      if (code_cap < pr.code.size()) return fail(GSDF_ERR_SHORT_BUFFER, "short buffer");
      std::memcpy(code_out, pr.code.data(), pr.code.size() * sizeof(uint32_t));
    }
    return GSDF_OK;
  } catch (const std::exception& e) {
    return fail(GSDF_ERR_BAD_TREE, e.what());
  }
}

// Test hook: the lower-bound region the compiler claims for the subtree of `node` (0 none, 1 box, 2 z-cylinder).
extern "C" int gsdf_hip_lower_region(const gsdf_tree* tree, uint32_t node, int* kind, float params[8]) {
  if (!tree || !kind || !params) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  try {
    *kind = gsdf_dev::region_of(*tree, node, params);
    return GSDF_OK;
  } catch (const std::exception& e) {
    return fail(GSDF_ERR_BAD_TREE, e.what());
  }
}

// ---- the UI's view of a 3-D part (gsdfaux.UI, gsdfaux/ui.go:247-355): camera helper (the frame: abi_eval.hip) -----------------
namespace {
// math32.Hypot (scaffold/ms.hpp: hypotf32): the bounds' Diagonal() = Norm(Size()) by nested hypot
float hypot32(float p, float q) {
  if (std::isinf(p) || std::isinf(q)) return INFINITY;
  if (p != p || q != q) return NAN;
  p = std::fabs(p); q = std::fabs(q);
  if (p < q) std::swap(p, q);
  if (p == 0) return 0;
  q = q / p;
  return p * std::sqrt(1 + q * q);
}
void normalize3(const float a[3], float out[3]) {
  const float len = std::sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
  out[0] = a[0] / len; out[1] = a[1] / len; out[2] = a[2] / len;
}
void cross3(const float a[3], const float b[3], float out[3]) {
  out[0] = a[1] * b[2] - a[2] * b[1];
  out[1] = a[2] * b[0] - a[0] * b[2];
  out[2] = a[0] * b[1] - a[1] * b[0];
}
}  // namespace

// ui.go:18 (diag), 123 (camDist = diag), 220 (charDist = camDist + diag), 276-297 (orbit camera).
extern "C" int gsdf_hip_view_orbit(const float bb[6], float yaw, float pitch, float cam_dist, const float target[3], gsdf_view* view) {
  if (!bb || !view) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (!finite_all(bb, 6) || !std::isfinite(yaw) || !std::isfinite(pitch) || !std::isfinite(cam_dist) || (target && !finite_all(target, 3)))
    return fail(GSDF_ERR_BAD_ARGUMENT, "non-finite bounds, angle, distance or target");
  const float diag = hypot32(bb[3] - bb[0], hypot32(bb[4] - bb[1], bb[5] - bb[2]));
  const float cd = cam_dist > 0.f ? cam_dist : diag;
  if (!(cd > 0.f) || !std::isfinite(cd + diag)) return fail(GSDF_ERR_BAD_ARGUMENT, "empty bounds and no camera distance");
  const float kPi = 3.14159265359f;  // ui.go:269
  const float lim_lo = -kPi / 2.0f + 0.01f, lim_hi = kPi / 2.0f - 0.01f;
  const float pc = std::fmin(std::fmax(pitch, lim_lo), lim_hi);
  const float cp = (float)std::cos((double)pc), sp = (float)std::sin((double)pc);
  const float cy = (float)std::cos((double)yaw), sy = (float)std::sin((double)yaw);
  const float dir[3] = {cp * sy, sp, cp * cy};
  const float ta[3] = {target ? target[0] : 0.f, target ? target[1] : 0.f, target ? target[2] : 0.f};
  gsdf_view v;
  std::memset(&v, 0, sizeof v);
  float fwd[3], right[3];
  for (int a = 0; a < 3; a++) v.ro[a] = ta[a] - dir[a] * cd;
  for (int a = 0; a < 3; a++) fwd[a] = ta[a] - v.ro[a];
  normalize3(fwd, v.ww);
  const float up[3] = {0.f, 1.f, 0.f};
  cross3(v.ww, up, right);
  normalize3(right, v.uu);
  cross3(v.uu, v.ww, v.vv);
  v.char_dist = cd + diag;
  v.aa = 1;
  v.max_steps = 256;
  if (!finite_all(v.ro, 3) || !finite_all(v.uu, 3) || !finite_all(v.vv, 3) || !finite_all(v.ww, 3))
    return fail(GSDF_ERR_BAD_ARGUMENT, "degenerate camera (the camera distance vanishes next to the target)");
  *view = v;
  return GSDF_OK;
}

// ---- a 2-D part's picture with gsdfaux's colour conversions (gsdfaux.RenderPNGFile, gsdfaux/gsdfaux.go:264-296; color.go) --------
// RenderPNGFile's picture size (gsdfaux.go:271-274).
extern "C" int gsdf_hip_picture_size(const float bb[6], int pic_height, int* w) {
  if (!bb || !w) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (!finite_all(bb, 6)) return fail(GSDF_ERR_BAD_ARGUMENT, "non-finite bounds");
  if (pic_height < 1 || pic_height > 16384) return fail(GSDF_ERR_BAD_ARGUMENT, "picture height must be 1 .. 16384");
  const float szx = bb[3] - bb[0], szy = bb[4] - bb[1];
  if (!(szy > 0.f) || !std::isfinite(szx) || !std::isfinite(szy)) return fail(GSDF_ERR_BAD_ARGUMENT, "empty or non-finite bounds");
  const double pix_per_unit = (double)pic_height / (double)szy;
  const double wd = pix_per_unit * (double)szx;
  if (!(wd >= 1.0 && wd < 16385.0)) return fail(GSDF_ERR_BAD_ARGUMENT, "picture width comes out outside 1 .. 16384");
  *w = (int)wd;
  return GSDF_OK;
}

// ColorConversionInigoQuilez with RenderPNGFile's default, ms2.Box.Diagonal() / 3 (gsdfaux.go:268).
extern "C" int gsdf_hip_color_iq(const float bb[6], float char_dist, gsdf_color2* out) {
  if (!out || (!bb && !(char_dist > 0.f))) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  float cd = char_dist;
  if (!std::isfinite(cd)) return fail(GSDF_ERR_BAD_ARGUMENT, "non-finite characteristic distance");
  if (!(cd > 0.f)) {
    if (!finite_all(bb, 6)) return fail(GSDF_ERR_BAD_ARGUMENT, "non-finite bounds");
    cd = hypot32(bb[3] - bb[0], bb[4] - bb[1]) / 3.f;
    if (!(cd > 0.f) || !std::isfinite(cd)) return fail(GSDF_ERR_BAD_ARGUMENT, "empty bounds and no characteristic distance");
  }
  gsdf_color2 c;
  std::memset(&c, 0, sizeof c);
  c.kind = GSDF_COLOR_IQ;
  c.length = cd;
  *out = c;
  return GSDF_OK;
}

// ColorConversionLinearGradient (color.go:50-71): Go's `c0 == color.Black && c1 == color.White` selects the black-and-white closure.
extern "C" int gsdf_hip_color_gradient(float length, const uint8_t c0[4], const uint8_t c1[4], gsdf_color2* out) {
  if (!c0 || !c1 || !out) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (!std::isfinite(length) || length < 0.f) return fail(GSDF_ERR_BAD_ARGUMENT, "gradient length must be finite and >= 0");
  gsdf_color2 c;
  std::memset(&c, 0, sizeof c);
  const bool black = c0[0] == 0 && c0[1] == 0 && c0[2] == 0 && c0[3] == 255;
  const bool white = c1[0] == 255 && c1[1] == 255 && c1[2] == 255 && c1[3] == 255;
  c.kind = black && white ? GSDF_COLOR_BW_SMOOTH : GSDF_COLOR_GRADIENT;
  c.length = length;
  std::memcpy(c.c0, c0, 4);
  std::memcpy(c.c1, c1, 4);
  *out = c;
  return GSDF_OK;
}

// ---- gleval.BlockCachedSDF3 (gleval/gleval.go:110-218) over a HIP program ---------------------------------------
// Host-side wrapper, as in the reference: a lossy cache keyed by the lattice cell of the position
// (int(mul * (p - bb.Min)) per axis, mul = 1/res); misses are evaluated in ONE batch by the wrapped evaluator.
struct gsdf_blockcache {
  gsdf_program* sdf = nullptr;
  float mul[3] = {0, 0, 0};
  struct Key { long long x, y, z; bool operator==(const Key& o) const { return x == o.x && y == o.y && z == o.z; } };
  struct Hash {
    size_t operator()(const Key& k) const {
      unsigned long long h = (unsigned long long)k.x * 0x9E3779B97F4A7C15ull;
      h ^= (unsigned long long)k.y + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
      h ^= (unsigned long long)k.z + 0x9E3779B97F4A7C15ull + (h << 6) + (h >> 2);
      return (size_t)h;
    }
  };
  std::unordered_map<Key, float, Hash> m;
  std::vector<float> posbuf, distbuf;
  std::vector<size_t> idxbuf;
  uint64_t hits = 0, evals = 0;
};

extern "C" int gsdf_hip_blockcache_reset(gsdf_blockcache* c, gsdf_program* sdf, float resx, float resy, float resz) {
  if (!c || !sdf) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (resx <= 0 || resy <= 0 || resz <= 0 || std::isnan(resx) || std::isnan(resy) || std::isnan(resz))
    return fail(GSDF_ERR_RESOLUTION, "invalid resolution for BlockCachedSDF3");  // gleval.go:127-129
  if (gsdf_hip_program_is2d(sdf)) return fail(GSDF_ERR_DIMENSION, "program is 2D");
  c->m.clear();
  c->sdf = sdf;
  c->mul[0] = 1.0f / resx; c->mul[1] = 1.0f / resy; c->mul[2] = 1.0f / resz;  // DivElem({1,1,1}, res)
  c->posbuf.clear(); c->distbuf.clear(); c->idxbuf.clear();
  c->hits = 0; c->evals = 0;  // Reset also resets the statistics (gleval.go:124)
  return GSDF_OK;
}
extern "C" int gsdf_hip_blockcache_create(gsdf_program* sdf, float resx, float resy, float resz, gsdf_blockcache** out) {
  if (!out) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  *out = nullptr;
  gsdf_blockcache* c = new (std::nothrow) gsdf_blockcache();
  if (!c) return fail(GSDF_ERR_BAD_ARGUMENT, "out of memory");
  const int rc = gsdf_hip_blockcache_reset(c, sdf, resx, resy, resz);
  if (rc) { delete c; return rc; }
  *out = c;
  return GSDF_OK;
}
extern "C" void gsdf_hip_blockcache_destroy(gsdf_blockcache* c) { delete c; }
extern "C" uint64_t gsdf_hip_blockcache_hits(const gsdf_blockcache* c) { return c ? c->hits : 0; }
extern "C" uint64_t gsdf_hip_blockcache_evaluations(const gsdf_blockcache* c) { return c ? c->evals : 0; }

// (*BlockCachedSDF3).Evaluate (gleval.go:154-211). pos: n x 3 float32 with the given byte stride (12 or 16).
extern "C" int gsdf_hip_blockcache_eval3(gsdf_blockcache* c, const void* pos, size_t stride, size_t n_pos, float* dist, size_t n_dist) {
  if (!c || !c->sdf) return fail(GSDF_ERR_BAD_ARGUMENT, "null argument");
  if (n_pos != n_dist) return fail(GSDF_ERR_LENGTH_MISMATCH, "position and distance buffer length mismatch");
  if (n_pos == 0) return fail(GSDF_ERR_EMPTY_BUFFERS, "empty buffers");
  if (!pos || !dist) return fail(GSDF_ERR_BAD_ARGUMENT, "null buffer");
  if (stride % 4 != 0 || stride < 12) return fail(GSDF_ERR_BAD_ARGUMENT, "bad position stride");
  float bb[6];
  if (int rc = gsdf_hip_program_bounds(c->sdf, bb)) return rc;
  const float* bbmin = bb;
  auto key_of = [&](const float* p) {
    // tp = MulElem(mul, Sub(p, bb.Min)); int(tp.X) truncates toward zero (Go float->int conversion)
    gsdf_blockcache::Key k;
    k.x = (long long)(c->mul[0] * (p[0] - bbmin[0]));
    k.y = (long long)(c->mul[1] * (p[1] - bbmin[1]));
    k.z = (long long)(c->mul[2] * (p[2] - bbmin[2]));
    return k;
  };
  c->posbuf.clear();
  c->idxbuf.clear();
  const char* base = (const char*)pos;
  for (size_t i = 0; i < n_pos; i++) {
    const float* p = (const float*)(base + i * stride);
    auto it = c->m.find(key_of(p));
    if (it != c->m.end()) {
      dist[i] = it->second;
    } else {
      c->posbuf.insert(c->posbuf.end(), p, p + 3);
      c->idxbuf.push_back(i);
    }
  }
  const size_t nseek = c->idxbuf.size();
  if (nseek > 0) {
    c->distbuf.resize(nseek);
    const int rc = gsdf_hip_eval3(c->sdf, c->posbuf.data(), 12, nseek, c->distbuf.data(), nseek);
    if (rc) return rc;
    for (size_t i = 0; i < nseek; i++) c->m[key_of(&c->posbuf[3 * i])] = c->distbuf[i];  // later entries of a cell overwrite
    for (size_t i = 0; i < nseek; i++) dist[c->idxbuf[i]] = c->distbuf[i];
  }
  c->evals += n_pos;
  c->hits += n_pos - nseek;
  return GSDF_OK;
}
