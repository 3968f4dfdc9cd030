// kernels_image.h -- a 2-D part's picture with the reference's colour conversions (gsdfaux.RenderPNGFile, gsdfaux/gsdfaux.go:264-296;
// gsdfaux/color.go): image2_color_kernel. The conversions' exact float32 arithmetic is stated in include/gsdf_hip.h (gsdf_color2);
// tests/colorref.py is its CPU twin.
//
// Not part of kernels.h: the whole-set builds compile what they compiled before; abi_eval.hip includes this header for the
// ahead-of-time (interpreter) kernels, and a specialised handle builds image2_color_kernel in a module of its own on its first
// picture (abi_eval.hip: spec_image_color; specialize.cpp: spec_includes).
//
// One fused pass: the lattice of image2_kernel (kernels_eval.h, the same statements), sdf_eval, then the conversion per point and
// one 32-bit store per pixel (plus the optional distance). The conversion runs after sdf_eval has returned, so it adds nothing to
// the interpreter's register peak; its kind is a template argument (KIND >= 0: the per-tree kernels, one per kind) or, for the
// interpreter kernels (KIND = -1), a kernel argument -- wave-uniform either way, no lane diverges on it.
//
// Comparisons that may meet a NaN test its bits: the specialised kernels are built with -fno-honor-nans, under which a comparison
// with a NaN operand is whatever is cheapest (kernels_common.h: nb). The float64 Exp / Cos are written operation by operation,
// uncontracted, as the contract states them.
#pragma once
#include "kernels_common.h"

// The conversion as the kernel takes it (filled by abi_eval.hip: gsdf_hip_image2_color from a gsdf_color2)
struct ColorConv {
  int kind;        // GSDF_COLOR_*: 0 default, 1 IQ, 2 gradient, 3 black and white
  float length;
  uint32_t c0, c1; // RGBA bytes, little-endian (R in the low byte), as the output pixels
};

namespace pic {
#pragma clang fp contract(off)
__device__ __forceinline__ bool is_nan(float v) { return (__float_as_uint(v) & 0x7fffffffu) > 0x7f800000u; }
__device__ __forceinline__ bool lt(float a, float b) { return !is_nan(a) && !is_nan(b) && a < b; }
__device__ __forceinline__ bool gt(float a, float b) { return !is_nan(a) && !is_nan(b) && a > b; }
__device__ __forceinline__ bool le(float a, float b) { return !is_nan(a) && !is_nan(b) && a <= b; }
__device__ __forceinline__ bool ge(float a, float b) { return !is_nan(a) && !is_nan(b) && a >= b; }
// ms1.Clamp: a NaN stays NaN
__device__ __forceinline__ float clamp(float v, float lo, float hi) { return is_nan(v) ? v : (v < lo ? lo : (v > hi ? hi : v)); }
// ms1.Interp
__device__ __forceinline__ float interp(float x, float y, float a) { return x + a * (y - x); }
// Go's float -> uint8 / uint32 conversion as amd64 performs it: truncation to int64, low bits kept; NaN and |v| >= 2^63 -> 0
__device__ __forceinline__ uint32_t to_int_bits(float v) {
  const uint32_t a = __float_as_uint(v) & 0x7fffffffu;
  if (a >= 0x5f000000u) return 0u;  // |v| >= 2^63, +-Inf, NaN
  return (uint32_t)(uint64_t)(long long)v;
}
__device__ __forceinline__ uint32_t rgba(uint32_t r, uint32_t g, uint32_t b) { return (r & 0xffu) | ((g & 0xffu) << 8) | ((b & 0xffu) << 16) | 0xff000000u; }

__device__ __forceinline__ bool is_nan64(double v) { return ((uint64_t)__double_as_longlong(v) & 0x7fffffffffffffffull) > 0x7ff0000000000000ull; }

// math.Exp (go/src/math/exp.go: FreeBSD e_exp.c), float64
__device__ inline double exp64(double x) {
#pragma clang fp contract(off)
  const double Ln2Hi = 6.93147180369123816490e-01, Ln2Lo = 1.90821492927058770002e-10, Log2e = 1.44269504088896338700e+00;
  const double Overflow = 7.09782712893383973096e+02, Underflow = -7.45133219101941108420e+02, NearZero = 1.0 / (1 << 28);
  const double P1 = 1.66666666666666657415e-01, P2 = -2.77777777770155933842e-03, P3 = 6.61375632143793436117e-05,
               P4 = -1.65339022054652515390e-06, P5 = 4.13813679705723846039e-08;
  const uint64_t b = (uint64_t)__double_as_longlong(x);
  if (is_nan64(x) || b == 0x7ff0000000000000ull) return x;
  if (b == 0xfff0000000000000ull) return 0.0;
  if (x > Overflow) return __longlong_as_double(0x7ff0000000000000ll);
  if (x < Underflow) return 0.0;
  if (-NearZero < x && x < NearZero) return 1.0 + x;
  int k = 0;
  if (x < 0) k = (int)(Log2e * x - 0.5);
  else if (x > 0) k = (int)(Log2e * x + 0.5);
  const double hi = x - (double)k * Ln2Hi;
  const double lo = (double)k * Ln2Lo;
  // expmulti
  const double r = hi - lo;
  const double t = r * r;
  const double c = r - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
  const double y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi);
  // Ldexp(y, k), exact up to the one rounding of the result: two power-of-two factors, each representable (|k| <= 1076)
  const int k1 = k / 2, k2 = k - k1;
  return (y * __longlong_as_double((long long)(k1 + 1023) << 52)) * __longlong_as_double((long long)(k2 + 1023) << 52);
}

// math.Cos (go/src/math/sin.go) with Cody-Waite reduction at every finite argument (the contract's statement; Go itself switches
// to Payne-Hanek at |x| >= 2^29); an integer part x (4/pi) >= 2^64 is taken as 0.
__device__ inline double cos64(double x) {
#pragma clang fp contract(off)
  const uint64_t b = (uint64_t)__double_as_longlong(x) & 0x7fffffffffffffffull;
  if (b >= 0x7ff0000000000000ull) return __longlong_as_double(0x7ff8000000000000ll);  // NaN, +-Inf -> NaN
  bool sign = false;
  x = __builtin_fabs(x);
  const double v = x * (4.0 / DM_PI);
  uint64_t j = v < 18446744073709551616.0 ? (uint64_t)v : 0ull;
  double y = (double)j;
  if (j & 1) { j++; y += 1.0; }
  j &= 7;
  const double z = ((x - y * 7.85398125648498535156e-1) - y * 3.77489470793079817668e-8) - y * 2.69515142907905952645e-15;
  if (j > 3) { j -= 4; sign = !sign; }
  if (j > 1) sign = !sign;
  const double zz = z * z;
  const double r = (j == 1 || j == 2) ? dm::trig_poly_sin(z, zz) : dm::trig_poly_cos(zz);
  return sign ? -r : r;
}

// ColorConversionInigoQuilez (color.go:21-46)
__device__ inline uint32_t iq(float d, float inv) {
#pragma clang fp contract(off)
  if (is_nan(d)) return 0xff0000ffu;
  d = d * inv;
  const bool pos = gt(d, 0.f);
  float cx = pos ? 0.9f : 0.65f, cy = pos ? 0.6f : 0.85f, cz = pos ? 0.3f : 1.0f;
  const float a = __builtin_fabsf(d);
  const float s1 = 1.f - (float)exp64((double)(-6.f * a));
  cx = s1 * cx; cy = s1 * cy; cz = s1 * cz;
  const float s2 = 0.8f + 0.2f * (float)cos64((double)(150.f * d));
  cx = s2 * cx; cy = s2 * cy; cz = s2 * cz;
  const float t = clamp(a / 0.01f, 0.f, 1.f);  // SmoothStep(0, 0.01, a): (a - 0) / (0.01 - 0)
  const float mx = 1.f - (t * t) * (3.f - 2.f * t);
  cx = interp(cx, 1.f, mx); cy = interp(cy, 1.f, mx); cz = interp(cz, 1.f, mx);
  return rgba(to_int_bits(cx * 255.f), to_int_bits(cy * 255.f), to_int_bits(cz * 255.f));
}

// the untyped constants k/6 and k/3 of color.go, as float32 nearest to the exact rationals
constexpr float k1_6 = 0.16666667163372039794921875f;   // float32(1/6)
constexpr float k1_3 = 0.3333333432674407958984375f;    // float32(1/3) = float32(2/6)
constexpr float k2_3 = 0.666666686534881591796875f;     // float32(2/3) = float32(4/6)
constexpr float k5_6 = 0.833333313465118408203125f;     // float32(5/6)

// rgbToHSV (color.go:178-200) of a colour's bytes through colorToHSV (color.go:124-127)
__device__ inline void hsv_of(uint32_t c, float& h, float& s, float& v) {
#pragma clang fp contract(off)
  const float r = (float)(c & 0xffu) / 255.f, g = (float)((c >> 8) & 0xffu) / 255.f, b = (float)((c >> 16) & 0xffu) / 255.f;
  const float xmax = __builtin_fmaxf(__builtin_fmaxf(r, g), b), xmin = __builtin_fminf(__builtin_fminf(r, g), b), cc = xmax - xmin;
  v = xmax;
  h = 0.f;
  if (cc == 0.f) h = 0.f;
  else if (v == r) h = (g - b) / (cc * 6.f);
  else if (v == g) h = k1_3 + (b - r) / (cc * 6.f);
  else if (v == b) h = k2_3 + (r - g) / (cc * 6.f);
  if (h < 0.f) h += 1.f;
  s = xmax > 0.f ? cc / xmax : 0.f;
}

// ColorConversionLinearGradient's closure for a pair other than black -> white (color.go:54-71; interpHSV, hsvToRGB, rgbToC)
__device__ inline uint32_t gradient(float d, const ColorConv& cv, float h0, float s0, float v0, float h1, float s1, float v1) {
#pragma clang fp contract(off)
  const float blend = d / cv.length + 0.5f;
  if (le(blend, 0.f)) return cv.c0;
  if (ge(blend, 1.f)) return cv.c1;
  if (h1 - h0 > 0.5f) h0 += 1.f;
  else if (h1 - h0 < -0.5f) h1 += 1.f;
  const float h = interp(h0, h1, blend), s = interp(s0, s1, blend), v = interp(v0, v1, blend);
  const float c = s * v;
  const float h6 = h * 6.f;
  // math32.Mod(h6, 2): the exact remainder (h6 / 2, its floor and twice that are exact; so is the difference), sign of h6
  const float ah = __builtin_fabsf(h6);
  const float md = __builtin_copysignf(ah - 2.f * __builtin_floorf(ah * 0.5f), h6);
  const float x = c * (1.f - __builtin_fabsf(md - 1.f));
  const float m = v - c;
  float r = 0.f, g = 0.f, b = 0.f;
  if (ge(h, 0.f) && le(h, k1_6)) { r = c; g = x; b = 0.f; }
  else if (gt(h, k1_6) && le(h, k1_3)) { r = x; g = c; b = 0.f; }
  else if (gt(h, k1_3) && le(h, 0.5f)) { r = 0.f; g = c; b = x; }
  else if (gt(h, 0.5f) && le(h, k2_3)) { r = 0.f; g = x; b = c; }
  else if (gt(h, k2_3) && le(h, k5_6)) { r = x; g = 0.f; b = c; }
  else if (gt(h, k5_6) && le(h, 1.f)) { r = c; g = 0.f; b = x; }
  r = r + m; g = g + m; b = b + m;
  return rgba(to_int_bits(clamp(r, 0.f, 1.f) * 255.f), to_int_bits(clamp(g, 0.f, 1.f) * 255.f), to_int_bits(clamp(b, 0.f, 1.f) * 255.f));
}

// blackAndWhiteLinearSmooth / blackAndWhiteNoSmoothing (color.go:73-99)
__device__ inline uint32_t bw(float d, float length) {
#pragma clang fp contract(off)
  if (length == 0.f) return lt(d, 0.f) ? 0xff000000u : 0xffffffffu;
  const float blend = d / length + 0.5f;
  if (le(blend, 0.f)) return 0xff000000u;
  if (ge(blend, 1.f)) return 0xffffffffu;
  const uint32_t y = to_int_bits(clamp(blend, 0.f, 1.f) * 255.f);
  return rgba(y, y, y);
}
}  // namespace pic

// ImageRendererSDF2.Render's lattice (image2_kernel) with a conversion of gsdfaux: rgba gets the converted pixels, dist (optional)
// the raw distances. KIND < 0: the kind is conv.kind.
template <int K, int KIND>
__global__ void __launch_bounds__(BLOCK, 3) image2_color_kernel(const uint32_t* __restrict__ code_g, int w, int h, float xmin, float ymax,
                                                                float dx, float dy, ColorConv conv, float* __restrict__ dist,
                                                                uint32_t* __restrict__ rgba) {
  code_ptr code = as_code(code_g);
  float* lds = g_smem + threadIdx.x;
  const int kind = KIND >= 0 ? KIND : conv.kind;
  // per-conversion constants (uniform): IQ's 1 / length, the gradient's end colours in HSV
  const float inv = 1.f / conv.length;
  float h0 = 0.f, s0 = 0.f, v0 = 0.f, h1 = 0.f, s1 = 0.f, v1 = 0.f;
  if (kind == 2) {
    pic::hsv_of(conv.c0, h0, s0, v0);
    pic::hsv_of(conv.c1, h1, s1, v1);
  }
  const uint64_t n = (uint64_t)w * (uint64_t)h;
  const uint64_t step = (uint64_t)gridDim.x * BLOCK * K;
  for (uint64_t base = (uint64_t)blockIdx.x * BLOCK * K; base < n; base += step) {
    P3 p[K];
    float d[K];
#pragma unroll
    for (int kp = 0; kp < K; kp++) {
      uint64_t i = base + (uint64_t)kp * BLOCK + threadIdx.x;
      if (i >= n) i = n - 1;
      const unsigned px = (unsigned)(i % (uint64_t)w), py = (unsigned)(i / (uint64_t)w);
      p[kp] = P3{(float)px * dx + xmin, ymax - (float)py * dy, 0.f};
    }
    gsdf_dev::sdf_eval<K>(code, p, d, lds, BLOCK);
#pragma unroll
    for (int kp = 0; kp < K; kp++) {
      const uint64_t i = base + (uint64_t)kp * BLOCK + threadIdx.x;
      if (i < n) {
        const float v = d[kp];
        if (dist) dist[i] = v;
        uint32_t c;
        if (kind == 1) c = pic::iq(v, inv);
        else if (kind == 2) c = pic::gradient(v, conv, h0, s0, v0, h1, s1, v1);
        else if (kind == 3) c = pic::bw(v, conv.length);
        else c = nb::nan_or_inf(v) ? 0xff0000ffu : (v > 0.f ? 0xffffffffu : 0xff000000u);  // image2_kernel's conversion
        if (rgba) rgba[i] = c;
      }
    }
  }
}
