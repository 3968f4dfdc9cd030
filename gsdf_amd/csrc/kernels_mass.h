// kernels_mass.h -- second moments: of an indexed mesh's shells (include/gsdf_hip.h, "indexed meshes: mass properties") and of loops
// ("contours: section properties"); tests/massref.py restates the arithmetic. One polynomial degree above the report's and the
// measures' sums, by their scheme: float64 terms, quantised at a power of two of the handle's exponent, summed as integers.
//   mass_second_kernel  a face per lane (abi_indexed.hip; after kernels_topo.h, with KERNELS_MASS_MESH defined): the face's shell from
//                       the report's retained numbering, the six terms of the tetrahedron (0, a, b, c), each split and added to the
//                       shell's record through topo_wave / topo_add: twelve atomics from a wave inside one shell, per-lane atomics
//                       from a mixed one, the same integers either way
//   csect_kernel        a vertex per lane (abi_contour.hip; after kernels_contour_simplify.h, with KERNELS_MASS_LOOPS defined): the edge
//                       to its successor, five terms (first x y, second xx yy xy) per loop, cmeas_kernel's two paths
// Each unit compiles the kernel it launches and not the other: the helpers of the two sides live in headers that define kernels of
// their own unit. A term is computed, split and added before the next one is: six float64 products stay live at no point.
#pragma once
#include "kernels_common.h"

#ifdef KERNELS_MASS_MESH
struct MassShellAcc {
  unsigned long long sum[12];  // xx yy zz xy xz yz: low 32 bits summed, then the (signed) rest summed
};

// sc: 2^(62 - 5 e). shell_of_face: the report's (TOPO_NONE: a degenerate face). A face with a non-finite coordinate adds nothing.
__global__ void __launch_bounds__(BLOCK) mass_second_kernel(const float* __restrict__ verts, const unsigned* __restrict__ idx, unsigned long long n_tris,
                                                            const unsigned* __restrict__ shell_of_face, MassShellAcc* __restrict__ acc, double sc) {
#pragma clang fp contract(off)
  const unsigned long long f = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  unsigned shell = TOPO_NONE;
  bool finite = false;
  double a[3] = {0.0, 0.0, 0.0}, b[3] = {0.0, 0.0, 0.0}, c[3] = {0.0, 0.0, 0.0};
  if (f < n_tris) {
    shell = shell_of_face[f];
    if (shell != TOPO_NONE) {
      const unsigned ia = idx[3ull * f], ib = idx[3ull * f + 1ull], ic = idx[3ull * f + 2ull];
      float p[9];
#pragma unroll
      for (int k = 0; k < 3; k++) { p[k] = verts[3ull * ia + k]; p[3 + k] = verts[3ull * ib + k]; p[6 + k] = verts[3ull * ic + k]; }
      finite = true;
#pragma unroll
      for (int k = 0; k < 9; k++) finite = finite && (__float_as_uint(p[k]) & 0x7fffffffu) < 0x7f800000u;
#pragma unroll
      for (int k = 0; k < 3; k++) { a[k] = (double)p[k]; b[k] = (double)p[3 + k]; c[k] = (double)p[6 + k]; }
    }
  }
  double det = 0.0, s[3] = {0.0, 0.0, 0.0};
  if (finite) {
    const double mx = b[1] * c[2] - b[2] * c[1], my = b[2] * c[0] - b[0] * c[2], mz = b[0] * c[1] - b[1] * c[0];
    det = (a[0] * mx + a[1] * my) + a[2] * mz;
#pragma unroll
    for (int k = 0; k < 3; k++) s[k] = (a[k] + b[k]) + c[k];
  }
  const TopoWave w = topo_wave(shell);
#pragma unroll
  for (int k = 0; k < 6; k++) {
    const int i = k < 3 ? k : (k == 5 ? 1 : 0), j = k < 3 ? k : (k == 3 ? 1 : 2);
    unsigned long long lo = 0ull, hi = 0ull;
    if (finite) topo_split((det * (((a[i] * a[j] + b[i] * b[j]) + c[i] * c[j]) + s[i] * s[j])) / 120.0, sc, &lo, &hi);
    topo_add(w, shell, lo, acc, 2u * k);
    topo_add(w, shell, hi, acc, 2u * k + 1u);
  }
}
#endif  // KERNELS_MASS_MESH

#ifdef KERNELS_MASS_LOOPS
struct CsectAcc {
  unsigned long long sum[10];  // first x, first y, second xx, yy, xy: low 32 bits summed, then the (signed) rest summed
};

// *maxbits: cmeas_maxbits_kernel's result, as cmeas_kernel reads it; the scales 2^(62 - 3 e) and 2^(62 - 4 e). acc: zeroed.
__global__ void __launch_bounds__(BLOCK) csect_kernel(const float* __restrict__ xy, const unsigned* __restrict__ loop_start, const unsigned* __restrict__ loop_of,
                                                      unsigned n_verts, const unsigned long long* __restrict__ maxbits, CsectAcc* acc) {
#pragma clang fp contract(off)
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  const bool live = g < n_verts;
  unsigned q = CONTOUR_NONE;
  unsigned long long s[10];
#pragma unroll
  for (int k = 0; k < 10; k++) s[k] = 0ull;
  if (live) {
    const unsigned v = (unsigned)g;
    q = loop_of[v];
    const unsigned l0 = loop_start[q], l1 = loop_start[q + 1];
    const unsigned long long nx = v + 1u == l1 ? l0 : (unsigned long long)v + 1ull;
    const unsigned biased = (unsigned)(*maxbits >> 23);
    const int e = (int)(biased > 1u ? biased : 1u) - 126;
    const double x0 = (double)xy[2ull * v], y0 = (double)xy[2ull * v + 1ull], x1 = (double)xy[2ull * nx], y1 = (double)xy[2ull * nx + 1ull];
    const double cross = x0 * y1 - x1 * y0;  // (the measures' area term)
    const double sc1 = cmeas_pow2(62 - 3 * e), sc2 = cmeas_pow2(62 - 4 * e);
    cmeas_split((cross * (x0 + x1)) / 6.0, sc1, &s[0], &s[1]);
    cmeas_split((cross * (y0 + y1)) / 6.0, sc1, &s[2], &s[3]);
    cmeas_split((cross * ((x0 * x0 + x0 * x1) + x1 * x1)) / 12.0, sc2, &s[4], &s[5]);
    cmeas_split((cross * ((y0 * y0 + y0 * y1) + y1 * y1)) / 12.0, sc2, &s[6], &s[7]);
    cmeas_split((cross * (((x0 * y1 + x1 * y0) + 2.0 * (x0 * y0)) + 2.0 * (x1 * y1))) / 24.0, sc2, &s[8], &s[9]);
  }
  // a wave inside one loop: one atomic per word; a mixed wave: each lane's own
  const unsigned long long m = __ballot(live);
  if (m == 0ull) return;  // (the whole wave)
  const unsigned q0 = (unsigned)__shfl((int)q, __builtin_ctzll(m), 64);
  const bool uniform = __ballot(live && q != q0) == 0ull;
  if (uniform) {
#pragma unroll
    for (int k = 0; k < 10; k++) {
      const unsigned long long t = cmeas_wave_sum(s[k]);
      if ((threadIdx.x & 63u) == 0u && t) atomicAdd(&acc[q0].sum[k], t);
    }
  } else if (live) {
#pragma unroll
    for (int k = 0; k < 10; k++)
      if (s[k]) atomicAdd(&acc[q].sum[k], s[k]);
  }
}
#endif  // KERNELS_MASS_LOOPS
