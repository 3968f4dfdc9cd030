// mass_host.h -- the host side of "indexed meshes: mass properties" and "contours: section properties" (include/gsdf_hip.h states the
// arithmetic; tests/massref.py restates it): the devices' integer sums -> the records' float64 values, one rounding each, the derived
// values in the header's order, and the Jacobi iteration of gsdf_hip_inertia_principal. Plain C++, no HIP, no state: abi_indexed.hip,
// abi_contour.hip and abi_mass.cpp include it, and a stand-alone program can run it under a sanitiser.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#pragma GCC visibility push(default)  // (as abi_host.h includes it: whichever of the two comes first decides what the library exports)
#include "../../include/gsdf_hip.h"
#pragma GCC visibility pop

namespace mass {
// low-word sum and (signed) rest sum of quantised terms -> the integer they stand for
inline __int128 whole(unsigned long long lo, unsigned long long hi) { return (__int128)(long long)hi * ((__int128)1 << 32) + (__int128)lo; }
// that integer as float64 (one rounding, to nearest even) times 2^-shift (exact)
inline double value(__int128 t, int shift) { return std::ldexp((double)t, -shift); }
inline double quiet_nan() {
  const uint64_t q = 0x7ff8000000000000ull;
  double d;
  std::memcpy(&d, &q, 8);
  return d;
}

// sums: volume, first x y z, second xx yy zz xy xz yz (the integers of the contract, exponent e)
inline void fill_mass(gsdf_mass* m, const __int128 sums[10], int e, uint32_t label) {
  const double nan = quiet_nan();
  m->volume = value(sums[0], 62 - 3 * e);
  for (int k = 0; k < 3; k++) m->first[k] = value(sums[1 + k], 62 - 4 * e);
  for (int k = 0; k < 6; k++) m->second[k] = value(sums[4 + k], 62 - 5 * e);
  m->exponent = e;
  m->label = label;
  if (m->volume == 0.0) {
    for (int k = 0; k < 3; k++) m->centroid[k] = nan;
    for (int k = 0; k < 6; k++) m->inertia[k] = nan;
    return;
  }
  static const int I[6] = {0, 1, 2, 0, 0, 1}, J[6] = {0, 1, 2, 1, 2, 2};
  double c[6];
  for (int k = 0; k < 3; k++) m->centroid[k] = m->first[k] / m->volume;
  for (int k = 0; k < 6; k++) {
    const double p = m->first[I[k]] * m->first[J[k]];
    const double q = p / m->volume;
    c[k] = m->second[k] - q;
  }
  m->inertia[0] = c[1] + c[2];
  m->inertia[1] = c[0] + c[2];
  m->inertia[2] = c[0] + c[1];
  for (int k = 3; k < 6; k++) m->inertia[k] = -c[k];
}

// sums: twice the area (the measures' integer), first x y, second xx yy xy
inline void fill_section(gsdf_section* s, const __int128 sums[6], int e, uint32_t n_verts, uint32_t layer_or_n_loops) {
  const double nan = quiet_nan();
  s->area = std::ldexp((double)sums[0], 2 * e - 62);  // (the measures' own expression: the same bytes)
  for (int k = 0; k < 2; k++) s->first[k] = value(sums[1 + k], 62 - 3 * e);
  for (int k = 0; k < 3; k++) s->second[k] = value(sums[3 + k], 62 - 4 * e);
  s->n_verts = n_verts;
  s->layer_or_n_loops = layer_or_n_loops;
  if (s->area == 0.0) {
    for (int k = 0; k < 2; k++) s->centroid[k] = nan;
    for (int k = 0; k < 3; k++) s->central[k] = nan;
    return;
  }
  static const int I[3] = {0, 1, 0}, J[3] = {0, 1, 1};
  for (int k = 0; k < 2; k++) s->centroid[k] = s->first[k] / s->area;
  for (int k = 0; k < 3; k++) {
    const double p = s->first[I[k]] * s->first[J[k]];
    const double q = p / s->area;
    s->central[k] = s->second[k] - q;
  }
}

// The header's cyclic Jacobi iteration. false: a non-finite entry.
inline bool principal(const double inertia[6], double moments[3], double axes[9]) {
  for (int k = 0; k < 6; k++)
    if (!std::isfinite(inertia[k])) return false;
  double a[3][3] = {{inertia[0], inertia[3], inertia[4]}, {inertia[3], inertia[1], inertia[5]}, {inertia[4], inertia[5], inertia[2]}};
  double v[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
  static const int P[3] = {0, 0, 1}, Q[3] = {1, 2, 2}, R[3] = {2, 1, 0};
  for (int sweep = 0; sweep < 32; sweep++) {
    if (a[0][1] == 0.0 && a[0][2] == 0.0 && a[1][2] == 0.0) break;
    for (int k = 0; k < 3; k++) {
      const int p = P[k], q = Q[k], r = R[k];
      const double apq = a[p][q];
      if (apq == 0.0) continue;
      const double g = std::fabs(apq), dp = std::fabs(a[p][p]), dq = std::fabs(a[q][q]);
      if (dp + g == dp && dq + g == dq) {  // negligible beside both diagonal entries
        a[p][q] = a[q][p] = 0.0;
        continue;
      }
      const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
      const double root = std::sqrt(theta * theta + 1.0);
      const double t = (theta >= 0.0 ? 1.0 : -1.0) / (std::fabs(theta) + root);
      const double c = 1.0 / std::sqrt(t * t + 1.0);
      const double s = t * c;
      const double h = t * apq;
      a[p][p] = a[p][p] - h;
      a[q][q] = a[q][q] + h;
      a[p][q] = a[q][p] = 0.0;
      const double arp = a[r][p], arq = a[r][q];
      a[r][p] = a[p][r] = c * arp - s * arq;
      a[r][q] = a[q][r] = s * arp + c * arq;
      for (int i = 0; i < 3; i++) {
        const double vip = v[i][p], viq = v[i][q];
        v[i][p] = c * vip - s * viq;
        v[i][q] = s * vip + c * viq;
      }
    }
  }
  int ord[3] = {0, 1, 2};
  static const int S0[3] = {0, 1, 0}, S1[3] = {1, 2, 1};
  for (int k = 0; k < 3; k++)
    if (a[ord[S0[k]]][ord[S0[k]]] > a[ord[S1[k]]][ord[S1[k]]]) {
      const int t = ord[S0[k]];
      ord[S0[k]] = ord[S1[k]];
      ord[S1[k]] = t;
    }
  for (int k = 0; k < 3; k++) moments[k] = a[ord[k]][ord[k]];
  for (int k = 0; k < 2; k++) {
    double* x = axes + 3 * k;
    for (int i = 0; i < 3; i++) x[i] = v[i][ord[k]];
    int big = 0;
    for (int i = 1; i < 3; i++)
      if (std::fabs(x[i]) > std::fabs(x[big])) big = i;
    if (x[big] < 0.0)
      for (int i = 0; i < 3; i++) x[i] = -x[i];
  }
  const double *x = axes, *y = axes + 3;
  axes[6] = x[1] * y[2] - x[2] * y[1];
  axes[7] = x[2] * y[0] - x[0] * y[2];
  axes[8] = x[0] * y[1] - x[1] * y[0];
  return true;
}
}  // namespace mass
