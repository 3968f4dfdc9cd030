// kernels_offset.h -- the signed in-plane distance of a lattice to the loops of a gsdf_contour handle, for the offset of those loops
// (include/gsdf_hip.h, section "contours: offset", states the arithmetic; tests/offsetref.py restates it in numpy over every edge).
// After cloop_of_kernel (kernels_contour_simplify.h):
//   offset_bbox_kernel     a vertex per lane: the handle's exact xmin, ymin, xmax, ymax by order-preserving bits (integer min / max)
//   offset_edges_kernel    a vertex per lane: the edge to its successor in the loop as four floats (ax, ay, bx, by)
//   offset_tile_kernel     one workgroup per 16 x 16 tile of nodes per input layer: the layer's edges through LDS in batches of 256,
//                          an edge per lane tested against the tile (near: its box within the band of the tile's box; crossing: its
//                          y-span over the tile's rows and its largest x not left of the tile), the survivors compacted into two LDS
//                          lists, then every lane runs the float64 distance over the near list and the crossing count over the other
//                          for its own node -> D, and the two node statistics
//   offset_field_kernel    a node of an output layer per lane: fl(D + inset[i]) into the tracer's dist buffer
// Both culling tests are conservative (OFFSET_NEAR_MARGIN, OFFSET_X_MARGIN): an edge they drop cannot change a node's clamped distance
// or its crossing count, so the result equals the one over all edges, to the byte. A minimum and a parity do not depend on order:
// nothing here is order-dependent, and the only atomics are integer sums and integer min / max.
#pragma once
#include "kernels_common.h"
#include "kernels_contour.h"

#define OFFSET_TILE 16u
#define OFFSET_MAX_INSETS 8u
// the band grown by 2^-12: |wx|, |ex| <= 2^31 res <= 2^30 band, so the roundings of q (those of w, of h carried through h ex, of the
// product and of the difference: a few units of 2^-53 relative to them) stay below 2^-20 band, and those of d2 and the square root
// below 2^-50 of the value
#define OFFSET_NEAR_MARGIN 0.000244140625
// x_c lies between a_x and b_x up to 2^-52 (|a_x| + |b_x|); 2^-40 of that sum covers it
#define OFFSET_X_MARGIN 9.094947017729282e-13

struct OffsetCounters {
  unsigned long long inside_nodes, band_nodes;
};

struct OffsetInsets {
  float v[OFFSET_MAX_INSETS];
};

// order-preserving bits of a float (the measures' scheme): a < b as floats iff ordered(a) < ordered(b) as integers
__device__ __forceinline__ unsigned offset_ordered(float f) {
  const unsigned b = __float_as_uint(f);
  return (b >> 31) ? ~b : (b ^ 0x80000000u);
}

// bb: ordered bits of xmin, ymin (initialised to 0xffffffff) and xmax, ymax (to 0)
__global__ void __launch_bounds__(BLOCK) offset_bbox_kernel(const float* __restrict__ xy, unsigned n_verts, unsigned* __restrict__ bb) {
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  unsigned lo_x = 0xffffffffu, lo_y = 0xffffffffu, hi_x = 0u, hi_y = 0u;
  if (g < n_verts) {
    lo_x = hi_x = offset_ordered(xy[2ull * g]);
    lo_y = hi_y = offset_ordered(xy[2ull * g + 1ull]);
  }
  hi_x = nb::wave_max_u32(hi_x);
  hi_y = nb::wave_max_u32(hi_y);
  lo_x = ~nb::wave_max_u32(~lo_x);
  lo_y = ~nb::wave_max_u32(~lo_y);
  if ((threadIdx.x & 63u) == 0u) {
    atomicMin(&bb[0], lo_x);
    atomicMin(&bb[1], lo_y);
    atomicMax(&bb[2], hi_x);
    atomicMax(&bb[3], hi_y);
  }
}

__global__ void __launch_bounds__(BLOCK) offset_edges_kernel(const float* __restrict__ xy, const unsigned* __restrict__ loop_start, const unsigned* __restrict__ loop_of,
                                                             unsigned n_verts, float4* __restrict__ edges) {
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= n_verts) return;
  const unsigned v = (unsigned)g, q = loop_of[v], l0 = loop_start[q], l1 = loop_start[q + 1];
  const unsigned long long nx = v + 1u == l1 ? l0 : (unsigned long long)v + 1ull;
  edges[v] = make_float4(xy[2ull * v], xy[2ull * v + 1ull], xy[2ull * nx], xy[2ull * nx + 1ull]);
}

// Workgroup b: tile b % (tiles_x tiles_y) of input layer layer0 + b / (tiles_x tiles_y) of the chunk; lane t: node (i0 + t % 16,
// j0 + t / 16). layer_edge[l] .. layer_edge[l + 1] are the edges (tail vertex numbers) of input layer l of the HANDLE. D: the chunk's
// lattices, layer after layer.
__global__ void __launch_bounds__(BLOCK) offset_tile_kernel(ContourLattice lat, const float4* __restrict__ edges, const unsigned* __restrict__ layer_edge, unsigned layer0,
                                                            unsigned tiles_x, unsigned tiles_y, float band, float* __restrict__ D, OffsetCounters* __restrict__ ctr) {
#pragma clang fp contract(off)
  __shared__ float4 s_near[BLOCK], s_cross[BLOCK];
  __shared__ unsigned s_wa[4], s_wb[4];
  const unsigned per_layer = tiles_x * tiles_y;
  const unsigned cl = blockIdx.x / per_layer, tile = blockIdx.x % per_layer;
  const unsigned i0 = (tile % tiles_x) * OFFSET_TILE, j0 = (tile / tiles_x) * OFFSET_TILE;
  const unsigned i = i0 + (threadIdx.x & (OFFSET_TILE - 1u)), j = j0 + threadIdx.x / OFFSET_TILE;
  const bool live = i < lat.nx && j < lat.ny;
  const unsigned i1 = i0 + OFFSET_TILE - 1u < lat.nx ? i0 + OFFSET_TILE - 1u : lat.nx - 1u;
  const unsigned j1 = j0 + OFFSET_TILE - 1u < lat.ny ? j0 + OFFSET_TILE - 1u : lat.ny - 1u;
  // the tile's box: the coordinates are non-decreasing in the index (every step of x_i is a monotone rounding)
  const double tx0 = (double)contour_coord(lat.x0, i0, lat.res), tx1 = (double)contour_coord(lat.x0, i1, lat.res);
  const double ty0 = (double)contour_coord(lat.y0, j0, lat.res), ty1 = (double)contour_coord(lat.y0, j1, lat.res);
  const double reach = (double)band + (double)band * OFFSET_NEAR_MARGIN;
  const double px = (double)contour_coord(lat.x0, i, lat.res), py = (double)contour_coord(lat.y0, j, lat.res);
  const unsigned e0 = layer_edge[layer0 + cl], e1 = layer_edge[layer0 + cl + 1u];
  double m2 = __builtin_inf();
  unsigned crossings = 0u;
  for (unsigned base = e0; base < e1; base += BLOCK) {
    const unsigned e = base + threadIdx.x;
    bool near = false, cross = false;
    float4 ed = make_float4(0.f, 0.f, 0.f, 0.f);
    if (e < e1) {
      ed = edges[e];
      const double ax = (double)ed.x, ay = (double)ed.y, bx = (double)ed.z, by = (double)ed.w;
      const double ex0 = ax < bx ? ax : bx, ex1 = ax < bx ? bx : ax, ey0 = ay < by ? ay : by, ey1 = ay < by ? by : ay;
      near = ex0 <= tx1 + reach && ex1 >= tx0 - reach && ey0 <= ty1 + reach && ey1 >= ty0 - reach;
      // some row of the tile with lo < y <= hi, and x_c can come out right of the tile's first column
      cross = ey0 < ty1 && ey1 >= ty0 && ex1 + (__builtin_fabs(ax) + __builtin_fabs(bx)) * OFFSET_X_MARGIN >= tx0;
    }
    unsigned n_near, n_cross;
    const unsigned at_near = contour_block_excl(near ? 1u : 0u, s_wa, &n_near);
    const unsigned at_cross = contour_block_excl(cross ? 1u : 0u, s_wb, &n_cross);
    if (near) s_near[at_near] = ed;
    if (cross) s_cross[at_cross] = ed;
    __syncthreads();
    if (live) {
      for (unsigned k = 0; k < n_near; k++) {
        const float4 q = s_near[k];
        const double ax = (double)q.x, ay = (double)q.y;
        const double ex = (double)q.z - ax, ey = (double)q.w - ay;
        const double wx = px - ax, wy = py - ay;
        const double ee = ex * ex + ey * ey;
        double h = 0.0;
        if (ee > 0.0) {
          h = (wx * ex + wy * ey) / ee;
          h = h > 0.0 ? h : 0.0;
          h = h < 1.0 ? h : 1.0;
        }
        const double qx = wx - h * ex, qy = wy - h * ey;
        const double d2 = qx * qx + qy * qy;
        m2 = d2 < m2 ? d2 : m2;
      }
      for (unsigned k = 0; k < n_cross; k++) {
        const float4 q = s_cross[k];
        const double ax = (double)q.x, ay = (double)q.y, bx = (double)q.z, by = (double)q.w;
        if ((ay < py) != (by < py)) {
          const double t = (py - ay) / (by - ay);
          const double xc = ax + t * (bx - ax);
          crossings += xc > px ? 1u : 0u;
        }
      }
    }
    __syncthreads();  // (the lists and the scan's words are written again in the next batch)
  }
  bool inside = false, in_band = false;
  if (live) {
    const double r = __builtin_sqrt(m2), b = (double)band;
    const double a = r < b ? r : b;
    inside = (crossings & 1u) != 0u;
    in_band = a < b;
    D[(unsigned long long)cl * lat.nx * lat.ny + (unsigned long long)j * lat.nx + i] = (float)(inside ? -a : a);
  }
  contour_tally(inside, &ctr->inside_nodes);
  contour_tally(in_band, &ctr->band_nodes);
}

// output layer (l, i) of the chunk = its input layer l with inset i: f = fl(D + inset[i]); n_nodes = layers n_insets nx ny
__global__ void __launch_bounds__(BLOCK) offset_field_kernel(const float* __restrict__ D, unsigned per_layer, unsigned n_insets, OffsetInsets insets, unsigned long long n_nodes,
                                                             float* __restrict__ dist) {
  const unsigned long long g = (unsigned long long)blockIdx.x * BLOCK + threadIdx.x;
  if (g >= n_nodes) return;
  const unsigned long long ol = g / per_layer;
  const unsigned n = (unsigned)(g % per_layer), k = (unsigned)(ol % n_insets);
  float inset = insets.v[0];
#pragma unroll
  for (unsigned q = 1; q < OFFSET_MAX_INSETS; q++) inset = k == q ? insets.v[q] : inset;
  dist[g] = D[(ol / n_insets) * per_layer + n] + inset;
}
