/*
 * gsdf_seams.h -- which seams of an array node may make the field jump (host only).
 *
 * Array / Array2D evaluate their child in the point's own cell and in the nearer neighbour per axis (clamped to the
 * array's extent), CircularArray / CircularArray2D in the two copies that sit on the rays bounding the point's sector, and
 * keep the minimum. The SET of copies changes when the point crosses a cell-centre plane (neighbour id - 1 becomes id + 1)
 * or a sector ray (copy k - 1 becomes k + 1). Across such a seam the field is continuous only if the copy that leaves and
 * the copy that enters give the same value there, or neither matters. The octree's interval evaluation (oracle/orc_eval.c:
 * lipctx; gsdf_amd/csrc/interp.h: LIP) bounds the field over a ball through the copies seen at its CENTRE, which says
 * nothing about a point across a seam that jumps: a ball that reaches one gets no bound at all.
 *
 * Proved here, structurally and conservatively (anything not listed counts as "may jump"):
 *   mirror symmetry   the child's field is invariant under the reflection in the seam (x_a -> -x_a in the cell's frame,
 *                     y -> -y in the frame of the copy on the ray): leaving and entering copy are mirror images there.
 *                     Followed through translations, rigid transforms, scales and the boolean nodes down to primitives
 *                     with that symmetry (a box turned by a quarter of pi about z with equal sides is its own mirror image).
 *                     Matrix entries and offsets are compared to GSDF_SEAM_TOL, the rounding of the sines the builder put
 *                     into them; the field itself is evaluated no more exactly than that.
 *   convexity         the first and last cell of an array axis see one neighbour only ({0} | {0, 1} at cell 0's centre):
 *                     continuous if the neighbour cannot win there, f(0, y, z) <= f(+-s, y, z). True for an exact distance
 *                     field of a convex shape that is mirror symmetric in that axis (a convex even function of x_a has its
 *                     minimum at 0).
 *   few copies        one cell along an axis: no seam. A circular array of one or two instances: one set of copies for
 *                     every sector. With fewer instances than divisions (and more than two) the rays of the first and the
 *                     last instance separate {last, 0} from {0, 1} resp. {last - 1, last}: may jump whatever the child is.
 *
 * One text for the device's host compiler (gsdf_amd/csrc/compile.cpp) and the oracle (oracle/orc_eval.c): the two must
 * take the same decision for every node. Whether the decision is RIGHT is tested against sampled balls
 * (tests/test_mesh_corpus_ref.py), not against a second copy of this text.
 */
#ifndef GSDF_SEAMS_H
#define GSDF_SEAMS_H
#include <math.h>
#include <stdint.h>

#include "gsdf_program.h"

#define GSDF_SEAM_TOL 2e-6

/* q -> l q + t in a node's frame (l row-major 3x3, orthogonal by construction); 2D nodes use the upper left 2x2 */
typedef struct { double l[9], t[3]; } gsdf_iso;
typedef struct { const gsdf_node* nodes; const uint32_t* links; const float* aux; } gsdf_seam_tree;

static inline int gsdf_seam_small(double v, double mag) { return fabs(v) <= GSDF_SEAM_TOL * (1.0 + mag); }
static inline int gsdf_seam_tsmall(const gsdf_iso* m, int dim, double mag) {
  for (int i = 0; i < dim; i++) if (!gsdf_seam_small(m->t[i], mag)) return 0;
  return 1;
}
/* l (dim x dim part) is a signed permutation to GSDF_SEAM_TOL: perm[i] = column of row i's unit entry */
static inline int gsdf_seam_perm(const gsdf_iso* m, int dim, int* perm) {
  for (int i = 0; i < dim; i++) {
    perm[i] = -1;
    for (int j = 0; j < dim; j++) {
      const double a = fabs(m->l[3 * i + j]);
      if (fabs(a - 1.0) <= GSDF_SEAM_TOL) { if (perm[i] >= 0) return 0; perm[i] = j; }
      else if (a > GSDF_SEAM_TOL) return 0;
    }
    if (perm[i] < 0) return 0;
  }
  return 1;
}
static inline int gsdf_seam_diag(const gsdf_iso* m, int dim) {
  int perm[3];
  if (!gsdf_seam_perm(m, dim, perm)) return 0;
  for (int i = 0; i < dim; i++) if (perm[i] != i) return 0;
  return 1;
}
/* l keeps the z axis (to sign) and so acts on the x,y plane alone */
static inline int gsdf_seam_zblock(const gsdf_iso* m) {
  return fabs(fabs(m->l[8]) - 1.0) <= GSDF_SEAM_TOL && fabs(m->l[2]) <= GSDF_SEAM_TOL && fabs(m->l[5]) <= GSDF_SEAM_TOL &&
         fabs(m->l[6]) <= GSDF_SEAM_TOL && fabs(m->l[7]) <= GSDF_SEAM_TOL;
}
/* a (row-major, row stride rs, dim x dim) is orthonormal to GSDF_SEAM_TOL */
static inline int gsdf_seam_orthonormal(const float* a, int rs, int dim) {
  for (int i = 0; i < dim; i++)
    for (int j = 0; j < dim; j++) {
      double acc = 0;
      for (int k = 0; k < dim; k++) acc += (double)a[rs * i + k] * (double)a[rs * j + k];
      if (fabs(acc - (i == j ? 1.0 : 0.0)) > 2 * GSDF_SEAM_TOL) return 0;
    }
  return 1;
}
/* the isometry seen from the frame q' = a q + b (a orthonormal, dim x dim, row stride rs): l' = a l a^T, t' = a t + b - l' b */
static inline void gsdf_seam_conj(const gsdf_iso* m, const float* a, int rs, const double* b, int dim, gsdf_iso* out) {
  double al[9];
  for (int i = 0; i < 9; i++) { out->l[i] = (i % 4 == 0) ? 1.0 : 0.0; al[i] = 0; }
  out->t[0] = out->t[1] = out->t[2] = 0;
  for (int i = 0; i < dim; i++)
    for (int j = 0; j < dim; j++) {
      double acc = 0;
      for (int k = 0; k < dim; k++) acc += (double)a[rs * i + k] * m->l[3 * k + j];
      al[3 * i + j] = acc;
    }
  for (int i = 0; i < dim; i++)
    for (int j = 0; j < dim; j++) {
      double acc = 0;
      for (int k = 0; k < dim; k++) acc += al[3 * i + k] * (double)a[rs * j + k];
      out->l[3 * i + j] = acc;
    }
  for (int i = 0; i < dim; i++) {
    double acc = b[i];
    for (int k = 0; k < dim; k++) acc += (double)a[rs * i + k] * m->t[k] - out->l[3 * i + k] * b[k];
    out->t[i] = acc;
  }
}
/* a translation by -d (q' = q - d): t' = l d + t - d */
static inline void gsdf_seam_shift(const gsdf_iso* m, const double* d, int dim, gsdf_iso* out) {
  *out = *m;
  for (int i = 0; i < dim; i++) {
    double acc = m->t[i] - d[i];
    for (int k = 0; k < dim; k++) acc += m->l[3 * i + k] * d[k];
    out->t[i] = acc;
  }
}

/* 1: the field of node ni is invariant under m, to rounding. mag = largest offset or size met on the way (the offsets'
 * tolerance is relative to it). depth guards against a malformed blob. */
static int gsdf_seam_invariant(const gsdf_seam_tree* tr, uint32_t ni, const gsdf_iso* m, double mag, int depth) {
  const gsdf_node* nd = &tr->nodes[ni];
  const float* P = nd->p;
  const int is2d = gsdf_op_is2d(nd->op), dim = is2d ? 2 : 3;
  int perm[3];
  gsdf_iso c;
  if (depth > 64) return 0;
#define GSDF_SEAM_CHILD(k) (tr->links[nd->link_off + (k)])
#define GSDF_SEAM_MAG(v) { const double a_ = fabs((double)(v)); if (a_ > mag) mag = a_; }
  switch (nd->op) {
    case GSDF_SPHERE: case GSDF_CIRCLE2D:
      GSDF_SEAM_MAG(P[0]);
      return gsdf_seam_tsmall(m, dim, mag);
    case GSDF_BOX: case GSDF_BOXFRAME: case GSDF_RECT2D:
      for (int i = 0; i < dim; i++) GSDF_SEAM_MAG(P[i]);
      if (!gsdf_seam_perm(m, dim, perm) || !gsdf_seam_tsmall(m, dim, mag)) return 0;
      for (int i = 0; i < dim; i++) if (P[perm[i]] != P[i]) return 0;
      return 1;
    case GSDF_TORUS: case GSDF_CYLINDER: /* bodies of revolution about z, mirror symmetric in z */
      GSDF_SEAM_MAG(P[0]); GSDF_SEAM_MAG(P[1]);
      return gsdf_seam_zblock(m) && gsdf_seam_tsmall(m, 3, mag);
    case GSDF_HEX: case GSDF_HEX2D: case GSDF_DIAMOND2D: case GSDF_X2D: case GSDF_OCT2D: case GSDF_ELLIPSE2D: /* functions of |x|, |y| (, |z|) */
      GSDF_SEAM_MAG(P[0]); GSDF_SEAM_MAG(P[1]);
      return gsdf_seam_diag(m, dim) && gsdf_seam_tsmall(m, dim, mag);
    case GSDF_EQTRI2D: case GSDF_ARC2D: /* functions of |x| and y */
      GSDF_SEAM_MAG(P[0]);
      return gsdf_seam_diag(m, 2) && m->l[4] > 0 && gsdf_seam_tsmall(m, 2, mag);
    case GSDF_UNION: case GSDF_INTERSECT: case GSDF_DIFF: case GSDF_XOR: case GSDF_SMOOTH_UNION: case GSDF_SMOOTH_DIFF:
    case GSDF_SMOOTH_INTERSECT: case GSDF_UNION2D: case GSDF_INTERSECT2D: case GSDF_DIFF2D: case GSDF_XOR2D:
      for (uint32_t k = 0; k < nd->nchild; k++)
        if (!gsdf_seam_invariant(tr, GSDF_SEAM_CHILD(k), m, mag, depth + 1)) return 0;
      return nd->nchild > 0;
    case GSDF_OFFSET: case GSDF_OFFSET2D: case GSDF_ANNULUS2D:
      return nd->nchild == 1 && gsdf_seam_invariant(tr, GSDF_SEAM_CHILD(0), m, mag, depth + 1);
    case GSDF_SCALE: case GSDF_SHELL: case GSDF_SCALE2D: /* q' = q / f */
      if (nd->nchild != 1 || !(P[0] != 0.0f)) return 0;
      c = *m;
      for (int i = 0; i < dim; i++) c.t[i] = m->t[i] / (double)P[0];
      return gsdf_seam_invariant(tr, GSDF_SEAM_CHILD(0), &c, mag / fabs((double)P[0]), depth + 1);
    case GSDF_ELONGATE: case GSDF_ELONGATE2D: /* a function of |x|, |y| (, |z|) whatever the child is */
      for (int i = 0; i < dim; i++) GSDF_SEAM_MAG(P[i]);
      return gsdf_seam_diag(m, dim) && gsdf_seam_tsmall(m, dim, mag);
    case GSDF_SYMMETRY: case GSDF_SYMMETRY2D: { /* folded axes: any sign, no offset; the others pass through */
      if (nd->nchild != 1 || !gsdf_seam_diag(m, dim)) return 0;
      const int bits = (int)P[0];
      c = *m;
      for (int i = 0; i < dim; i++)
        if (bits & (1 << i)) {
          if (!gsdf_seam_small(m->t[i], mag)) return 0;
          c.l[4 * i] = 1.0; c.t[i] = 0.0;
        }
      return gsdf_seam_invariant(tr, GSDF_SEAM_CHILD(0), &c, mag, depth + 1);
    }
    case GSDF_TRANSLATE: case GSDF_TRANSLATE2D: {
      if (nd->nchild != 1) return 0;
      double d[3] = {P[0], P[1], is2d ? 0.0 : P[2]};
      for (int i = 0; i < dim; i++) GSDF_SEAM_MAG(d[i]);
      gsdf_seam_shift(m, d, dim, &c);
      return gsdf_seam_invariant(tr, GSDF_SEAM_CHILD(0), &c, mag, depth + 1);
    }
    case GSDF_TRANSFORM: { /* q' = a q + b, rows of the 4x4 */
      if (nd->nchild != 1 || nd->aux_len < 16) return 0;
      const float* a = &tr->aux[nd->aux_off];
      if (!gsdf_seam_orthonormal(a, 4, 3)) return 0;
      double b[3] = {a[3], a[7], a[11]};
      for (int i = 0; i < 3; i++) GSDF_SEAM_MAG(b[i]);
      gsdf_seam_conj(m, a, 4, b, 3, &c);
      return gsdf_seam_invariant(tr, GSDF_SEAM_CHILD(0), &c, mag, depth + 1);
    }
    case GSDF_ROTATION2D: {
      if (nd->nchild != 1 || !gsdf_seam_orthonormal(P, 2, 2)) return 0;
      double b[2] = {0, 0};
      gsdf_seam_conj(m, P, 2, b, 2, &c);
      return gsdf_seam_invariant(tr, GSDF_SEAM_CHILD(0), &c, mag, depth + 1);
    }
    case GSDF_EXTRUSION: /* a function of the child's field at (x, y) and of |z| */
      GSDF_SEAM_MAG(P[0]);
      if (nd->nchild != 1 || !gsdf_seam_zblock(m) || !gsdf_seam_small(m->t[2], mag)) return 0;
      c = *m;
      c.l[8] = 1.0; c.t[2] = 0.0;
      return gsdf_seam_invariant(tr, GSDF_SEAM_CHILD(0), &c, mag, depth + 1);
    default: /* polygons and lines, twist, screw, revolution, nested arrays: not followed */
      return 0;
  }
#undef GSDF_SEAM_MAG
}

/* 1: node ni's field is the exact distance field of a convex shape (a convex function) */
static int gsdf_seam_convex(const gsdf_seam_tree* tr, uint32_t ni, int depth) {
  const gsdf_node* nd = &tr->nodes[ni];
  if (depth > 64) return 0;
  switch (nd->op) {
    case GSDF_SPHERE: case GSDF_BOX: case GSDF_CYLINDER: case GSDF_HEX:
    case GSDF_CIRCLE2D: case GSDF_RECT2D: case GSDF_HEX2D: case GSDF_OCT2D: case GSDF_EQTRI2D: case GSDF_DIAMOND2D:
      return 1;
    case GSDF_INTERSECT: case GSDF_INTERSECT2D: /* a maximum of convex functions */
      for (uint32_t k = 0; k < nd->nchild; k++)
        if (!gsdf_seam_convex(tr, GSDF_SEAM_CHILD(k), depth + 1)) return 0;
      return nd->nchild > 0;
    case GSDF_SCALE: case GSDF_SCALE2D:
      return nd->nchild == 1 && nd->p[0] > 0.0f && gsdf_seam_convex(tr, GSDF_SEAM_CHILD(0), depth + 1);
    case GSDF_TRANSLATE: case GSDF_TRANSLATE2D: case GSDF_TRANSFORM: case GSDF_ROTATION2D: case GSDF_OFFSET: case GSDF_OFFSET2D:
    case GSDF_EXTRUSION: /* affine maps of the position, a constant added; a prism over a convex outline */
      return nd->nchild == 1 && gsdf_seam_convex(tr, GSDF_SEAM_CHILD(0), depth + 1);
    default:
      return 0;
  }
}
#undef GSDF_SEAM_CHILD

/* Array / Array2D node ni: bit a set = a ball that reaches a cell-centre plane of axis a gets no bound */
static inline unsigned gsdf_array_seams(const gsdf_seam_tree* tr, uint32_t ni) {
  const gsdf_node* nd = &tr->nodes[ni];
  const int dim = nd->op == GSDF_ARRAY2D ? 2 : 3;
  if (nd->nchild != 1) return 0;
  const uint32_t child = tr->links[nd->link_off];
  const int convex = gsdf_seam_convex(tr, child, 0);
  unsigned mask = 0;
  for (int a = 0; a < dim; a++) {
    if (!(nd->p[dim + a] > 1.0f)) continue; /* one cell: every copy index clamps to 0 */
    gsdf_iso m;
    for (int i = 0; i < 9; i++) m.l[i] = (i % 4 == 0) ? 1.0 : 0.0;
    m.t[0] = m.t[1] = m.t[2] = 0;
    m.l[4 * a] = -1.0;
    if (!(convex && gsdf_seam_invariant(tr, child, &m, 0.0, 0))) mask |= 1u << a;
  }
  return mask;
}
/* CircularArray / CircularArray2D node ni: 1 = a ball that reaches a ray bounding its sector gets no bound */
static inline int gsdf_circ_seams(const gsdf_seam_tree* tr, uint32_t ni) {
  const gsdf_node* nd = &tr->nodes[ni];
  if (nd->nchild != 1) return 0;
  const int ninst = (int)nd->p[0];
  if (ninst <= 2) return 0;
  if ((float)ninst < nd->p[1]) return 1;
  gsdf_iso m;
  for (int i = 0; i < 9; i++) m.l[i] = (i % 4 == 0) ? 1.0 : 0.0;
  m.t[0] = m.t[1] = m.t[2] = 0;
  m.l[4] = -1.0;
  return !gsdf_seam_invariant(tr, tr->links[nd->link_off], &m, 0.0, 0);
}
#endif
