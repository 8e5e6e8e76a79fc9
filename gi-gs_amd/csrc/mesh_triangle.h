// mesh_triangle.h -- the exact closest point of a triangle to a point, once: the d^2 that mesh_distance.hip's search compares
// and, with kWeights, the barycentric weights that mesh_atlas.hip's transfer lands a texel with.  One routine for both, so
// the transfer places a point by the candidates, expressions and order the search chose its face by.  include/gigs_hip.h,
// "Comparing meshes" and "Texturing meshes", states the quantities; float64, + - * / only.  Header-only.
#pragma once
#include "mesh_grid.h"

namespace gigs {
namespace mesh_common {

// d^2 from p to the segment a -> b; with kWeights, *s in [0, 1] is the place on it
template <bool kWeights>
__device__ __forceinline__ double segment_closest(const double* p, const double* a, const double* b, double* s) {
  double ab[3], ap[3];
#pragma unroll
  for (int c = 0; c < 3; c++) ab[c] = b[c] - a[c], ap[c] = p[c] - a[c];
  const double t = dot3(ap, ab), den = dot3(ab, ab);
  if (t <= 0.0) {
    if constexpr (kWeights) *s = 0.0;
    return dot3(ap, ap);
  }
  if (t >= den) {
    double bp[3];
#pragma unroll
    for (int c = 0; c < 3; c++) bp[c] = p[c] - b[c];
    if constexpr (kWeights) *s = 1.0;
    return dot3(bp, bp);
  }
  const double u = t / den;
  if constexpr (kWeights) *s = u;
  double q[3];
#pragma unroll
  for (int c = 0; c < 3; c++) q[c] = ap[c] - u * ab[c];
  return dot3(q, q);
}

// the edge from vertex (ia, a) to vertex (ib, b): d^2 and, with kWeights, the weights of a and of b.  Every segment is
// walked from its lower vertex index, so two faces that share an edge get the same bits from it.
template <bool kWeights>
__device__ __forceinline__ double edge_closest(const double* p, int ia, const double* a, int ib, const double* b, double* wa,
                                               double* wb) {
  double s;
  if (ia > ib) {
    const double d2 = segment_closest<kWeights>(p, b, a, &s);
    if constexpr (kWeights) *wb = 1.0 - s, *wa = s;
    return d2;
  }
  const double d2 = segment_closest<kWeights>(p, a, b, &s);
  if constexpr (kWeights) *wa = 1.0 - s, *wb = s;
  return d2;
}

__device__ __forceinline__ double edge_fn(const double* p, const double* a, const double* b, const double* n) {
  double ab[3], ap[3], c[3];
#pragma unroll
  for (int k = 0; k < 3; k++) ab[k] = b[k] - a[k], ap[k] = p[k] - a[k];
  cross3(ab, ap, c);
  return dot3(c, n);
}

// d^2 from p to the triangle (p0, p1, p2) of vertex indices (i0, i1, i2): the least of the three edges and, inside the
// prism, the plane, in that order with a strict <.  With kWeights, *w0 *w1 *w2 are the weights of the winning candidate
// (finite inputs, so edge 01 always enters); without, they are not touched.
template <bool kWeights>
__device__ __forceinline__ double triangle_closest(const double* p, int i0, int i1, int i2, const double* p0, const double* p1,
                                                   const double* p2, double* w0 = nullptr, double* w1 = nullptr,
                                                   double* w2 = nullptr) {
  double d2 = INFINITY, wa, wb;
  if constexpr (kWeights) *w0 = 1.0, *w1 = 0.0, *w2 = 0.0;
  double s = edge_closest<kWeights>(p, i0, p0, i1, p1, &wa, &wb);
  if (s < d2) {
    d2 = s;
    if constexpr (kWeights) *w0 = wa, *w1 = wb, *w2 = 0.0;
  }
  s = edge_closest<kWeights>(p, i1, p1, i2, p2, &wa, &wb);
  if (s < d2) {
    d2 = s;
    if constexpr (kWeights) *w0 = 0.0, *w1 = wa, *w2 = wb;
  }
  s = edge_closest<kWeights>(p, i2, p2, i0, p0, &wa, &wb);
  if (s < d2) {
    d2 = s;
    if constexpr (kWeights) *w0 = wb, *w1 = 0.0, *w2 = wa;
  }
  double e1[3], e2[3], n[3], w[3];
#pragma unroll
  for (int c = 0; c < 3; c++) e1[c] = p1[c] - p0[c], e2[c] = p2[c] - p0[c], w[c] = p[c] - p0[c];
  cross3(e1, e2, n);
  // the same inside test both ways: the weights need all three edge functions; the search, which needs none of them
  // again, stops at the first negative one -- the form its kernel was compiled and measured in
  if constexpr (kWeights) {
    const double f0 = edge_fn(p, p0, p1, n), f1 = edge_fn(p, p1, p2, n), f2 = edge_fn(p, p2, p0, n);
    if (f0 >= 0.0 && f1 >= 0.0 && f2 >= 0.0) {
      const double h = dot3(w, n);
      const double plane = h * h / dot3(n, n);
      const double W = (f0 + f1) + f2;
      if (plane < d2 && W > 0.0) {  // a NaN (n = 0) loses
        d2 = plane;
        *w0 = f1 / W;  // the edge function of an edge weighs the vertex opposite
        *w1 = f2 / W;
        *w2 = f0 / W;
      }
    }
  } else if (edge_fn(p, p0, p1, n) >= 0.0 && edge_fn(p, p1, p2, n) >= 0.0 && edge_fn(p, p2, p0, n) >= 0.0) {
    const double h = dot3(w, n);
    const double plane = h * h / dot3(n, n);
    if (plane < d2) d2 = plane;  // a NaN (n = 0) loses
  }
  return d2;
}

}  // namespace mesh_common
}  // namespace gigs
