// mesh_ray.h -- what mesh_raycast.hip, mesh_light.hip, mesh_gather.hip, mesh_reflect.hip and mesh_shadow.hip share: the ray against one face, the
// slab traversal of the triangle grid (include/gigs_hip.h, "Baking occlusion", 2 to 7) and its any-hit form, the hemisphere of a vertex (8: the no_normal rule, the
// basis of Duff et al., the origin, the rotation and the direction of a table row) and the sky texel of a direction ("Baking
// light", 3).  Header-only; nothing here is a symbol of the
// library.  float64 on the float32 inputs, + - * / only, and the library is built with -ffp-contract=off.
#pragma once
#include "mesh_grid.h"

namespace gigs {
namespace mesh_raycast {

using namespace gigs::mesh_common;    // item, in_range, finite3, dot3, cross3, load3, mix64, blocks_for
using namespace gigs::mesh_distance;  // Grid, cell_at, plane_at, make_grid

constexpr double kGuard = 0x1p-40;  // a face is a candidate only if dn^2 > kGuard (d.d)(n.n)
constexpr double kSlack = 0x1p-26;  // sigma = kSlack (M + max |o_a|)
constexpr unsigned kWave = 64;

struct MeshView {
  Grid g;
  int V, F;
  const float* vertices;
  const int* faces;
  const long long *cell_start, *pairs;
  long long n_pairs;
  double M;  // the largest |coordinate| of a corner of a usable face: the scale of sigma
};

struct Hit {
  double t, w1, w2, sum;
  int face;
};

// w of the edge a -> b (a, b: the two ends minus the ray's origin): the ends are taken in ascending vertex index, so two
// faces that share an edge compute the same bits with opposite signs
__device__ __forceinline__ double edge_w(const double* d, int ia, const double* a, int ib, const double* b) {
  double c[3];
  if (ia < ib) {
    cross3(a, b, c);
    return dot3(d, c);
  }
  cross3(b, a, c);
  return -dot3(d, c);
}

__device__ __forceinline__ double min3(double a, double b, double c) { return fmin(a, fmin(b, c)); }
__device__ __forceinline__ double max3(double a, double b, double c) { return fmax(a, fmax(b, c)); }

// the ray (o, d) against one face; true if the face is accepted, then h->t, w1, w2, sum are its
__device__ __forceinline__ bool ray_triangle(const double* o, const double* d, double dd, double sigma, double tmax,
                                             const int* idx, const double* p0, const double* p1, const double* p2, Hit* h) {
  double a0[3], a1[3], a2[3];
#pragma unroll
  for (int c = 0; c < 3; c++) a0[c] = p0[c] - o[c], a1[c] = p1[c] - o[c], a2[c] = p2[c] - o[c];
  const double w0 = edge_w(d, idx[1], a1, idx[2], a2);
  const double w1 = edge_w(d, idx[2], a2, idx[0], a0);
  const double w2 = edge_w(d, idx[0], a0, idx[1], a1);
  const bool pos = w0 >= 0.0 && w1 >= 0.0 && w2 >= 0.0, neg = w0 <= 0.0 && w1 <= 0.0 && w2 <= 0.0;
  if (!(pos || neg) || (pos && neg)) return false;  // pos && neg: all three are zero
  double e1[3], e2[3], n[3];
#pragma unroll
  for (int c = 0; c < 3; c++) e1[c] = p1[c] - p0[c], e2[c] = p2[c] - p0[c];
  cross3(e1, e2, n);
  const double dn = dot3(d, n);
  if (!(dn * dn > kGuard * (dd * dot3(n, n)))) return false;
  const double t = dot3(a0, n) / dn;
  if (!(t >= 0.0 && t <= tmax)) return false;
#pragma unroll
  for (int c = 0; c < 3; c++) {  // the hit point lies in the face's box, widened by sigma
    const double x = o[c] + t * d[c];
    if (!(x >= min3(p0[c], p1[c], p2[c]) - sigma && x <= max3(p0[c], p1[c], p2[c]) + sigma)) return false;
  }
  h->t = t, h->w1 = w1, h->w2 = w2, h->sum = (w0 + w1) + w2;
  return true;
}

__device__ __forceinline__ double pick(const double* p, int a) { return a == 0 ? p[0] : (a == 1 ? p[1] : p[2]); }
__device__ __forceinline__ int pick(const int* p, int a) { return a == 0 ? p[0] : (a == 1 ? p[1] : p[2]); }

// The nearest accepted face of the ray, by slabs along its dominant axis.  *best: t = +inf, face = -1 on entry.  Returns
// false if an index left its range.
__device__ __forceinline__ bool traverse(const MeshView& m, const double* o, const double* d, double tmax, Hit* best) {
  const Grid& g = m.g;
  const double ax = fabs(d[0]), ay = fabs(d[1]), az = fabs(d[2]);
  const int A = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2), U = A == 2 ? 0 : A + 1, W = A == 0 ? 2 : A - 1;
  const double oA = pick(o, A), dA = pick(d, A), oU = pick(o, U), dU = pick(d, U), oW = pick(o, W), dW = pick(d, W);
  const double loA = pick(g.lo, A), loU = pick(g.lo, U), loW = pick(g.lo, W), cell = g.cell;
  const int GA = pick(g.G, A), GU = pick(g.G, U), GW = pick(g.G, W);
  const int stride[3] = {1, g.G[0], g.G[0] * g.G[1]};
  const int sA = pick(stride, A), sU = pick(stride, U), sW = pick(stride, W);
  const double sigma = kSlack * (m.M + max3(fabs(o[0]), fabs(o[1]), fabs(o[2])));
  const double s2 = 2.0 * sigma, s3 = 3.0 * sigma;
  const double dd = dot3(d, d);
  const bool up = dA > 0.0;
  const int step = up ? 1 : -1;
  bool ok = true;
  for (int k = cell_at(loA, cell, GA, up ? oA - s3 : oA + s3); k >= 0 && k < GA; k += step) {
    const double ta = ((plane_at(loA, cell, k) - s2) - oA) / dA, tb = ((plane_at(loA, cell, k + 1) + s2) - oA) / dA;
    double tn = fmin(ta, tb), tf = fmax(ta, tb);
    if (tf < 0.0) continue;                 // the slab lies behind the origin
    if (tn > tmax || best->t < tn) break;  // every later slab starts later still
    tn = fmax(tn, 0.0), tf = fmin(tf, tmax);
    const double u_n = oU + tn * dU, u_f = oU + tf * dU, w_n = oW + tn * dW, w_f = oW + tf * dW;
    const int u0 = cell_at(loU, cell, GU, fmin(u_n, u_f) - s2), u1 = cell_at(loU, cell, GU, fmax(u_n, u_f) + s2);
    const int w0 = cell_at(loW, cell, GW, fmin(w_n, w_f) - s2), w1 = cell_at(loW, cell, GW, fmax(w_n, w_f) + s2);
    for (int w = w0; w <= w1; w++)
      for (int u = u0; u <= u1; u++) {
        const long long c = (long long)k * sA + (long long)u * sU + (long long)w * sW;
        const long long s = m.cell_start[c], e = m.cell_start[c + 1];
        if (s < 0 || e < s || e > m.n_pairs) {
          ok = false;
          continue;
        }
        for (long long r = s; r < e; r++) {
          const long long key = m.pairs[r];
          const long long f = key & 0xffffffffLL;
          if ((key >> 32) != c || f >= m.F) {
            ok = false;
            continue;
          }
          const int idx[3] = {m.faces[3 * (size_t)f], m.faces[3 * (size_t)f + 1], m.faces[3 * (size_t)f + 2]};
          if (!in_range(idx[0], idx[1], idx[2], m.V)) {
            ok = false;
            continue;
          }
          double p0[3], p1[3], p2[3];
          load3(m.vertices, idx[0], p0);
          load3(m.vertices, idx[1], p1);
          load3(m.vertices, idx[2], p2);
          Hit h;
          if (ray_triangle(o, d, dd, sigma, tmax, idx, p0, p1, p2, &h) &&
              (h.t < best->t || (h.t == best->t && (int)f < best->face))) {
            *best = h;
            best->face = (int)f;
          }
        }
      }
  }
  return ok;
}

// Any hit: true iff the ray has an accepted face within tmax, i.e. iff traverse() would leave best->face >= 0 (DESIGN.md,
// "Analytic lights and shadows", has the proof).  The slab walk, the range checks and ray_triangle are traverse()'s; the
// walk returns at the first accepted face and keeps no nearest one.  *ok (true on entry) turns false if an index left its
// range before that.
__device__ __forceinline__ bool occluded(const MeshView& m, const double* o, const double* d, double tmax, bool* ok) {
  const Grid& g = m.g;
  const double ax = fabs(d[0]), ay = fabs(d[1]), az = fabs(d[2]);
  const int A = (ax >= ay && ax >= az) ? 0 : (ay >= az ? 1 : 2), U = A == 2 ? 0 : A + 1, W = A == 0 ? 2 : A - 1;
  const double oA = pick(o, A), dA = pick(d, A), oU = pick(o, U), dU = pick(d, U), oW = pick(o, W), dW = pick(d, W);
  const double loA = pick(g.lo, A), loU = pick(g.lo, U), loW = pick(g.lo, W), cell = g.cell;
  const int GA = pick(g.G, A), GU = pick(g.G, U), GW = pick(g.G, W);
  const int stride[3] = {1, g.G[0], g.G[0] * g.G[1]};
  const int sA = pick(stride, A), sU = pick(stride, U), sW = pick(stride, W);
  const double sigma = kSlack * (m.M + max3(fabs(o[0]), fabs(o[1]), fabs(o[2])));
  const double s2 = 2.0 * sigma, s3 = 3.0 * sigma;
  const double dd = dot3(d, d);
  const bool up = dA > 0.0;
  const int step = up ? 1 : -1;
  for (int k = cell_at(loA, cell, GA, up ? oA - s3 : oA + s3); k >= 0 && k < GA; k += step) {
    const double ta = ((plane_at(loA, cell, k) - s2) - oA) / dA, tb = ((plane_at(loA, cell, k + 1) + s2) - oA) / dA;
    double tn = fmin(ta, tb), tf = fmax(ta, tb);
    if (tf < 0.0) continue;  // the slab lies behind the origin
    if (tn > tmax) break;    // every later slab starts later still
    tn = fmax(tn, 0.0), tf = fmin(tf, tmax);
    const double u_n = oU + tn * dU, u_f = oU + tf * dU, w_n = oW + tn * dW, w_f = oW + tf * dW;
    const int u0 = cell_at(loU, cell, GU, fmin(u_n, u_f) - s2), u1 = cell_at(loU, cell, GU, fmax(u_n, u_f) + s2);
    const int w0 = cell_at(loW, cell, GW, fmin(w_n, w_f) - s2), w1 = cell_at(loW, cell, GW, fmax(w_n, w_f) + s2);
    for (int w = w0; w <= w1; w++)
      for (int u = u0; u <= u1; u++) {
        const long long c = (long long)k * sA + (long long)u * sU + (long long)w * sW;
        const long long s = m.cell_start[c], e = m.cell_start[c + 1];
        if (s < 0 || e < s || e > m.n_pairs) {
          *ok = false;
          continue;
        }
        for (long long r = s; r < e; r++) {
          const long long key = m.pairs[r];
          const long long f = key & 0xffffffffLL;
          if ((key >> 32) != c || f >= m.F) {
            *ok = false;
            continue;
          }
          const int idx[3] = {m.faces[3 * (size_t)f], m.faces[3 * (size_t)f + 1], m.faces[3 * (size_t)f + 2]};
          if (!in_range(idx[0], idx[1], idx[2], m.V)) {
            *ok = false;
            continue;
          }
          double p0[3], p1[3], p2[3];
          load3(m.vertices, idx[0], p0);
          load3(m.vertices, idx[1], p1);
          load3(m.vertices, idx[2], p2);
          Hit h;
          if (ray_triangle(o, d, dd, sigma, tmax, idx, p0, p1, p2, &h)) return true;
        }
      }
  }
  return false;
}

// ---- the hemisphere of a vertex ("Baking occlusion", 8) -----------------------------------------------------------------------
struct Hemisphere {
  double n[3], T[3], B[3], o[3];
  const float* row;  // this lane's direction of the vertex's rotation, chunk 0; the next chunk is 3 kWave floats on
};

// false: the no_normal rule (a position that is not finite, a normal that is not of unit length within 2^-10)
__device__ __forceinline__ bool hemisphere(const float* vertices, const float* normals, const float* table, int R, int K,
                                           unsigned long long seed, double bias, long long v, unsigned lane, Hemisphere* h) {
  double p[3];
  load3(vertices, (int)v, p);
  load3(normals, (int)v, h->n);
  const double* n = h->n;
  const double n2 = dot3(n, n);
  if (!finite3(p) || !(n2 >= 1.0 - 0x1p-10 && n2 <= 1.0 + 0x1p-10)) return false;
  // the branch-free orthonormal basis of Duff et al. (2017)
  const double sign = copysign(1.0, n[2]);
  const double fa = -1.0 / (sign + n[2]);
  const double fb = (n[0] * n[1]) * fa;
  h->T[0] = 1.0 + ((sign * n[0]) * n[0]) * fa, h->T[1] = sign * fb, h->T[2] = (-sign) * n[0];
  h->B[0] = fb, h->B[1] = sign + (n[1] * n[1]) * fa, h->B[2] = -n[1];
#pragma unroll
  for (int c = 0; c < 3; c++) h->o[c] = p[c] + bias * n[c];
  const unsigned k = (unsigned)(mix64((seed << 32) + (unsigned long long)v) % (unsigned long long)K);
  h->row = table + 3 * ((size_t)k * R + lane);
  return true;
}

// the world direction of the table row `row` in the frame of h
__device__ __forceinline__ void hemisphere_direction(const Hemisphere& h, const float* row, double* d) {
  const double x = (double)row[0], y = (double)row[1], z = (double)row[2];
#pragma unroll
  for (int c = 0; c < 3; c++) d[c] = (x * h.T[c] + y * h.B[c]) + z * h.n[c];
}

// ---- the sky of a direction ("Baking light", 3): shared by mesh_light.hip, mesh_gather.hip and mesh_reflect.hip ----------------
// the texel of u in [0, 1] on an edge of n texels: min(n - 1, floor(u n)); a NaN goes to 0
__device__ __forceinline__ int texel_of(double u, int n) {
  const double t = floor(u * (double)n);
  return !(t >= 0.0) ? 0 : (t > (double)(n - 1) ? n - 1 : (int)t);
}

// the index of the sky texel of d: cube_face_uv's face, swaps and signs (cube.h) in float64, the nearest texel
__device__ __forceinline__ size_t sky_texel(const double* d, int n) {
  double x = d[0], y = d[1];
  const double z = d[2], ax = fabs(x), ay = fabs(y), az = fabs(z);
  int idx;
  double c;
  if (az > fmax(ax, ay)) {
    idx = 4, c = z;
  } else if (ay > ax) {
    idx = 2, c = y, y = z;
  } else {
    idx = 0, c = x, x = z;
  }
  if (c < 0.0) idx += 1;
  const double m = 0.5 / fabs(c);
  const double m0 = (idx == 0 || idx == 5) ? -m : m, m1 = (idx != 2) ? -m : m;
  const double u = fmin(fmax(x * m0 + 0.5, 0.0), 1.0), w = fmin(fmax(y * m1 + 0.5, 0.0), 1.0);
  return ((size_t)idx * n + texel_of(w, n)) * n + texel_of(u, n);
}

// the arguments the hemisphere kernels share, checked on the host
inline bool hemisphere_args(int n_rays, int n_rotations, double max_distance, double bias) {
  return max_distance >= 0.0 && std::fabs(bias) <= DBL_MAX && n_rays >= 64 && n_rays <= 1024 && n_rays % 64 == 0 &&
         n_rotations >= 1 && n_rotations <= 64;
}

inline bool make_view(int n_vertices, int n_faces, const float* vertices, const int* faces, const float* lo, double cell,
                      const int* dims, const long long* cell_start, const long long* pair_keys, long long n_pairs, double scale,
                      MeshView* m) {
  if (!(scale >= 0.0 && scale <= DBL_MAX) || n_vertices < 0 || n_faces < 0 || n_pairs < 0 || !make_grid(lo, cell, dims, &m->g) || !cell_start ||
      (n_pairs > 0 && (!pair_keys || !faces || !vertices)))
    return false;
  m->V = n_vertices, m->F = n_faces, m->vertices = vertices, m->faces = faces;
  m->cell_start = cell_start, m->pairs = pair_keys, m->n_pairs = n_pairs;
  m->M = scale;
  return true;
}

}  // namespace mesh_raycast
}  // namespace gigs
