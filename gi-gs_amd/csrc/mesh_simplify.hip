// mesh_simplify.hip -- simplifying a mesh by vertex clustering with quadric placement (Rossignac-Borrel cells, Lindstrom's
// representative vertex).  include/gigs_hip.h, "Simplifying meshes", states every quantity and tests/mesh_simplify_ref.py
// restates them in numpy.  The sorts and scans between the kernels are the caller's (mesh.simplify).
//
//   determinism   No kernel waits on another thread and there is no float atomic: a cluster is one thread that walks its
//                 members (ascending vertex index) and its faces (ascending face index) in the order the caller's stable
//                 sorts fixed, so every float64 sum has one order and the output bits do not depend on the schedule.  The
//                 two counters of cluster_faces_kernel and the one of dedupe_kernel are integer atomics.  The library is
//                 built with -ffp-contract=off (build.py): no product below is fused into a sum, in any run.
//   addresses     Every index read from `faces`, from a sort order, from an offset table or out of a pair key is compared
//                 with its range before it is used.  A violation cannot come from mesh.simplify; it sets *overflow and the
//                 thread stores nothing (gigs_mesh_compact's convention).
#include "mesh_grid.h"  // item, in_range, blocks_for

namespace gigs {
namespace mesh_simplify {

constexpr int kCellBits = 21;
constexpr float kCellLimit = 2097152.0f;  // 2^21: cell coordinates lie in [0, 2^21)
constexpr long long kCellMask = (1LL << kCellBits) - 1;
constexpr long long kNoPair = 0x7fffffffffffffffLL;  // sorts behind every (cluster, face) pair

using namespace gigs::mesh_common;

__global__ __launch_bounds__(256) void keys_kernel(int V, const float* __restrict__ vertices, float ox, float oy, float oz,
                                                   float inv, long long* __restrict__ keys) {
  const int v = item<256>(V);
  if (v < 0) return;
  const float o[3] = {ox, oy, oz};
  long long key = 0;
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float x = vertices[3 * (size_t)v + c];
    const float t = floorf(__fmul_rn(__fsub_rn(x, o[c]), inv));
    // a NaN fails every comparison; an infinite x, or a difference that overflowed, fails t < 2^21
    const bool in = fabsf(x) <= FLT_MAX && t >= 0.0f && t < kCellLimit;
    ok = ok && in;
    key |= (long long)(in ? (int)t : 0) << (kCellBits * c);
  }
  keys[v] = ok ? key : -1;
}

__device__ __forceinline__ long long pair_key(int cluster, int face) {
  return ((long long)cluster << 32) | (long long)(unsigned)face;
}

// counts[0]: invalid faces, counts[1]: valid faces with a repeated cluster
__global__ __launch_bounds__(256) void cluster_faces_kernel(int V, int F, int C, const int* __restrict__ faces,
                                                            const int* __restrict__ cluster_of, int* __restrict__ triples,
                                                            long long* __restrict__ pairs, int* counts) {
  const int f = item<256>(F);
  if (f < 0) return;
  const int a = faces[3 * (size_t)f], b = faces[3 * (size_t)f + 1], c = faces[3 * (size_t)f + 2];
  int ca = -1, cb = -1, cc = -1;
  if (in_range(a, b, c, V)) {  // else never dereferenced
    ca = cluster_of[a];
    cb = cluster_of[b];
    cc = cluster_of[c];
  }
  int t0 = -1, t1 = -1, t2 = -1;
  long long p0 = kNoPair, p1 = kNoPair, p2 = kNoPair;
  if (in_range(ca, cb, cc, C)) {
    p0 = pair_key(ca, f);
    if (cb != ca) p1 = pair_key(cb, f);
    if (cc != ca && cc != cb) p2 = pair_key(cc, f);
    if (ca != cb && cb != cc && ca != cc) {  // survives: rotated so that the smallest cluster leads, winding unchanged
      if (ca < cb && ca < cc) {
        t0 = ca, t1 = cb, t2 = cc;
      } else if (cb < cc) {
        t0 = cb, t1 = cc, t2 = ca;
      } else {
        t0 = cc, t1 = ca, t2 = cb;
      }
    } else {
      atomicAdd(counts + 1, 1);
    }
  } else {
    atomicAdd(counts, 1);
  }
  triples[3 * (size_t)f] = t0;
  triples[3 * (size_t)f + 1] = t1;
  triples[3 * (size_t)f + 2] = t2;
  pairs[3 * (size_t)f] = p0;
  pairs[3 * (size_t)f + 1] = p1;
  pairs[3 * (size_t)f + 2] = p2;
}

// row i of the faces sorted by triple (ties in ascending face index): the face keeps its triple unless it equals its
// predecessor's.  out_faces was set to -1 throughout; `triples` is read-only here, so no thread reads what another writes.
__global__ __launch_bounds__(256) void dedupe_kernel(int F, const int* __restrict__ triples, const long long* __restrict__ order,
                                                     int* __restrict__ out_faces, int* duplicates, int* overflow) {
  const int i = item<256>(F);
  if (i < 0) return;
  const long long f = order[i];
  const long long g = i > 0 ? order[i - 1] : 0;
  if (f < 0 || f >= F || g < 0 || g >= F) {
    *overflow = 1;
    return;
  }
  const int t0 = triples[3 * (size_t)f], t1 = triples[3 * (size_t)f + 1], t2 = triples[3 * (size_t)f + 2];
  if (t0 < 0) return;
  if (i > 0 && triples[3 * (size_t)g] == t0 && triples[3 * (size_t)g + 1] == t1 && triples[3 * (size_t)g + 2] == t2) {
    atomicAdd(duplicates, 1);
    return;
  }
  out_faces[3 * (size_t)f] = t0;
  out_faces[3 * (size_t)f + 1] = t1;
  out_faces[3 * (size_t)f + 2] = t2;
}

struct SolveArgs {
  int V, F, C;
  const float *vertices, *normals, *albedo, *roughness, *metallic;
  const int* faces;
  const long long *member_order, *member_start, *pairs, *pair_start, *cluster_keys;
  float ox, oy, oz, cell;
  double reg;
  float *out_vertices, *out_normals, *out_albedo, *out_roughness, *out_metallic;
  int* overflow;
};

constexpr unsigned kSolveBlock = 64;  // one wave: clusters are few and their segments differ in length

// One thread per cluster.  Segment lengths diverge within a wave (a handful of members and a dozen faces on an extracted
// mesh, hundreds in a crowded cell) and every load depends on an index loaded just before it, so the kernel lives on waves
// in flight, not on lanes in step: 64-thread blocks spread the clusters over the CUs.
__global__ __launch_bounds__(kSolveBlock) void solve_kernel(SolveArgs p) {
  const int k = item<kSolveBlock>(p.C);
  if (k < 0) return;
  const long long m0 = p.member_start[k], m1 = p.member_start[k + 1];
  const long long f0 = p.pair_start[k], f1 = p.pair_start[k + 1];
  const long long key = p.cluster_keys[k];
  if (m0 < 0 || m1 <= m0 || m1 > p.V || f0 < 0 || f1 < f0 || f1 > 3LL * p.F || key < 0) {
    *p.overflow = 1;
    return;
  }
  const double cell = (double)p.cell;
  const double g[3] = {(double)p.ox + ((double)(key & kCellMask) + 0.5) * cell,
                       (double)p.oy + ((double)((key >> kCellBits) & kCellMask) + 0.5) * cell,
                       (double)p.oz + ((double)((key >> (2 * kCellBits)) & kCellMask) + 0.5) * cell};
  bool bad = false;

  // members, ascending vertex index
  double sp[3] = {0.0, 0.0, 0.0}, sn[3] = {0.0, 0.0, 0.0}, sa[3] = {0.0, 0.0, 0.0}, sr = 0.0, st = 0.0;
  for (long long i = m0; i < m1; i++) {
    const long long v = p.member_order[i];
    if (v < 0 || v >= p.V) {
      bad = true;
      continue;
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
      sp[c] += (double)p.vertices[3 * (size_t)v + c] - g[c];
      sn[c] += (double)p.normals[3 * (size_t)v + c];
      sa[c] += (double)p.albedo[3 * (size_t)v + c];
    }
    sr += (double)p.roughness[v];
    st += (double)p.metallic[v];
  }

  // the area-weighted plane quadrics of the cluster's valid faces, ascending face index: A (symmetric) and b
  double a00 = 0.0, a01 = 0.0, a02 = 0.0, a11 = 0.0, a12 = 0.0, a22 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0;
  for (long long i = f0; i < f1; i++) {
    const long long pk = p.pairs[i];
    const long long f = pk & 0xffffffffLL;
    if ((pk >> 32) != k || f >= p.F) {
      bad = true;
      continue;
    }
    const int ia = p.faces[3 * (size_t)f], ib = p.faces[3 * (size_t)f + 1], ic = p.faces[3 * (size_t)f + 2];
    if (!in_range(ia, ib, ic, p.V)) {
      bad = true;
      continue;
    }
    double q0[3], e1[3], e2[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      q0[c] = (double)p.vertices[3 * (size_t)ia + c] - g[c];
      e1[c] = ((double)p.vertices[3 * (size_t)ib + c] - g[c]) - q0[c];
      e2[c] = ((double)p.vertices[3 * (size_t)ic + c] - g[c]) - q0[c];
    }
    const double nx = e1[1] * e2[2] - e1[2] * e2[1];
    const double ny = e1[2] * e2[0] - e1[0] * e2[2];
    const double nz = e1[0] * e2[1] - e1[1] * e2[0];
    const double len = sqrt(nx * nx + ny * ny + nz * nz);
    if (!(len > 0.0)) continue;
    const double ux = nx / len, uy = ny / len, uz = nz / len;
    const double w = len * 0.5;
    const double d = -(ux * q0[0] + uy * q0[1] + uz * q0[2]);
    const double wx = w * ux, wy = w * uy, wz = w * uz;
    a00 += wx * ux;
    a01 += wx * uy;
    a02 += wx * uz;
    a11 += wy * uy;
    a12 += wy * uz;
    a22 += wz * uz;
    b0 += wx * d;
    b1 += wy * d;
    b2 += wz * d;
  }
  if (bad) {
    *p.overflow = 1;
    return;
  }

  const double n = (double)(m1 - m0);
  double x[3] = {sp[0] / n, sp[1] / n, sp[2] / n};  // the member mean
  const double lam = p.reg * ((a00 + a11) + a22) / 3.0;
  if (lam > 0.0) {  // (A + lam I) x = lam m - b by cofactors: symmetric positive definite, condition <= 3 / reg + 1
    const double m00 = a00 + lam, m11 = a11 + lam, m22 = a22 + lam;
    const double r0 = lam * x[0] - b0, r1 = lam * x[1] - b1, r2 = lam * x[2] - b2;
    const double c00 = m11 * m22 - a12 * a12, c01 = a02 * a12 - a01 * m22, c02 = a01 * a12 - a02 * m11;
    const double c11 = m00 * m22 - a02 * a02, c12 = a01 * a02 - m00 * a12, c22 = m00 * m11 - a01 * a01;
    const double det = m00 * c00 + a01 * c01 + a02 * c02;
    x[0] = (c00 * r0 + c01 * r1 + c02 * r2) / det;
    x[1] = (c01 * r0 + c11 * r1 + c12 * r2) / det;
    x[2] = (c02 * r0 + c12 * r1 + c22 * r2) / det;
  }
  const double half = 0.5 * cell;
  const double nl = sqrt(sn[0] * sn[0] + sn[1] * sn[1] + sn[2] * sn[2]);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const double xc = x[c] < -half ? -half : (x[c] > half ? half : x[c]);
    p.out_vertices[3 * (size_t)k + c] = (float)(g[c] + xc);
    p.out_normals[3 * (size_t)k + c] = nl > 0.0 ? (float)(sn[c] / nl) : 0.0f;
    p.out_albedo[3 * (size_t)k + c] = (float)(sa[c] / n);
  }
  p.out_roughness[k] = (float)(sr / n);
  p.out_metallic[k] = (float)(st / n);
}

}  // namespace mesh_simplify
}  // namespace gigs

extern "C" {

int gigs_mesh_cluster_keys(int n_vertices, const float* vertices, const float* origin, float inv_cell, long long* keys,
                           void* stream) {
  using namespace gigs::mesh_simplify;
  if (n_vertices < 0 || !origin || !(inv_cell > 0.0f && inv_cell <= FLT_MAX) || (n_vertices > 0 && (!vertices || !keys)))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_cluster_keys: bad argument");
  if (n_vertices == 0) return 0;
  hipLaunchKernelGGL(keys_kernel, dim3(blocks_for(n_vertices)), dim3(256), 0, (hipStream_t)stream, n_vertices, vertices,
                     origin[0], origin[1], origin[2], inv_cell, keys);
  return gigs_internal_check_launch("mesh_cluster_keys");
}

int gigs_mesh_cluster_faces(int n_vertices, int n_faces, int n_clusters, const int* faces, const int* cluster_of, int* triples,
                            long long* pair_keys, int* counts, void* stream) {
  using namespace gigs::mesh_simplify;
  if (n_vertices < 0 || n_faces < 0 || n_clusters < 0 || !counts || (n_faces > 0 && (!faces || !triples || !pair_keys)) ||
      (n_vertices > 0 && !cluster_of))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_cluster_faces: bad argument");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, 2 * sizeof(int), s) != hipSuccess)
    return gigs_internal_fail(GIGS_ERR_HIP, "mesh_cluster_faces: clear failed");
  if (n_faces == 0) return 0;
  hipLaunchKernelGGL(cluster_faces_kernel, dim3(blocks_for(n_faces)), dim3(256), 0, s, n_vertices, n_faces, n_clusters, faces,
                     cluster_of, triples, pair_keys, counts);
  return gigs_internal_check_launch("mesh_cluster_faces");
}

int gigs_mesh_face_dedupe(int n_faces, const int* triples, const long long* order, int* out_faces, int* duplicates,
                          int* overflow, void* stream) {
  using namespace gigs::mesh_simplify;
  if (n_faces < 0 || !duplicates || !overflow || (n_faces > 0 && (!triples || !order || !out_faces)))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_face_dedupe: bad argument");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(duplicates, 0, sizeof(int), s) != hipSuccess ||
      (n_faces > 0 && hipMemsetAsync(out_faces, 0xff, 3 * sizeof(int) * (size_t)n_faces, s) != hipSuccess))
    return gigs_internal_fail(GIGS_ERR_HIP, "mesh_face_dedupe: clear failed");
  if (n_faces == 0) return 0;
  hipLaunchKernelGGL(dedupe_kernel, dim3(blocks_for(n_faces)), dim3(256), 0, s, n_faces, triples, order, out_faces, duplicates,
                     overflow);
  return gigs_internal_check_launch("mesh_face_dedupe");
}

int gigs_mesh_cluster_solve(int n_vertices, int n_faces, int n_clusters, const float* vertices, const float* normals,
                            const float* albedo, const float* roughness, const float* metallic, const int* faces,
                            const long long* member_order, const long long* member_start, const long long* pair_keys,
                            const long long* pair_start, const long long* cluster_keys, const float* origin, float cell,
                            double reg, float* out_vertices, float* out_normals, float* out_albedo, float* out_roughness,
                            float* out_metallic, int* overflow, void* stream) {
  using namespace gigs::mesh_simplify;
  if (n_vertices < 0 || n_faces < 0 || n_clusters < 0 || n_clusters > n_vertices || !origin || !overflow ||
      !(cell > 0.0f && cell <= FLT_MAX) || !(reg > 0.0 && reg <= 1.0))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_cluster_solve: bad argument");
  if (n_clusters == 0) return 0;
  if (!vertices || !normals || !albedo || !roughness || !metallic || !member_order || !member_start || !pair_start ||
      !cluster_keys || (n_faces > 0 && (!faces || !pair_keys)))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_cluster_solve: NULL input");
  if (!out_vertices || !out_normals || !out_albedo || !out_roughness || !out_metallic)
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_cluster_solve: NULL output");
  SolveArgs p;
  p.V = n_vertices, p.F = n_faces, p.C = n_clusters;
  p.vertices = vertices, p.normals = normals, p.albedo = albedo, p.roughness = roughness, p.metallic = metallic;
  p.faces = faces;
  p.member_order = member_order, p.member_start = member_start, p.pairs = pair_keys, p.pair_start = pair_start;
  p.cluster_keys = cluster_keys;
  p.ox = origin[0], p.oy = origin[1], p.oz = origin[2], p.cell = cell, p.reg = reg;
  p.out_vertices = out_vertices, p.out_normals = out_normals, p.out_albedo = out_albedo, p.out_roughness = out_roughness;
  p.out_metallic = out_metallic, p.overflow = overflow;
  hipLaunchKernelGGL(solve_kernel, dim3(blocks_for(n_clusters, kSolveBlock)), dim3(kSolveBlock), 0, (hipStream_t)stream, p);
  return gigs_internal_check_launch("mesh_cluster_solve");
}
}  // extern "C"
