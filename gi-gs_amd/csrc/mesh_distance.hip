// mesh_distance.hip -- comparing two meshes: face areas, stratified surface samples, a uniform grid of triangle lists and the
// exact closest triangle of a point by an expanding-shell search.  include/gigs_hip.h, "Comparing meshes", states every
// quantity and tests/mesh_distance_ref.py restates them in numpy.  The sorts and scans between the kernels are the caller's
// (mesh.sample_surface / mesh.closest_point).
//
//   determinism   One independent thread per face, sample or query; no thread waits on another and there is no float
//                 atomic.  The closest face is the minimum of (d^2, face index) over the faces a query visits, so neither
//                 the order of the cells nor the schedule shows in the result.  The counters are integer atomics.  The
//                 library is built with -ffp-contract=off (build.py): no product below is fused into a sum, in any run.
//   addresses     Every index read from `faces`, from a sort order, from cell_start or out of a pair key is compared with
//                 its range before it is used.  A violation cannot come from mesh.py; it sets *overflow and the thread
//                 stores nothing (gigs_mesh_compact's convention).
//   closest       Thread per query.  The work of a query is a walk over cell headers and short face lists in which every
//                 load depends on the one before it, and its length differs from query to query; the caller sorts the
//                 queries by cell, so the lanes of a wave walk the same lists and the loads of a step hit the same lines.
//                 A lane group per query would share one query's faces among its lanes, but the lists hold a dozen faces
//                 where a group wants 16 or 64, and the (d^2, index) minimum would need a cross-lane reduction per shell.
//                 One-wave blocks: a block retires with its slowest wave, and an outlier query keeps only its own wave.
#include "mesh_triangle.h"  // triangle_closest, shared with mesh_atlas.hip; through it mesh_grid.h: the per-thread and vector
                            // helpers, the hash, and the grid arithmetic shared with mesh_raycast.hip

namespace gigs {
namespace mesh_distance {

constexpr double kShrink = 1.0 - 0x1p-40;  // the relative part of the slack on L(r)

// ---- areas -----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void areas_kernel(int V, int F, const float* __restrict__ vertices,
                                                    const int* __restrict__ faces, double* __restrict__ areas, int* skipped) {
  const int f = item<256>(F);
  if (f < 0) return;
  const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
  double area = 0.0;
  if (in_range(ia, ib, ic, V)) {  // else never dereferenced
    double p0[3], p1[3], p2[3], e1[3], e2[3], n[3];
    load3(vertices, ia, p0);
    load3(vertices, ib, p1);
    load3(vertices, ic, p2);
    if (finite3(p0) && finite3(p1) && finite3(p2)) {
#pragma unroll
      for (int c = 0; c < 3; c++) e1[c] = p1[c] - p0[c], e2[c] = p2[c] - p0[c];
      cross3(e1, e2, n);
      const double len = sqrt(dot3(n, n));
      if (len > 0.0) area = len * 0.5;
    }
  }
  areas[f] = area;
  if (!(area > 0.0)) atomicAdd(skipped, 1);
}

// ---- samples ---------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double uniform(unsigned long long seed, unsigned i, unsigned k) {
  return (double)(mix64(((seed << 32) + i) * 4ULL + k) >> 11) * 0x1p-53;
}

__global__ __launch_bounds__(256) void sample_kernel(int V, int F, const float* __restrict__ vertices,
                                                     const int* __restrict__ faces, const double* __restrict__ cum, int n,
                                                     unsigned long long seed, float* __restrict__ points,
                                                     int* __restrict__ face, float* __restrict__ bary, int* overflow) {
  const int i = item<256>(n);
  if (i < 0) return;
  const double A = cum[F - 1];
  if (!(A > 0.0 && A <= DBL_MAX)) {
    *overflow = 1;
    return;
  }
  const double t = ((double)i + uniform(seed, (unsigned)i, 0)) / (double)n * A;
  int lo = 0, hi = F;  // the first f with cum[f] > t
  while (lo < hi) {
    const int mid = lo + ((hi - lo) >> 1);
    if (cum[mid] > t) hi = mid; else lo = mid + 1;
  }
  if (lo == F) {  // t reached A: the face that brings cum to A
    lo = 0, hi = F - 1;
    while (lo < hi) {
      const int mid = lo + ((hi - lo) >> 1);
      if (cum[mid] >= A) hi = mid; else lo = mid + 1;
    }
  }
  const int f = lo;
  const int ia = faces[3 * (size_t)f], ib = faces[3 * (size_t)f + 1], ic = faces[3 * (size_t)f + 2];
  if (!in_range(ia, ib, ic, V)) {
    *overflow = 1;
    return;
  }
  double a = uniform(seed, (unsigned)i, 1), b = uniform(seed, (unsigned)i, 2);
  if (a + b > 1.0) a = 1.0 - a, b = 1.0 - b;
  double p0[3], p1[3], p2[3];
  load3(vertices, ia, p0);
  load3(vertices, ib, p1);
  load3(vertices, ic, p2);
#pragma unroll
  for (int c = 0; c < 3; c++) points[3 * (size_t)i + c] = (float)((p0[c] + a * (p1[c] - p0[c])) + b * (p2[c] - p0[c]));
  face[i] = f;
  bary[2 * (size_t)i] = (float)a;
  bary[2 * (size_t)i + 1] = (float)b;
}

// ---- the grid --------------------------------------------------------------------------------------------------------------
// the cell range of a usable face, or false
__device__ __forceinline__ bool face_cells(const Grid& g, int V, const float* vertices, const int* faces, const double* areas,
                                           int f, int* c0, int* c1) {
  if (!(areas[f] > 0.0)) return false;
  const int idx[3] = {faces[3 * (size_t)f], faces[3 * (size_t)f + 1], faces[3 * (size_t)f + 2]};
  if (!in_range(idx[0], idx[1], idx[2], V)) return false;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const double x0 = (double)vertices[3 * (size_t)idx[0] + a], x1 = (double)vertices[3 * (size_t)idx[1] + a],
                 x2 = (double)vertices[3 * (size_t)idx[2] + a];
    c0[a] = cell_of(g, a, fmin(x0, fmin(x1, x2)));
    c1[a] = cell_of(g, a, fmax(x0, fmax(x1, x2)));
    if (c1[a] < c0[a]) c1[a] = c0[a];  // only with a NaN, which the areas exclude
  }
  return true;
}

__global__ __launch_bounds__(256) void grid_count_kernel(Grid g, int V, int F, const float* __restrict__ vertices,
                                                         const int* __restrict__ faces, const double* __restrict__ areas,
                                                         int* __restrict__ counts) {
  const int f = item<256>(F);
  if (f < 0) return;
  int c0[3], c1[3], n = 0;
  if (face_cells(g, V, vertices, faces, areas, f, c0, c1)) n = (c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1);
  counts[f] = n;  // at most 256^3
}

__global__ __launch_bounds__(256) void grid_pairs_kernel(Grid g, int V, int F, const float* __restrict__ vertices,
                                                         const int* __restrict__ faces, const double* __restrict__ areas,
                                                         const long long* __restrict__ offsets, long long n_pairs,
                                                         long long* __restrict__ pairs, int* overflow) {
  const int f = item<256>(F);
  if (f < 0) return;
  int c0[3], c1[3];
  if (!face_cells(g, V, vertices, faces, areas, f, c0, c1)) return;
  const long long n = (long long)(c1[0] - c0[0] + 1) * (c1[1] - c0[1] + 1) * (c1[2] - c0[2] + 1);
  long long at = offsets[f];
  if (at < 0 || at > n_pairs || n > n_pairs - at) {
    *overflow = 1;
    return;
  }
  for (int z = c0[2]; z <= c1[2]; z++)
    for (int y = c0[1]; y <= c1[1]; y++)
      for (int x = c0[0]; x <= c1[0]; x++) {
        const long long cell = ((long long)z * g.G[1] + y) * g.G[0] + x;
        pairs[at++] = (cell << 32) | (long long)(unsigned)f;
      }
}

// ---- closest ---------------------------------------------------------------------------------------------------------------
struct ClosestArgs {
  Grid g;
  int V, F, N;
  const float* vertices;
  const int* faces;
  const long long *cell_start, *pairs;
  long long n_pairs;
  const float* points;
  const long long* order;
  double max_distance, max_d2, slack;
  float* distance;
  int *face, *counts, *overflow;
};

constexpr unsigned kClosestBlock = 64;

__global__ __launch_bounds__(kClosestBlock) void closest_kernel(ClosestArgs a) {
  const int i = item<kClosestBlock>(a.N);
  if (i < 0) return;
  const long long q = a.order ? a.order[i] : (long long)i;
  if (q < 0 || q >= a.N) {
    *a.overflow = 1;
    return;
  }
  double p[3];
  load3(a.points, (int)q, p);
  if (!finite3(p)) {
    a.distance[q] = INFINITY;
    a.face[q] = -1;
    atomicAdd(a.counts + 1, 1);
    return;
  }
  const Grid& g = a.g;
  const int c0[3] = {cell_of(g, 0, p[0]), cell_of(g, 1, p[1]), cell_of(g, 2, p[2])};
  const int rounds = max(g.G[0], max(g.G[1], g.G[2]));
  double best2 = INFINITY;
  int bestf = -1;
  bool bad = false;

  auto visit = [&](int x, int y, int z) {
    const long long cell = ((long long)z * g.G[1] + y) * g.G[0] + x;
    const long long s = a.cell_start[cell], e = a.cell_start[cell + 1];
    if (s < 0 || e < s || e > a.n_pairs) {
      bad = true;
      return;
    }
    for (long long k = s; k < e; k++) {
      const long long key = a.pairs[k];
      const long long f = key & 0xffffffffLL;
      if ((key >> 32) != cell || f >= a.F) {
        bad = true;
        continue;
      }
      const int idx[3] = {a.faces[3 * (size_t)f], a.faces[3 * (size_t)f + 1], a.faces[3 * (size_t)f + 2]};
      if (!in_range(idx[0], idx[1], idx[2], a.V)) {
        bad = true;
        continue;
      }
      double p0[3], p1[3], p2[3];
      load3(a.vertices, idx[0], p0);
      load3(a.vertices, idx[1], p1);
      load3(a.vertices, idx[2], p2);
      const double d2 = triangle_closest<false>(p, idx[0], idx[1], idx[2], p0, p1, p2);
      if (d2 < best2 || (d2 == best2 && (int)f < bestf)) best2 = d2, bestf = (int)f;
    }
  };

  for (int r = 0; r < rounds; r++) {
    // shell r: the cells of the grid at Chebyshev distance r from c0
    const int z0 = max(c0[2] - r, 0), z1 = min(c0[2] + r, g.G[2] - 1);
    const int y0 = max(c0[1] - r, 0), y1 = min(c0[1] + r, g.G[1] - 1);
    const int x0 = max(c0[0] - r, 0), x1 = min(c0[0] + r, g.G[0] - 1);
    for (int z = z0; z <= z1; z++)
      for (int y = y0; y <= y1; y++) {
        if (abs(z - c0[2]) == r || abs(y - c0[1]) == r) {
          for (int x = x0; x <= x1; x++) visit(x, y, z);
        } else {  // r > 0 here: the two ends of the row
          if (c0[0] - r >= 0) visit(c0[0] - r, y, z);
          if (c0[0] + r < g.G[0]) visit(c0[0] + r, y, z);
        }
      }
    // L(r): every face the block [c0 - r, c0 + r] has not seen lies behind a side of it that has cells behind it
    double L = INFINITY;
#pragma unroll
    for (int ax = 0; ax < 3; ax++) {
      if (c0[ax] - r > 0) L = fmin(L, fmax(p[ax] - plane_of(g, ax, c0[ax] - r), 0.0));
      if (c0[ax] + r < g.G[ax] - 1) L = fmin(L, fmax(plane_of(g, ax, c0[ax] + r + 1) - p[ax], 0.0));
    }
    if (!(L <= DBL_MAX)) break;  // the block covers the grid
    const double Ls = (L - a.slack) * kShrink;
    if (Ls > 0.0 && best2 <= Ls * Ls) break;
    if (Ls > a.max_distance) break;
  }
  if (bad) {
    *a.overflow = 1;
    return;
  }
  if (bestf < 0 || best2 > a.max_d2) {
    a.distance[q] = (float)a.max_distance;
    a.face[q] = -1;
    atomicAdd(a.counts, 1);
    return;
  }
  a.distance[q] = (float)sqrt(best2);
  a.face[q] = bestf;
}

}  // namespace mesh_distance
}  // namespace gigs

extern "C" {

int gigs_mesh_face_areas(int n_vertices, int n_faces, const float* vertices, const int* faces, double* areas, int* skipped,
                         void* stream) {
  using namespace gigs::mesh_distance;
  if (n_vertices < 0 || n_faces < 0 || !skipped || (n_faces > 0 && (!faces || !areas)) || (n_vertices > 0 && !vertices))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_face_areas: bad argument");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(skipped, 0, sizeof(int), s) != hipSuccess)
    return gigs_internal_fail(GIGS_ERR_HIP, "mesh_face_areas: clear failed");
  if (n_faces == 0) return 0;
  hipLaunchKernelGGL(areas_kernel, dim3(blocks_for(n_faces)), dim3(256), 0, s, n_vertices, n_faces, vertices, faces, areas,
                     skipped);
  return gigs_internal_check_launch("mesh_face_areas");
}

int gigs_mesh_sample_surface(int n_vertices, int n_faces, const float* vertices, const int* faces, const double* cum_areas,
                             int n_samples, unsigned long long seed, float* points, int* face, float* bary, int* overflow,
                             void* stream) {
  using namespace gigs::mesh_distance;
  if (n_vertices < 0 || n_faces < 0 || n_samples < 0 || !overflow)
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_sample_surface: bad argument");
  if (n_samples == 0) return 0;
  if (n_faces == 0 || n_vertices == 0 || !vertices || !faces || !cum_areas || !points || !face || !bary)
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_sample_surface: samples of nothing, or a NULL array");
  hipLaunchKernelGGL(sample_kernel, dim3(blocks_for(n_samples)), dim3(256), 0, (hipStream_t)stream, n_vertices, n_faces,
                     vertices, faces, cum_areas, n_samples, seed, points, face, bary, overflow);
  return gigs_internal_check_launch("mesh_sample_surface");
}

int gigs_mesh_grid_count(int n_vertices, int n_faces, const float* vertices, const int* faces, const double* areas,
                         const float* lo, double cell, const int* dims, int* counts, void* stream) {
  using namespace gigs::mesh_distance;
  Grid g;
  if (n_vertices < 0 || n_faces < 0 || !make_grid(lo, cell, dims, &g) ||
      (n_faces > 0 && (!faces || !areas || !counts)) || (n_vertices > 0 && !vertices))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_grid_count: bad argument");
  if (n_faces == 0) return 0;
  hipLaunchKernelGGL(grid_count_kernel, dim3(blocks_for(n_faces)), dim3(256), 0, (hipStream_t)stream, g, n_vertices, n_faces,
                     vertices, faces, areas, counts);
  return gigs_internal_check_launch("mesh_grid_count");
}

int gigs_mesh_grid_pairs(int n_vertices, int n_faces, const float* vertices, const int* faces, const double* areas,
                         const float* lo, double cell, const int* dims, const long long* offsets, long long n_pairs,
                         long long* pair_keys, int* overflow, void* stream) {
  using namespace gigs::mesh_distance;
  Grid g;
  if (n_vertices < 0 || n_faces < 0 || n_pairs < 0 || !overflow || !make_grid(lo, cell, dims, &g) ||
      (n_faces > 0 && (!faces || !areas || !offsets)) || (n_vertices > 0 && !vertices) || (n_pairs > 0 && !pair_keys))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_grid_pairs: bad argument");
  if (n_faces == 0) return 0;
  hipLaunchKernelGGL(grid_pairs_kernel, dim3(blocks_for(n_faces)), dim3(256), 0, (hipStream_t)stream, g, n_vertices, n_faces,
                     vertices, faces, areas, offsets, n_pairs, pair_keys, overflow);
  return gigs_internal_check_launch("mesh_grid_pairs");
}

int gigs_mesh_closest(int n_vertices, int n_faces, const float* vertices, const int* faces, const float* lo, double cell,
                      const int* dims, const long long* cell_start, const long long* pair_keys, long long n_pairs,
                      int n_points, const float* points, const long long* order, double max_distance, float* distance,
                      int* face, int* counts, int* overflow, void* stream) {
  using namespace gigs::mesh_distance;
  ClosestArgs a;
  if (n_vertices < 0 || n_faces < 0 || n_points < 0 || n_pairs < 0 || !counts || !overflow || !make_grid(lo, cell, dims, &a.g) ||
      !(max_distance >= 0.0) || !cell_start || (n_pairs > 0 && (!pair_keys || !faces || !vertices)))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_closest: bad argument");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, 2 * sizeof(int), s) != hipSuccess)
    return gigs_internal_fail(GIGS_ERR_HIP, "mesh_closest: clear failed");
  if (n_points == 0) return 0;
  if (!points || !distance || !face) return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_closest: NULL array");
  a.V = n_vertices, a.F = n_faces, a.N = n_points;
  a.vertices = vertices, a.faces = faces, a.cell_start = cell_start, a.pairs = pair_keys, a.n_pairs = n_pairs;
  a.points = points, a.order = order;
  a.max_distance = max_distance, a.max_d2 = max_distance * max_distance;
  double m = 0.0;
  for (int k = 0; k < 3; k++) m = std::fmax(m, std::fmax(std::fabs(a.g.lo[k]), std::fabs(a.g.lo[k] + a.g.G[k] * a.g.cell)));
  a.slack = 0x1p-45 * m;
  a.distance = distance, a.face = face, a.counts = counts, a.overflow = overflow;
  hipLaunchKernelGGL(closest_kernel, dim3(blocks_for(n_points, kClosestBlock)), dim3(kClosestBlock), 0, s, a);
  return gigs_internal_check_launch("mesh_closest");
}
}  // extern "C"
