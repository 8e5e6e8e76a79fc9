// mesh_raycast.hip -- what a ray hits: the nearest usable face of a mesh along a ray, through the uniform grid of triangle
// lists of mesh.triangle_grid, and on top of it the ambient occlusion of every vertex (mesh.raycast / mesh.bake_occlusion).
// include/gigs_hip.h, "Baking occlusion", states every quantity and tests/mesh_raycast_ref.py restates them in numpy; the
// sorts before the kernels are the caller's.
//
//   arithmetic    float64 on the float32 inputs, + - * / only: no sqrt, no transcendental, and the library is built with
//                 -ffp-contract=off, so numpy reproduces every bit.
//   determinism   One independent thread per ray; no thread waits on another and there is no float atomic.  The answer is
//                 the minimum of (t, face index) over the ACCEPTED faces (ray_triangle), a property of the ray and the
//                 mesh alone; the traversal only has to visit every cell that can list an accepted face ("Baking
//                 occlusion", has the argument), so neither the grid nor the schedule shows in the result.  The counters
//                 are integer atomics.
//   addresses     Every index read from `faces`, from a sort order, from cell_start or out of a pair key is compared with
//                 its range before it is used; a violation sets *overflow and the thread stores nothing.
//   raycast       Thread per ray, one-wave blocks, the rays sorted by the cell they enter the grid in: closest_kernel's
//                 shape and for its reason (dependent loads along lists of differing length; a block retires with its
//                 slowest wave).
//   bake          One one-wave block per vertex, in cell order.  The wave loops over the vertex's R / 64 chunks of 64
//                 directions, one direction per lane, and OWNS the vertex: the 64 lanes share origin and first cells (their
//                 first loads hit the same lines), a chunk's hits are __popcll(__ballot(hit)), and lane 0 stores the count
//                 and the float32 value itself -- no per-vertex atomic, no second kernel, no LDS.
#include "mesh_ray.h"  // ray_triangle, traverse, the hemisphere of a vertex: shared with mesh_light.hip

namespace gigs {
namespace mesh_raycast {

// ---- raycast ---------------------------------------------------------------------------------------------------------------
struct RaycastArgs {
  MeshView m;
  int N;
  const float *origins, *directions;
  const long long* order;
  double tmax;
  float *t, *bary;
  int *face, *counts, *overflow;
};

__global__ __launch_bounds__(kWave) void raycast_kernel(RaycastArgs a) {
  const int i = item<kWave>(a.N);
  if (i < 0) return;
  const long long q = a.order ? a.order[i] : (long long)i;
  if (q < 0 || q >= a.N) {
    *a.overflow = 1;
    return;
  }
  double o[3], d[3];
  load3(a.origins, (int)q, o);
  load3(a.directions, (int)q, d);
  Hit best;
  best.t = INFINITY, best.w1 = best.w2 = 0.0, best.sum = 1.0, best.face = -1;
  if (!finite3(o) || !finite3(d) || (d[0] == 0.0 && d[1] == 0.0 && d[2] == 0.0)) {
    atomicAdd(a.counts + 1, 1);
  } else {
    if (!traverse(a.m, o, d, a.tmax, &best)) {
      *a.overflow = 1;
      return;
    }
    if (best.face >= 0) atomicAdd(a.counts, 1);
  }
  a.t[q] = (float)best.t;
  a.face[q] = best.face;
  a.bary[2 * (size_t)q] = (float)(best.w1 / best.sum);
  a.bary[2 * (size_t)q + 1] = (float)(best.w2 / best.sum);
}

// ---- bake ------------------------------------------------------------------------------------------------------------------
struct BakeArgs {
  MeshView m;
  const float* normals;
  const long long* order;
  const float* table;  // [K,R,3]
  int R, K;
  unsigned long long seed;
  double tmax, bias;
  float* occlusion;
  int* hits;
  unsigned long long* counts;  // hits_total, no_normal
  int* overflow;
};

__global__ __launch_bounds__(kWave) void bake_kernel(BakeArgs a) {
  const unsigned lane = threadIdx.x;
  const long long v = a.order ? a.order[blockIdx.x] : (long long)blockIdx.x;  // the whole wave takes one branch from here on
  if (v < 0 || v >= a.m.V) {
    *a.overflow = 1;
    return;
  }
  Hemisphere h;
  if (!hemisphere(a.m.vertices, a.normals, a.table, a.R, a.K, a.seed, a.bias, v, lane, &h)) {
    if (lane == 0) {
      a.occlusion[v] = 1.0f;
      a.hits[v] = 0;
      atomicAdd(a.counts + 1, 1ULL);
    }
    return;
  }
  const float* row = h.row;
  int hits = 0;
  bool ok = true;
  for (int j = 0; j < a.R; j += kWave, row += 3 * kWave) {
    double d[3];
    hemisphere_direction(h, row, d);
    Hit best;
    best.t = INFINITY, best.face = -1;
    ok = traverse(a.m, h.o, d, a.tmax, &best) && ok;
    hits += __popcll(__ballot(best.face >= 0));
  }
  if (__ballot(!ok) != 0ULL) {
    *a.overflow = 1;
    return;
  }
  if (lane == 0) {
    a.hits[v] = hits;
    a.occlusion[v] = (float)((double)(a.R - hits) / (double)a.R);
    atomicAdd(a.counts, (unsigned long long)hits);
  }
}

}  // namespace mesh_raycast
}  // namespace gigs

extern "C" {

int gigs_mesh_raycast(int n_vertices, int n_faces, const float* vertices, const int* faces, const float* lo, double cell,
                      const int* dims, const long long* cell_start, const long long* pair_keys, long long n_pairs, double scale,
                      int n_rays, const float* origins, const float* directions, const long long* order, double t_max, float* t,
                      int* face, float* bary, int* counts, int* overflow, void* stream) {
  using namespace gigs::mesh_raycast;
  RaycastArgs a;
  if (n_rays < 0 || !counts || !overflow || !(t_max >= 0.0) ||
      !make_view(n_vertices, n_faces, vertices, faces, lo, cell, dims, cell_start, pair_keys, n_pairs, scale, &a.m))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_raycast: bad argument");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, 2 * sizeof(int), s) != hipSuccess)
    return gigs_internal_fail(GIGS_ERR_HIP, "mesh_raycast: clear failed");
  if (n_rays == 0) return 0;
  if (!origins || !directions || !t || !face || !bary) return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_raycast: NULL array");
  a.N = n_rays, a.origins = origins, a.directions = directions, a.order = order, a.tmax = t_max;
  a.t = t, a.face = face, a.bary = bary, a.counts = counts, a.overflow = overflow;
  hipLaunchKernelGGL(raycast_kernel, dim3(blocks_for(n_rays, kWave)), dim3(kWave), 0, s, a);
  return gigs_internal_check_launch("mesh_raycast");
}

int gigs_mesh_bake_occlusion(int n_vertices, int n_faces, const float* vertices, const float* normals, const int* faces,
                             const float* lo, double cell, const int* dims, const long long* cell_start,
                             const long long* pair_keys, long long n_pairs, double scale, const long long* order,
                             const float* directions, int n_rays, int n_rotations, unsigned long long seed, double max_distance, double bias,
                             float* occlusion, int* hits, unsigned long long* counts, int* overflow, void* stream) {
  using namespace gigs::mesh_raycast;
  BakeArgs a;
  if (!counts || !overflow || !hemisphere_args(n_rays, n_rotations, max_distance, bias) ||
      !make_view(n_vertices, n_faces, vertices, faces, lo, cell, dims, cell_start, pair_keys, n_pairs, scale, &a.m))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_bake_occlusion: bad argument");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), s) != hipSuccess)
    return gigs_internal_fail(GIGS_ERR_HIP, "mesh_bake_occlusion: clear failed");
  if (n_vertices == 0) return 0;
  if (!vertices || !normals || !directions || !occlusion || !hits)
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_bake_occlusion: NULL array");
  a.normals = normals, a.order = order, a.table = directions, a.R = n_rays, a.K = n_rotations, a.seed = seed;
  a.tmax = max_distance, a.bias = bias, a.occlusion = occlusion, a.hits = hits, a.counts = counts, a.overflow = overflow;
  hipLaunchKernelGGL(bake_kernel, dim3((unsigned)n_vertices), dim3(kWave), 0, s, a);
  return gigs_internal_check_launch("mesh_bake_occlusion");
}
}  // extern "C"
