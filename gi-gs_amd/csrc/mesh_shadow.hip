// mesh_shadow.hip -- shadows of analytic lights per POINT: for any set of surface points with normals (the covered pixels of a
// G-buffer) and L point or directional lights, the share of each light's S samples that reach the point past the mesh
// (mesh.shadow_points).  include/gigs_hip.h, "Shadows of analytic lights", states every quantity and tests/mesh_shadow_ref.py
// restates them in numpy.
//
//   arithmetic    mesh_ray.h's: float64 on the float32 inputs, + - * / only, no root, no transcendental, built with
//                 -ffp-contract=off.  hemisphere() is the siblings', handed the table of ball offsets in the directions' place:
//                 the no_normal rule, the origin p + bias n and the rotation k are formed by the same code.
//   any hit       A shadow ray asks "is anything in the way": occluded() (mesh_ray.h) is traverse()'s walk that returns at its
//                 first accepted face.  It answers exactly as traverse() would ("Analytic lights and shadows").
//   determinism   lit[q, l] counts samples; the counts are integer atomics into an array cleared inside the call, the counters
//                 64-bit integer atomics of per-wave ballots.  No float atomics, no thread waits on another: the result is a
//                 pure function of the inputs.  A second, trivial launch turns the counts into float32(lit / S).
//   addresses     Every order row, cell_start entry, pair key and face index is compared with its range before it is used; a
//                 violation sets *overflow and the thread adds nothing.
//   shape         One THREAD per (point in cell order, light, sample), flattened in that order over one-wave blocks
//                 (raycast_kernel's shape): with hard shadows a point has L S = 1 .. 4 rays, and a wave per point would idle
//                 60 lanes.  A wave holds the rays of 64 / (L S) neighbouring points, which start in the same cells.
#include "mesh_ray.h"

namespace gigs {
namespace mesh_shadow {

using namespace gigs::mesh_raycast;

struct ShadowArgs {
  MeshView m;
  int N, L, S, K;
  long long rays;                 // N L S
  const float *points, *normals;  // [N,3] each
  const unsigned char* mask;      // [N] or NULL
  const long long* order;         // [N] or NULL
  const float* lights;            // [L, GIGS_LIGHT_ROW]
  const float* offsets;           // [K,S,3]
  unsigned long long seed;
  double tmax, bias;
  int* lit;                    // [N,L]
  float* visibility;           // [N,L]
  unsigned long long* counts;  // rays cast, blocked, below the horizon, no_normal points, masked points
  int* overflow;
};

enum : int { kIdle = 0, kOpen, kBlocked, kBelow, kNoNormal, kMasked };

__global__ __launch_bounds__(kWave) void shadow_points_kernel(ShadowArgs a) {
  const long long g = (long long)blockIdx.x * kWave + threadIdx.x;
  int what = kIdle;  // this lane's entry in the counters
  bool ok = true;
  if (g < a.rays) {
    const int LS = a.L * a.S;
    const long long i = g / LS;
    const int r = (int)(g - i * LS), l = r / a.S, s = r - l * a.S;
    const long long q = a.order ? a.order[i] : i;
    if (q < 0 || q >= a.N) {
      ok = false;
    } else {
      int* lit = a.lit + (size_t)q * a.L + l;
      const bool masked = a.mask && a.mask[q] == 0;
      Hemisphere h;
      if (masked || !hemisphere(a.points, a.normals, a.offsets, a.S, a.K, a.seed, a.bias, q, (unsigned)s, &h)) {
        atomicAdd(lit, 1);  // no ray is cast: every sample counts as lit
        if (r == 0) what = masked ? kMasked : kNoNormal;
      } else {
        const float* row = a.lights + GIGS_LIGHT_ROW * (size_t)l;
        const double e = (double)row[4];
        double d[3], tmax;
        if (row[0] == 0.0f) {  // a point light: towards the sample on its sphere, which lies at t = 1
#pragma unroll
          for (int c = 0; c < 3; c++) d[c] = ((double)row[1 + c] + e * (double)h.row[c]) - h.o[c];
          tmax = 1.0;
        } else {  // a directional light: against its travel direction, widened by the tangent of its half-angle
#pragma unroll
          for (int c = 0; c < 3; c++) d[c] = (-(double)row[1 + c]) + e * (double)h.row[c];
          tmax = a.tmax;
        }
        if (!(dot3(d, h.n) > 0.0)) {  // d = 0 and a NaN as well
          what = kBelow;
        } else {
          what = occluded(a.m, h.o, d, tmax, &ok) ? kBlocked : kOpen;
          if (ok && what == kOpen) atomicAdd(lit, 1);
        }
      }
    }
  }
  if (!ok) {
    *a.overflow = 1;
    what = kIdle;
  }
  const unsigned long long open = __ballot(what == kOpen), blocked = __ballot(what == kBlocked), below = __ballot(what == kBelow),
                           bad = __ballot(what == kNoNormal), masked = __ballot(what == kMasked);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    if ((open | blocked) != 0ULL) atomicAdd(a.counts, (unsigned long long)__popcll(open | blocked));
    if (blocked != 0ULL) atomicAdd(a.counts + 1, (unsigned long long)__popcll(blocked));
    if (below != 0ULL) atomicAdd(a.counts + 2, (unsigned long long)__popcll(below));
    if (bad != 0ULL) atomicAdd(a.counts + 3, (unsigned long long)__popcll(bad));
    if (masked != 0ULL) atomicAdd(a.counts + 4, (unsigned long long)__popcll(masked));
  }
}

__global__ __launch_bounds__(256) void visibility_kernel(long long n, int S, const int* lit, float* visibility) {
  const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
  if (j < n) visibility[j] = (float)((double)lit[j] / (double)S);
}

}  // namespace mesh_shadow
}  // namespace gigs

extern "C" {

int gigs_mesh_shadow_points(int n_vertices, int n_faces, const float* vertices, const int* faces, const float* lo, double cell,
                            const int* dims, const long long* cell_start, const long long* pair_keys, long long n_pairs,
                            double scale, int n_points, const float* points, const float* normals, const unsigned char* mask,
                            const long long* order, int n_lights, const float* lights, const float* offsets, int n_samples,
                            int n_rotations, unsigned long long seed, double bias, double max_distance, int* lit,
                            float* visibility, unsigned long long* counts, int* overflow, void* stream) {
  using namespace gigs::mesh_shadow;
  ShadowArgs a;
  if (n_points < 0 || !counts || !overflow || !(max_distance >= 0.0) || !(std::fabs(bias) <= DBL_MAX) || n_lights < 1 ||
      n_lights > GIGS_MAX_LIGHTS || n_samples < 1 || n_samples > 64 || n_rotations < 1 || n_rotations > 64 ||
      !make_view(n_vertices, n_faces, vertices, faces, lo, cell, dims, cell_start, pair_keys, n_pairs, scale, &a.m))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_shadow_points: bad argument");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, 5 * sizeof(unsigned long long), s) != hipSuccess)
    return gigs_internal_fail(GIGS_ERR_HIP, "mesh_shadow_points: clear failed");
  if (n_points == 0) return 0;
  if (!points || !normals || !lights || !offsets || !lit || !visibility)
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_shadow_points: NULL array");
  const long long cells = (long long)n_points * n_lights;
  a.rays = cells * n_samples;
  const long long blocks = (a.rays + kWave - 1) / kWave;
  if (blocks > 0x7fffffffLL) return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_shadow_points: too many rays for one launch");
  if (hipMemsetAsync(lit, 0, (size_t)cells * sizeof(int), s) != hipSuccess)
    return gigs_internal_fail(GIGS_ERR_HIP, "mesh_shadow_points: clear failed");
  a.N = n_points, a.L = n_lights, a.S = n_samples, a.K = n_rotations, a.points = points, a.normals = normals, a.mask = mask;
  a.order = order, a.lights = lights, a.offsets = offsets, a.seed = seed, a.tmax = max_distance, a.bias = bias;
  a.lit = lit, a.visibility = visibility, a.counts = counts, a.overflow = overflow;
  hipLaunchKernelGGL(shadow_points_kernel, dim3((unsigned)blocks), dim3(kWave), 0, s, a);
  if (int rc = gigs_internal_check_launch("mesh_shadow_points")) return rc;
  hipLaunchKernelGGL(visibility_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, cells, n_samples, lit, visibility);
  return gigs_internal_check_launch("mesh_shadow_points");
}
}  // extern "C"
