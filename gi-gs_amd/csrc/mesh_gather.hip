// mesh_gather.hip -- ray-traced light per POINT: for any set of surface points with normals (the covered pixels of a
// G-buffer) the open share of the hemisphere, the irradiance under an environment cube shadowed by the mesh, and the diffuse
// light bounced from the mesh's baked radiosity -- a lightmap final gather (mesh.gather_points / mesh.final_gather).
// include/gigs_hip.h, "Ray-traced light per point", states every quantity and tests/mesh_gather_ref.py restates them in numpy.
//
//   arithmetic    mesh_ray.h's as it stands: float64 on the float32 inputs, + - * / only, no sqrt, no transcendental, built
//                 with -ffp-contract=off.  hemisphere() is bake_kernel's and trace_kernel's, handed the POINTS and their normals
//                 in place of the mesh's vertices; traverse, ray_triangle, hemisphere_direction and sky_texel are used as they are.
//   determinism   No float atomics.  A lane adds its chunks' contributions in ascending chunk order and the 64 lane sums meet
//                 in gather_kernel's butterfly S <- S + S[lane xor s], s = 32 .. 1.  The counters are 64-bit integer atomics,
//                 a set per wave.
//   addresses     Every order row, cell_start entry, pair key and face index is compared with its range before it is used; a
//                 violation sets *overflow and the wave stores nothing.  The sky texel is in range by construction.
//   shape         One one-wave block per point, in cell order; the wave loops over the R / 64 chunks, one direction per lane:
//                 trace_kernel's shape for trace_kernel's reason (the 64 lanes share origin and first cells), and no LDS.  Trace and
//                 gather are ONE kernel here: a point is lit once, so there is no record worth 12 bytes a ray.
//   occlusion     hits = the rays whose nearest accepted face has t <= ao_distance.  With a sky the rays are traversed to
//                 max_distance, because light rays see the whole scene.  Without one they are traversed to
//                 min(ao_distance, max_distance) only: a ray has an accepted face within a distance exactly when its NEAREST
//                 accepted face lies there, and which faces are accepted within a distance does not depend on t_max beyond it
//                 (ray_triangle tests t <= t_max last but for the box), so the count is the same and the walk is shorter.
#include "mesh_ray.h"

namespace gigs {
namespace mesh_gather {

using namespace gigs::mesh_raycast;

struct PointArgs {
  MeshView m;
  int N;
  const float *points, *normals;  // [N,3] each
  const unsigned char* mask;      // [N] or NULL
  const long long* order;         // [N] or NULL
  const float* table;             // [K,R,3]
  int R, K, n;                    // n: the cube's edge
  unsigned long long seed;
  double ao, tmax, bias;
  const float *sky, *radiosity;  // [6,n,n,3] or NULL, [V,3] or NULL
  int* hits;                     // [N]
  float *occlusion, *irradiance, *indirect;  // [N], [N,3], [N,3] (the last two NULL iff sky is)
  unsigned long long* counts;                // misses, front hits, back hits, no_normal, masked
  int* overflow;
};

// Three waves a SIMD, trace_kernel's occupancy: left alone the compiler takes 181 VGPRs (two waves); held to 168 it spills 20
// of them to 60 bytes of scratch a lane and the kernel is 22 - 24 % faster on every row measured.
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(3, 3))) void gather_points_kernel(PointArgs a) {
  const unsigned lane = threadIdx.x;
  const long long q = a.order ? a.order[blockIdx.x] : (long long)blockIdx.x;  // the whole wave takes one branch from here on
  if (q < 0 || q >= a.N) {
    *a.overflow = 1;
    return;
  }
  const bool masked = a.mask && a.mask[q] == 0;
  Hemisphere h;
  if (masked || !hemisphere(a.points, a.normals, a.table, a.R, a.K, a.seed, a.bias, q, lane, &h)) {
    if (lane == 0) {
      a.hits[q] = 0;
      a.occlusion[q] = 1.0f;
      atomicAdd(a.counts + (masked ? 4 : 3), 1ULL);
    }
    if (a.sky && lane < 3) a.irradiance[3 * (size_t)q + lane] = 0.0f, a.indirect[3 * (size_t)q + lane] = 0.0f;
    return;
  }
  const double tmax = a.sky ? a.tmax : fmin(a.ao, a.tmax);
  const float* row = h.row;
  unsigned misses = 0, fronts = 0, backs = 0;
  int hits = 0;
  double S[3] = {0.0, 0.0, 0.0}, S_ind[3] = {0.0, 0.0, 0.0};
  for (int j = 0; j < a.R; j += kWave, row += 3 * kWave) {
    double d[3];
    hemisphere_direction(h, row, d);
    Hit best;
    best.t = INFINITY, best.w1 = best.w2 = 0.0, best.sum = 1.0, best.face = -1;
    bool ok = traverse(a.m, h.o, d, tmax, &best);
    int kind = 0;  // 0 a miss, 1 a front hit, 2 a back hit
    double c[3] = {0.0, 0.0, 0.0};
    if (ok && best.face >= 0) {  // which side of the winning face: the sign of d . n_g, n_g from the corners once more
      const int f = best.face;
      ok = f < a.m.F;
      if (ok) {
        const int i0 = a.m.faces[3 * (size_t)f], i1 = a.m.faces[3 * (size_t)f + 1], i2 = a.m.faces[3 * (size_t)f + 2];
        ok = in_range(i0, i1, i2, a.m.V);
        if (ok) {
          double p0[3], p1[3], p2[3], e1[3], e2[3], ng[3];
          load3(a.m.vertices, i0, p0);
          load3(a.m.vertices, i1, p1);
          load3(a.m.vertices, i2, p2);
#pragma unroll
          for (int k = 0; k < 3; k++) e1[k] = p1[k] - p0[k], e2[k] = p2[k] - p0[k];
          cross3(e1, e2, ng);
          kind = dot3(d, ng) < 0.0 ? 1 : 2;
          if (kind == 1 && a.sky && a.radiosity) {  // the weights rounded to float32, as the record path stores them
            const double b1 = (double)(float)(best.w1 / best.sum), b2 = (double)(float)(best.w2 / best.sum);
            const double b0 = fmax(0.0, (1.0 - b1) - b2);
            double q0[3], q1[3], q2[3];
            load3(a.radiosity, i0, q0);
            load3(a.radiosity, i1, q1);
            load3(a.radiosity, i2, q2);
#pragma unroll
            for (int k = 0; k < 3; k++) c[k] = (b0 * q0[k] + b1 * q1[k]) + b2 * q2[k];
          }
        }
      }
    } else if (ok && a.sky) {
      const float* texel = a.sky + 3 * sky_texel(d, a.n);
      c[0] = (double)texel[0], c[1] = (double)texel[1], c[2] = (double)texel[2];
    }
    if (__ballot(!ok) != 0ULL) {
      *a.overflow = 1;
      return;
    }
    hits += __popcll(__ballot(kind != 0 && best.t <= a.ao));
    misses += __popcll(__ballot(kind == 0));
    fronts += __popcll(__ballot(kind == 1));
    backs += __popcll(__ballot(kind == 2));
#pragma unroll
    for (int k = 0; k < 3; k++) {
      S[k] = S[k] + c[k];
      if (kind == 1) S_ind[k] = S_ind[k] + c[k];
    }
  }
  if (a.sky) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
      for (int k = 0; k < 3; k++) {
        S[k] = S[k] + __shfl_xor(S[k], s, (int)kWave);
        S_ind[k] = S_ind[k] + __shfl_xor(S_ind[k], s, (int)kWave);
      }
    }
    if (lane < 3) {
      const double sum = lane == 0 ? S[0] : (lane == 1 ? S[1] : S[2]);
      const double ind = lane == 0 ? S_ind[0] : (lane == 1 ? S_ind[1] : S_ind[2]);
      a.irradiance[3 * (size_t)q + lane] = (float)(sum / (double)a.R);
      a.indirect[3 * (size_t)q + lane] = (float)(ind / (double)a.R);
    }
  }
  if (lane == 0) {
    a.hits[q] = hits;
    a.occlusion[q] = (float)((double)(a.R - hits) / (double)a.R);
    atomicAdd(a.counts, (unsigned long long)misses);
    atomicAdd(a.counts + 1, (unsigned long long)fronts);
    atomicAdd(a.counts + 2, (unsigned long long)backs);
  }
}

}  // namespace mesh_gather
}  // namespace gigs

extern "C" {

int gigs_mesh_gather_points(int n_vertices, int n_faces, const float* vertices, const int* faces, const float* lo, double cell,
                            const int* dims, const long long* cell_start, const long long* pair_keys, long long n_pairs,
                            double scale, int n_points, const float* points, const float* normals, const unsigned char* mask,
                            const long long* order, const float* directions, int n_rays, int n_rotations, unsigned long long seed,
                            double ao_distance, double max_distance, double bias, int sky_res, const float* sky,
                            const float* radiosity, int* hits, float* occlusion, float* irradiance, float* indirect,
                            unsigned long long* counts, int* overflow, void* stream) {
  using namespace gigs::mesh_gather;
  PointArgs a;
  if (n_points < 0 || !counts || !overflow || !(ao_distance >= 0.0) || !hemisphere_args(n_rays, n_rotations, max_distance, bias) ||
      (sky && (sky_res < 1 || sky_res > 4096)) ||
      !make_view(n_vertices, n_faces, vertices, faces, lo, cell, dims, cell_start, pair_keys, n_pairs, scale, &a.m))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_gather_points: bad argument");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, 5 * sizeof(unsigned long long), s) != hipSuccess)
    return gigs_internal_fail(GIGS_ERR_HIP, "mesh_gather_points: clear failed");
  if (n_points == 0) return 0;
  if (!points || !normals || !directions || !hits || !occlusion || (sky && (!irradiance || !indirect)) ||
      (radiosity && n_vertices > 0 && !vertices))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_gather_points: NULL array");
  a.N = n_points, a.points = points, a.normals = normals, a.mask = mask, a.order = order, a.table = directions;
  a.R = n_rays, a.K = n_rotations, a.n = sky_res, a.seed = seed, a.ao = ao_distance, a.tmax = max_distance, a.bias = bias;
  a.sky = sky, a.radiosity = radiosity, a.hits = hits, a.occlusion = occlusion, a.irradiance = irradiance, a.indirect = indirect;
  a.counts = counts, a.overflow = overflow;
  hipLaunchKernelGGL(gather_points_kernel, dim3((unsigned)n_points), dim3(kWave), 0, s, a);
  return gigs_internal_check_launch("mesh_gather_points");
}
}  // extern "C"
