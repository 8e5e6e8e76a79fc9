// mesh_light.hip -- the light a mesh receives from an environment: the rays of every vertex's hemisphere traced ONCE and what
// each hit RECORDED (mesh.trace_hemispheres), then any number of gathers over the records: the sky where a ray escaped, the
// previous pass's radiosity where it met the front of a face (mesh.gather_light / mesh.bake_light).  include/gigs_hip.h,
// "Baking light", states every quantity and tests/mesh_light_ref.py restates them in numpy.
//
//   arithmetic    mesh_raycast.hip's: float64 on the float32 inputs, + - * / only, no sqrt, no transcendental, built with
//                 -ffp-contract=off.  The rays are bake_kernel's own (mesh_ray.h: one table, one rotation rule, one frame, one
//                 origin), traverse and ray_triangle are used as they are.
//   determinism   No float atomics.  A lane adds its chunks' contributions in ascending chunk order and the 64 lane sums
//                 meet in a butterfly S <- S + S[lane xor s], s = 32 .. 1: IEEE addition is commutative, so every lane ends
//                 with the same bits and numpy restates the pairing.  The counters are 64-bit integer atomics, a set per wave.
//   addresses     Every order row, record and face index is compared with its range before it is used; a violation sets
//                 *overflow and the wave stores nothing more.
//   trace         One one-wave block per vertex, in cell order; the wave loops over the R / 64 chunks, one direction per
//                 lane, and stores the chunk's 64 records side by side.
//   gather        One one-wave block per vertex, one launch per pass.  A ray costs 12 bytes of records and, on a hit, three
//                 indices and nine floats out of arrays that stay in L2.  No LDS is ALLOCATED: the butterfly is 18 cross-lane
//                 shuffles of 64-bit values, each two ds_bpermute through the LDS crossbar (not its memory).
#include "mesh_ray.h"

namespace gigs {
namespace mesh_light {

using namespace gigs::mesh_raycast;

// ---- trace -----------------------------------------------------------------------------------------------------------------
struct TraceArgs {
  MeshView m;
  const float* normals;
  const long long* order;
  const float* table;  // [K,R,3]
  int R, K;
  unsigned long long seed;
  double tmax, bias;
  int* hit_face;               // [V,R]
  float* hit_bary;             // [V,R,2]
  unsigned long long* counts;  // misses, front hits, back hits, no_normal
  int* overflow;
};

__global__ __launch_bounds__(kWave) void trace_kernel(TraceArgs a) {
  const unsigned lane = threadIdx.x;
  const long long v = a.order ? a.order[blockIdx.x] : (long long)blockIdx.x;  // the whole wave takes one branch from here on
  if (v < 0 || v >= a.m.V) {
    *a.overflow = 1;
    return;
  }
  int* face_out = a.hit_face + (size_t)v * a.R + lane;
  float* bary_out = a.hit_bary + 2 * ((size_t)v * a.R + lane);
  Hemisphere h;
  if (!hemisphere(a.m.vertices, a.normals, a.table, a.R, a.K, a.seed, a.bias, v, lane, &h)) {
    for (int j = 0; j < a.R; j += kWave) face_out[j] = -1, bary_out[2 * j] = 0.0f, bary_out[2 * j + 1] = 0.0f;
    if (lane == 0) atomicAdd(a.counts + 3, 1ULL);
    return;
  }
  const float* row = h.row;
  unsigned misses = 0, fronts = 0, backs = 0;
  for (int j = 0; j < a.R; j += kWave, row += 3 * kWave) {
    double d[3];
    hemisphere_direction(h, row, d);
    Hit best;
    best.t = INFINITY, best.w1 = best.w2 = 0.0, best.sum = 1.0, best.face = -1;
    bool ok = traverse(a.m, h.o, d, a.tmax, &best);
    int record = -1;
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
          for (int c = 0; c < 3; c++) e1[c] = p1[c] - p0[c], e2[c] = p2[c] - p0[c];
          cross3(e1, e2, ng);
          record = dot3(d, ng) < 0.0 ? f : -2 - f;
        }
      }
    }
    if (__ballot(!ok) != 0ULL) {
      *a.overflow = 1;
      return;
    }
    face_out[j] = record;
    bary_out[2 * j] = (float)(best.w1 / best.sum);
    bary_out[2 * j + 1] = (float)(best.w2 / best.sum);
    misses += __popcll(__ballot(record == -1));
    fronts += __popcll(__ballot(record >= 0));
    backs += __popcll(__ballot(record <= -2));
  }
  if (lane == 0) {
    atomicAdd(a.counts, (unsigned long long)misses);
    atomicAdd(a.counts + 1, (unsigned long long)fronts);
    atomicAdd(a.counts + 2, (unsigned long long)backs);
  }
}

// ---- gather ----------------------------------------------------------------------------------------------------------------
struct GatherArgs {
  int V, F, R, K, n;  // n: the cube's edge
  const float *vertices, *normals;
  const int* faces;
  const float* table;
  unsigned long long seed;
  const int* hit_face;
  const float* hit_bary;
  const float *sky, *rho, *previous;  // [6,n,n,3], [V,3], [V,3] or NULL (pass 0)
  float *irradiance, *radiosity;      // [V,3] each
  int* overflow;
};

__global__ __launch_bounds__(kWave) void gather_kernel(GatherArgs a) {
  const unsigned lane = threadIdx.x;
  const long long v = blockIdx.x;
  if (v >= a.V) {
    *a.overflow = 1;
    return;
  }
  Hemisphere h;
  if (!hemisphere(a.vertices, a.normals, a.table, a.R, a.K, a.seed, 0.0, v, lane, &h)) {
    if (lane < 3) a.irradiance[3 * (size_t)v + lane] = 0.0f, a.radiosity[3 * (size_t)v + lane] = 0.0f;
    return;
  }
  const int* face_in = a.hit_face + (size_t)v * a.R + lane;
  const float* bary_in = a.hit_bary + 2 * ((size_t)v * a.R + lane);
  const float* row = h.row;
  double S[3] = {0.0, 0.0, 0.0};
  bool ok = true;
  for (int j = 0; j < a.R; j += kWave, row += 3 * kWave) {
    const int record = face_in[j];
    double c[3] = {0.0, 0.0, 0.0};
    if (record == -1) {
      double d[3];
      hemisphere_direction(h, row, d);
      const float* texel = a.sky + 3 * sky_texel(d, a.n);
      c[0] = (double)texel[0], c[1] = (double)texel[1], c[2] = (double)texel[2];
    } else {
      const int f = record >= 0 ? record : -2 - record;  // record <= -2: -2 - record >= 0 without overflow
      if (f < 0 || f >= a.F) {
        ok = false;
      } else if (record >= 0 && a.previous) {
        const int i0 = a.faces[3 * (size_t)f], i1 = a.faces[3 * (size_t)f + 1], i2 = a.faces[3 * (size_t)f + 2];
        if (!in_range(i0, i1, i2, a.V)) {
          ok = false;
        } else {
          const double b1 = (double)bary_in[2 * j], b2 = (double)bary_in[2 * j + 1];
          const double b0 = fmax(0.0, (1.0 - b1) - b2);
          double q0[3], q1[3], q2[3];
          load3(a.previous, i0, q0);
          load3(a.previous, i1, q1);
          load3(a.previous, i2, q2);
#pragma unroll
          for (int k = 0; k < 3; k++) c[k] = (b0 * q0[k] + b1 * q1[k]) + b2 * q2[k];
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 3; k++) S[k] = S[k] + c[k];
  }
  if (__ballot(!ok) != 0ULL) {
    *a.overflow = 1;
    return;
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
#pragma unroll
    for (int k = 0; k < 3; k++) S[k] = S[k] + __shfl_xor(S[k], s, (int)kWave);
  }
  if (lane < 3) {
    const double sum = lane == 0 ? S[0] : (lane == 1 ? S[1] : S[2]);
    const float irr = (float)(sum / (double)a.R);
    a.irradiance[3 * (size_t)v + lane] = irr;
    a.radiosity[3 * (size_t)v + lane] = (float)((double)a.rho[3 * (size_t)v + lane] * (double)irr);
  }
}

}  // namespace mesh_light
}  // namespace gigs

extern "C" {

int gigs_mesh_trace_hemisphere(int n_vertices, int n_faces, const float* vertices, const float* normals, const int* faces,
                               const float* lo, double cell, const int* dims, const long long* cell_start,
                               const long long* pair_keys, long long n_pairs, double scale, const long long* order,
                               const float* directions, int n_rays, int n_rotations, unsigned long long seed, double max_distance,
                               double bias, int* hit_face, float* hit_bary, unsigned long long* counts, int* overflow, void* stream) {
  using namespace gigs::mesh_light;
  TraceArgs a;
  if (!counts || !overflow || !hemisphere_args(n_rays, n_rotations, max_distance, bias) ||
      !make_view(n_vertices, n_faces, vertices, faces, lo, cell, dims, cell_start, pair_keys, n_pairs, scale, &a.m))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_trace_hemisphere: bad argument");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, 4 * sizeof(unsigned long long), s) != hipSuccess)
    return gigs_internal_fail(GIGS_ERR_HIP, "mesh_trace_hemisphere: clear failed");
  if (n_vertices == 0) return 0;
  if (!vertices || !normals || !directions || !hit_face || !hit_bary)
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_trace_hemisphere: NULL array");
  a.normals = normals, a.order = order, a.table = directions, a.R = n_rays, a.K = n_rotations, a.seed = seed;
  a.tmax = max_distance, a.bias = bias, a.hit_face = hit_face, a.hit_bary = hit_bary, a.counts = counts, a.overflow = overflow;
  hipLaunchKernelGGL(trace_kernel, dim3((unsigned)n_vertices), dim3(kWave), 0, s, a);
  return gigs_internal_check_launch("mesh_trace_hemisphere");
}

int gigs_mesh_gather_light(int n_vertices, int n_faces, const float* vertices, const float* normals, const int* faces,
                           const float* directions, int n_rays, int n_rotations, unsigned long long seed, const int* hit_face,
                           const float* hit_bary, int sky_res, const float* sky, const float* reflectance, const float* previous,
                           float* irradiance, float* radiosity, int* overflow, void* stream) {
  using namespace gigs::mesh_light;
  if (n_vertices < 0 || n_faces < 0 || !overflow || !hemisphere_args(n_rays, n_rotations, 0.0, 0.0) || sky_res < 1 || sky_res > 4096)
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_gather_light: bad argument");
  if (n_vertices == 0) return 0;
  if (!vertices || !normals || !directions || !hit_face || !hit_bary || !sky || !reflectance || !irradiance || !radiosity ||
      (n_faces > 0 && !faces))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_gather_light: NULL array");
  GatherArgs a;
  a.V = n_vertices, a.F = n_faces, a.R = n_rays, a.K = n_rotations, a.n = sky_res, a.vertices = vertices, a.normals = normals;
  a.faces = faces, a.table = directions, a.seed = seed, a.hit_face = hit_face, a.hit_bary = hit_bary, a.sky = sky;
  a.rho = reflectance, a.previous = previous, a.irradiance = irradiance, a.radiosity = radiosity, a.overflow = overflow;
  hipLaunchKernelGGL(gather_kernel, dim3((unsigned)n_vertices), dim3(kWave), 0, (hipStream_t)stream, a);
  return gigs_internal_check_launch("mesh_gather_light");
}
}  // extern "C"
