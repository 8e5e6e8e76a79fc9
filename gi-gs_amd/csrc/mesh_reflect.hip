// mesh_reflect.hip -- ray-traced glossy reflections per POINT: for any set of surface points with normals, view directions and
// roughness (the covered pixels of a G-buffer) the radiance a GGX lobe about the mirror direction brings past the mesh -- the
// environment cube where a ray escapes, the mesh's baked radiosity where it meets the front of a face -- and the open share of
// that lobe (mesh.reflect_points), and the few float32 lines that turn such a radiance into the shade's specular_rgb
// (mesh_render.compose_reflections).  include/gigs_hip.h, "Ray-traced reflections per point", states every quantity and
// tests/mesh_reflect_ref.py restates them in numpy.
//
//   arithmetic    The trace: mesh_ray.h's as it stands, float64 on the float32 inputs, + - * / only, no sqrt, no transcendental,
//                 built with -ffp-contract=off.  hemisphere() is gather_points_kernel's with the table base advanced to the
//                 point's roughness level; the table holds HALF vectors, hemisphere_direction gives h, and the ray is the view
//                 direction mirrored about it, l = 2 (v.h) h - v, NOT normalised: ray_triangle takes d.d and sky_texel divides by
//                 the major component.  The compose: float32, shade.hip's shade_pixel_n restated term by term.
//   determinism   No float atomics.  A lane adds its chunks' contributions in ascending chunk order and the 64 lane sums meet
//                 in gather_kernel's butterfly S <- S + S[lane xor s], s = 32 .. 1.  The counters are 64-bit integer atomics,
//                 a set per wave.
//   addresses     Every order row, cell_start entry, pair key and face index is compared with its range before it is used; a
//                 violation sets *overflow and the wave stores nothing.  The level is texel_of's, in [0, L - 1] for any
//                 roughness; the sky texel is in range by construction.
//   shape         gather_points_kernel's: one one-wave block per point, in cell order; the wave loops over the R / 64 chunks, one
//                 half vector per lane, and no LDS.  A ray below the horizon (v.h <= 0 or n.l <= 0) is not traversed: its lane
//                 idles through the chunk, which is the price of one lobe per wave.
#include "mesh_ray.h"

namespace gigs {
namespace mesh_reflect {

using namespace gigs::mesh_raycast;

struct ReflectArgs {
  MeshView m;
  int N;
  const float *points, *normals, *views;  // [N,3] each
  const float* roughness;                 // [N]
  const unsigned char* mask;              // [N] or NULL
  const long long* order;                 // [N] or NULL
  const float* table;                     // [L,K,R,3]
  int R, K, L, n;                         // n: the cube's edge
  unsigned long long seed;
  double tmax, bias;
  const float *sky, *radiosity;  // [6,n,n,3] or NULL, [V,3] or NULL
  float *specular, *reflected;   // [N,3] each (NULL iff sky is)
  float* visibility;             // [N]
  int *valid, *blocked;          // [N] each
  unsigned long long* counts;    // misses, front hits, back hits, below_horizon, no_normal, no_view, masked
  int* overflow;
};

enum { kMisses = 0, kFronts, kBacks, kBelow, kNoNormal, kNoView, kMasked, kCounters };

// Three waves a SIMD, gather_points_kernel's occupancy: left alone the compiler takes 191 VGPRs (two waves, no scratch); held
// to 168 it spills 24 of them to 100 bytes of scratch a lane ("Ray-traced reflections per pixel").
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(3, 3))) void reflect_points_kernel(ReflectArgs a) {
  const unsigned lane = threadIdx.x;
  const long long q = a.order ? a.order[blockIdx.x] : (long long)blockIdx.x;  // the whole wave takes one branch from here on
  if (q < 0 || q >= a.N) {
    *a.overflow = 1;
    return;
  }
  const bool masked = a.mask && a.mask[q] == 0;
  Hemisphere h;
  double v[3];
  int dead = masked ? kMasked : -1;
  if (dead < 0) {
    const int lev = texel_of((double)a.roughness[q], a.L);
    if (!hemisphere(a.points, a.normals, a.table + 3 * ((size_t)lev * a.K * a.R), a.R, a.K, a.seed, a.bias, q, lane, &h))
      dead = kNoNormal;
  }
  if (dead < 0) {
    load3(a.views, (int)q, v);
    const double vv = dot3(v, v);
    if (!finite3(v) || !(vv >= 1.0 - 0x1p-10 && vv <= 1.0 + 0x1p-10)) dead = kNoView;
  }
  if (dead >= 0) {
    if (lane == 0) {
      a.visibility[q] = 1.0f;
      a.valid[q] = 0, a.blocked[q] = 0;
      atomicAdd(a.counts + dead, 1ULL);
    }
    if (a.sky && lane < 3) a.specular[3 * (size_t)q + lane] = 0.0f, a.reflected[3 * (size_t)q + lane] = 0.0f;
    return;
  }
  const float* row = h.row;
  unsigned misses = 0, fronts = 0, backs = 0, below = 0;
  double S[3] = {0.0, 0.0, 0.0}, S_front[3] = {0.0, 0.0, 0.0}, W = 0.0, W_miss = 0.0;
  for (int j = 0; j < a.R; j += kWave, row += 3 * kWave) {
    double hv[3], d[3];
    hemisphere_direction(h, row, hv);
    const double vh = dot3(v, hv);
#pragma unroll
    for (int k = 0; k < 3; k++) d[k] = (2.0 * vh) * hv[k] - v[k];
    const double nl = dot3(h.n, d);
    const bool live = vh > 0.0 && nl > 0.0;
    const double w = live ? nl : 0.0;
    bool ok = true;
    int kind = -1;  // -1 below the horizon, 0 a miss, 1 a front hit, 2 a back hit
    double c[3] = {0.0, 0.0, 0.0};
    if (live) {
      Hit best;
      best.t = INFINITY, best.w1 = best.w2 = 0.0, best.sum = 1.0, best.face = -1;
      ok = traverse(a.m, h.o, d, a.tmax, &best);
      kind = 0;
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
            if (kind == 1 && a.sky && a.radiosity) {  // the weights rounded to float32, as gather_points_kernel takes them
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
    }
    if (__ballot(!ok) != 0ULL) {
      *a.overflow = 1;
      return;
    }
    below += __popcll(__ballot(kind < 0));
    misses += __popcll(__ballot(kind == 0));
    fronts += __popcll(__ballot(kind == 1));
    backs += __popcll(__ballot(kind == 2));
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double wc = w * c[k];
      S[k] = S[k] + wc;
      S_front[k] = S_front[k] + (kind == 1 ? wc : 0.0);
    }
    W = W + w;
    W_miss = W_miss + (kind == 0 ? w : 0.0);
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    if (a.sky) {
#pragma unroll
      for (int k = 0; k < 3; k++) {
        S[k] = S[k] + __shfl_xor(S[k], s, (int)kWave);
        S_front[k] = S_front[k] + __shfl_xor(S_front[k], s, (int)kWave);
      }
    }
    W = W + __shfl_xor(W, s, (int)kWave);
    W_miss = W_miss + __shfl_xor(W_miss, s, (int)kWave);
  }
  const bool none = !(W > 0.0);  // no valid ray: nothing is reflected and nothing is in the way
  if (a.sky && lane < 3) {
    const double sum = lane == 0 ? S[0] : (lane == 1 ? S[1] : S[2]);
    const double front = lane == 0 ? S_front[0] : (lane == 1 ? S_front[1] : S_front[2]);
    a.specular[3 * (size_t)q + lane] = none ? 0.0f : (float)(sum / W);
    a.reflected[3 * (size_t)q + lane] = none ? 0.0f : (float)(front / W);
  }
  if (lane == 0) {
    a.visibility[q] = none ? 1.0f : (float)(W_miss / W);
    a.valid[q] = (int)(misses + fronts + backs);
    a.blocked[q] = (int)(fronts + backs);
    atomicAdd(a.counts + kMisses, (unsigned long long)misses);
    atomicAdd(a.counts + kFronts, (unsigned long long)fronts);
    atomicAdd(a.counts + kBacks, (unsigned long long)backs);
    atomicAdd(a.counts + kBelow, (unsigned long long)below);
  }
}

// ---- the compose: shade.hip's shade_pixel_n, the specular half, on a supplied radiance -----------------------------------------
struct ComposeArgs {
  int N;
  const float *normals, *views, *albedo;  // [N,3] each
  const float *roughness, *metallic;      // [N], [N] or NULL
  const unsigned char* mask;              // [N] or NULL
  const float *radiance, *visibility;     // [N,3], [N] or NULL
  const float* lut;
  int lut_w, lut_h;
  float* out;  // [N,3]
};

__global__ __launch_bounds__(256) void reflect_compose_kernel(ComposeArgs A) {
  const int p = item<256>(A.N);
  if (p < 0) return;
  const size_t e = 3 * (size_t)p;
  if (A.mask && A.mask[p] == 0) {
    A.out[e] = 0.0f, A.out[e + 1] = 0.0f, A.out[e + 2] = 0.0f;
    return;
  }
  const float nx = A.normals[e], ny = A.normals[e + 1], nz = A.normals[e + 2];
  const float vx = A.views[e], vy = A.views[e + 1], vz = A.views[e + 2];
  const float r = A.roughness[p];
  // shade_pixel_n forms the dot product on the swizzled vectors (-y, z, -x): the y term first, then z, then x
  const float nov = fminf(fmaxf(((-ny) * (-vy) + nz * vz) + (-nx) * (-vx), 1e-4f), 1.0f);
  const float fu = nov * (float)A.lut_w - 0.5f, fv = r * (float)A.lut_h - 0.5f;
  const float flu = floorf(fu), flv = floorf(fv);
  const float tu = fu - flu, tv = fv - flv;
  const int x0 = min(A.lut_w - 1, max(0, (int)flu)), x1 = min(A.lut_w - 1, max(0, (int)flu + 1));
  const int y0 = min(A.lut_h - 1, max(0, (int)flv)), y1 = min(A.lut_h - 1, max(0, (int)flv + 1));
  const float2 t00 = reinterpret_cast<const float2*>(A.lut)[(size_t)y0 * A.lut_w + x0];
  const float2 t10 = reinterpret_cast<const float2*>(A.lut)[(size_t)y0 * A.lut_w + x1];
  const float2 t01 = reinterpret_cast<const float2*>(A.lut)[(size_t)y1 * A.lut_w + x0];
  const float2 t11 = reinterpret_cast<const float2*>(A.lut)[(size_t)y1 * A.lut_w + x1];
  const float w00 = (1 - tu) * (1 - tv), w10 = tu * (1 - tv), w01 = (1 - tu) * tv, w11 = tu * tv;
  const float fgx = t00.x * w00 + t10.x * w10 + t01.x * w01 + t11.x * w11;
  const float fgy = t00.y * w00 + t10.y * w10 + t01.y * w01 + t11.y * w11;
  const float vis = A.visibility ? A.visibility[p] : 1.0f;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float F0 = 0.04f;
    if (A.metallic) {
      const float m = A.metallic[p];
      F0 = (1.0f - m) * 0.04f + A.albedo[e + c] * m;
    }
    const float refl = F0 * fgx + fgy;
    const float sp = A.visibility ? A.radiance[e + c] * vis : A.radiance[e + c];
    A.out[e + c] = sp * refl;
  }
}

}  // namespace mesh_reflect
}  // namespace gigs

extern "C" {

int gigs_mesh_reflect_points(int n_vertices, int n_faces, const float* vertices, const int* faces, const float* lo, double cell,
                             const int* dims, const long long* cell_start, const long long* pair_keys, long long n_pairs,
                             double scale, int n_points, const float* points, const float* normals, const float* views,
                             const float* roughness, const unsigned char* mask, const long long* order, const float* directions,
                             int n_levels, int n_rays, int n_rotations, unsigned long long seed, double max_distance, double bias,
                             int sky_res, const float* sky, const float* radiosity, float* specular, float* reflected,
                             float* visibility, int* valid, int* blocked, unsigned long long* counts, int* overflow,
                             void* stream) {
  using namespace gigs::mesh_reflect;
  ReflectArgs a;
  if (n_points < 0 || !counts || !overflow || n_levels < 1 || n_levels > 64 ||
      !hemisphere_args(n_rays, n_rotations, max_distance, bias) || (sky && (sky_res < 1 || sky_res > 4096)) ||
      !make_view(n_vertices, n_faces, vertices, faces, lo, cell, dims, cell_start, pair_keys, n_pairs, scale, &a.m))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_reflect_points: bad argument");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, kCounters * sizeof(unsigned long long), s) != hipSuccess)
    return gigs_internal_fail(GIGS_ERR_HIP, "mesh_reflect_points: clear failed");
  if (n_points == 0) return 0;
  if (!points || !normals || !views || !roughness || !directions || !visibility || !valid || !blocked ||
      (sky && (!specular || !reflected)) || (radiosity && n_vertices > 0 && !vertices))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_reflect_points: NULL array");
  a.N = n_points, a.points = points, a.normals = normals, a.views = views, a.roughness = roughness, a.mask = mask, a.order = order;
  a.table = directions, a.R = n_rays, a.K = n_rotations, a.L = n_levels, a.n = sky_res, a.seed = seed, a.tmax = max_distance;
  a.bias = bias, a.sky = sky, a.radiosity = radiosity, a.specular = specular, a.reflected = reflected, a.visibility = visibility;
  a.valid = valid, a.blocked = blocked, a.counts = counts, a.overflow = overflow;
  hipLaunchKernelGGL(reflect_points_kernel, dim3((unsigned)n_points), dim3(kWave), 0, s, a);
  return gigs_internal_check_launch("mesh_reflect_points");
}

int gigs_reflect_compose(int n_points, const float* normals, const float* views, const float* albedo, const float* roughness,
                         const float* metallic, const unsigned char* mask, const float* radiance, const float* visibility,
                         const float* lut, int lut_w, int lut_h, float* specular_rgb, void* stream) {
  using namespace gigs::mesh_reflect;
  if (n_points < 0 || lut_w <= 0 || lut_h <= 0) return gigs_internal_fail(GIGS_ERR_INVALID, "reflect_compose: bad argument");
  if (n_points == 0) return 0;
  if (!normals || !views || !roughness || !radiance || !lut || !specular_rgb || (metallic && !albedo))
    return gigs_internal_fail(GIGS_ERR_INVALID, "reflect_compose: NULL array");
  ComposeArgs A;
  A.N = n_points, A.normals = normals, A.views = views, A.albedo = albedo, A.roughness = roughness, A.metallic = metallic;
  A.mask = mask, A.radiance = radiance, A.visibility = visibility, A.lut = lut, A.lut_w = lut_w, A.lut_h = lut_h;
  A.out = specular_rgb;
  hipLaunchKernelGGL(reflect_compose_kernel, dim3(blocks_for(n_points, 256)), dim3(256), 0, (hipStream_t)stream, A);
  return gigs_internal_check_launch("reflect_compose");
}
}  // extern "C"
