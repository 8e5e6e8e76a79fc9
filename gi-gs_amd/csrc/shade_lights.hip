// shade_lights.hip -- a surface point under L analytic lights: Lambert plus GGX with Smith-correlated masking and Schlick
// Fresnel, evaluated against each light's direction (analytic_lights.shade_lights).  include/gigs_hip.h, "Shading under
// analytic lights", states every expression; they restate pbr/renderutils/bsdf.py's bsdf_pbr (BSDF = 0, min_roughness = 0.08)
// line by line: the clamps at specular_epsilon, the frontfacing test, alpha = roughness^2, (1 - cos)^5 by multiplication.
// Both terms carry the cosine of the light's incidence.
//
//   arithmetic    float32, built with -ffp-contract=off; the device's sqrtf and division.  Only the no_normal rule is
//                 float64: it is mesh_ray.h's, so a point is shaded exactly when the shadow kernel gave it rays.
//   shape         One thread per point, a loop over the lights in ascending order: diffuse and specular are sums in light
//                 order from 0, so the result of two lights is the float32 sum of the two single results.  No atomics.
//   addresses     Every index is in range by construction.
#include <cfloat>
#include <cmath>

#include "gigs_internal.h"

namespace gigs {
namespace shade_lights {

constexpr float kEps = 1e-4f;           // specular_epsilon
constexpr float kMinRoughness = 0.08f;  // min_roughness
constexpr float kPi = 3.14159265358979323846f;

struct ShadeArgs {
  int N, L;
  const float *points, *normals;      // [N,3] each
  const unsigned char* mask;          // [N] or NULL
  const float *albedo, *roughness;    // [N,3], [N]
  const float* metallic;              // [N] or NULL: 0
  const float* campos;                // [3]
  const float *lights, *radiance;     // [L, GIGS_LIGHT_ROW], [L,3]
  const float* visibility;            // [N,L] or NULL: 1
  float *diffuse, *specular;          // [N,3] each
};

__device__ __forceinline__ float dot(const float* a, const float* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }
__device__ __forceinline__ float clamp_eps(float c) { return fminf(fmaxf(c, kEps), 1.0f - kEps); }

// torch.nn.functional.normalize: v / max(|v|, 1e-12)
__device__ __forceinline__ void safe_normalize(const float* v, float* out) {
  const float len = fmaxf(sqrtf(dot(v, v)), 1e-12f);
  out[0] = v[0] / len, out[1] = v[1] / len, out[2] = v[2] / len;
}

// bsdf_lambda_ggx
__device__ __forceinline__ float lambda_ggx(float alphaSqr, float cosTheta) {
  const float c = clamp_eps(cosTheta);
  const float cosThetaSqr = c * c;
  const float tanThetaSqr = (1.0f - cosThetaSqr) / cosThetaSqr;
  return 0.5f * (sqrtf(1.0f + alphaSqr * tanThetaSqr) - 1.0f);
}

__global__ __launch_bounds__(256) void shade_lights_kernel(ShadeArgs a) {
  const unsigned q = blockIdx.x * 256u + threadIdx.x;
  if (q >= (unsigned)a.N) return;
  float diffuse[3] = {0.0f, 0.0f, 0.0f}, specular[3] = {0.0f, 0.0f, 0.0f};
  const float p[3] = {a.points[3 * (size_t)q], a.points[3 * (size_t)q + 1], a.points[3 * (size_t)q + 2]};
  const float n[3] = {a.normals[3 * (size_t)q], a.normals[3 * (size_t)q + 1], a.normals[3 * (size_t)q + 2]};
  const double n2 = ((double)n[0] * (double)n[0] + (double)n[1] * (double)n[1]) + (double)n[2] * (double)n[2];
  const bool finite = fabsf(p[0]) <= FLT_MAX && fabsf(p[1]) <= FLT_MAX && fabsf(p[2]) <= FLT_MAX;
  if (!(a.mask && a.mask[q] == 0) && finite && n2 >= 1.0 - 0x1p-10 && n2 <= 1.0 + 0x1p-10) {
    const float m = a.metallic ? a.metallic[q] : 0.0f, rough = a.roughness[q];
    float kd[3], ks[3];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float base = a.albedo[3 * (size_t)q + c];
      ks[c] = 0.04f * (1.0f - m) + base * m;  // spec_str = 0
      kd[c] = base * (1.0f - m);
    }
    const float view[3] = {a.campos[0] - p[0], a.campos[1] - p[1], a.campos[2] - p[2]};
    float wo[3];
    safe_normalize(view, wo);
    const float alpha = fminf(fmaxf(rough * rough, kMinRoughness * kMinRoughness), 1.0f);
    const float alphaSqr = alpha * alpha;
    const float woDotN = dot(wo, n);
    const float lambdaI = lambda_ggx(alphaSqr, woDotN);
    for (int l = 0; l < a.L; l++) {
      const float* row = a.lights + GIGS_LIGHT_ROW * (size_t)l;
      float wi[3], fall = 1.0f;
      if (row[0] == 0.0f) {  // a point light: the inverse square of its distance
        const float v[3] = {row[1] - p[0], row[2] - p[1], row[3] - p[2]};
        const float v2 = dot(v, v), len = sqrtf(v2);
        wi[0] = v[0] / len, wi[1] = v[1] / len, wi[2] = v[2] / len;
        fall = fmaxf(v2, 1e-8f);
      } else {
        wi[0] = -row[1], wi[1] = -row[2], wi[2] = -row[3];
      }
      const float vis = a.visibility ? a.visibility[(size_t)q * a.L + l] : 1.0f;
      // bsdf_pbr sees the light at p + wi and normalises (p + wi) - p: that is wi, a unit vector already
      float sum[3], h[3];
      const float wiDotN = dot(wi, n);
      const float lambert = (wiDotN > 0.0f ? wiDotN : 0.0f) / kPi;  // a NaN (a light at the point itself) gives 0
      sum[0] = wo[0] + wi[0], sum[1] = wo[1] + wi[1], sum[2] = wo[2] + wi[2];
      safe_normalize(sum, h);
      const float woDotH = dot(wo, h), nDotH = dot(n, h);
      const float cd = clamp_eps(nDotH);
      const float dd = (cd * alphaSqr - cd) * cd + 1.0f;
      const float D = alphaSqr / (dd * dd * kPi);
      const float G = 1.0f / (1.0f + lambdaI + lambda_ggx(alphaSqr, wiDotN));
      const float cf = 1.0f - clamp_eps(woDotH);
      const float cf5 = ((cf * cf) * (cf * cf)) * cf;
      const bool frontfacing = woDotN > kEps && wiDotN > kEps;
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float E = a.radiance[3 * l + c] / fall;
        const float F = ks[c] + (1.0f - ks[c]) * cf5;
        const float spec = frontfacing ? F * D * G * 0.25f / fmaxf(woDotN, kEps) : 0.0f;
        diffuse[c] = diffuse[c] + (vis * E) * (kd[c] * lambert);
        specular[c] = specular[c] + (vis * E) * spec;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < 3; c++) a.diffuse[3 * (size_t)q + c] = diffuse[c], a.specular[3 * (size_t)q + c] = specular[c];
}

}  // namespace shade_lights
}  // namespace gigs

extern "C" {

int gigs_shade_lights(int n_points, const float* points, const float* normals, const unsigned char* mask, const float* albedo,
                      const float* roughness, const float* metallic, const float* campos, int n_lights, const float* lights,
                      const float* radiance, const float* visibility, float* diffuse, float* specular, void* stream) {
  using namespace gigs::shade_lights;
  if (n_points < 0 || n_lights < 1 || n_lights > GIGS_MAX_LIGHTS)
    return gigs_internal_fail(GIGS_ERR_INVALID, "shade_lights: bad argument");
  if (n_points == 0) return 0;
  if (!points || !normals || !albedo || !roughness || !campos || !lights || !radiance || !diffuse || !specular)
    return gigs_internal_fail(GIGS_ERR_INVALID, "shade_lights: NULL array");
  ShadeArgs a;
  a.N = n_points, a.L = n_lights, a.points = points, a.normals = normals, a.mask = mask, a.albedo = albedo;
  a.roughness = roughness, a.metallic = metallic, a.campos = campos, a.lights = lights, a.radiance = radiance;
  a.visibility = visibility, a.diffuse = diffuse, a.specular = specular;
  hipLaunchKernelGGL(shade_lights_kernel, dim3(((unsigned)n_points + 255u) / 256u), dim3(256), 0, (hipStream_t)stream, a);
  return gigs_internal_check_launch("shade_lights");
}
}  // extern "C"
