// ssr_apply.hip -- the indirect-diffuse gather over a recorded hit list (gigs_ssr_apply, gigs_ssr_apply_multi): what
// replaces the SSR march (gi.hip) for a view whose geometry does not change.  It never marches; it shares the march's
// tail (gi_march.h: Tbn, ssr_finish) and reads the ray weights from the ray table that gi.hip owns.
//
// Reference behaviour restated (R/ = submodules/diff-gaussian-rasterization): the accumulation and the tail of SSRCUDA,
// R/cuda_rasterizer/forward.cu:824-826 and :832-909 (fresnelSchlick ssr.h:13-16).
#include <type_traits>

#include "gi_march.h"
#include "gigs_internal.h"

namespace gigs {

// The gather that replaces the march for a view whose hit list is known (see SsrHits): per pixel the four waves' hit
// sequences are summed in their recorded order, the four partial sums combined as the march combines them, and the same
// tail evaluated -- the march's outputs bit for bit for the geometry the list was recorded with.
//
// kLights > 1 (gigs_ssr_apply_multi; color and abd are [kLights,3,H,W]): the walk over a pixel's entries is serial and
// every hit is a scattered gather.  Gathering kLights PLANES at a hit touches 3 kLights cache lines, as many as kLights
// single-light passes do, and was measured no faster than them; so the planes of a pass are first packed pixel-major
// (ssr_pack_kernel: `rgb` is then [H W][kQuads] float4, a pixel's 3 kLights values side by side, zero-padded) and a hit is
// kQuads adjacent 16-byte loads -- one or two lines instead of 3 kLights.  Each entry and its ray weights are read once per
// pass.  Every light keeps the single-light arithmetic: per wave slot its own sequence in recorded order, the slots folded
// as ((p0 + p1) + p2) + p3 -- here as they finish, which is the same four-term expression --, then ssr_finish.
template <int kLights>
__global__ void __launch_bounds__(256)
ssr_pack_kernel(size_t HW, const float* __restrict__ rgb, float4* __restrict__ packed) {
  constexpr int kQuads = (3 * kLights + 3) / 4;
  const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= HW) return;
  float v[4 * kQuads];
#pragma unroll
  for (int i = 0; i < 4 * kQuads; i++) v[i] = i < 3 * kLights ? rgb[(size_t)i * HW + q] : 0.0f;  // plane 3 l + c
#pragma unroll
  for (int j = 0; j < kQuads; j++) packed[q * kQuads + j] = make_float4(v[4 * j], v[4 * j + 1], v[4 * j + 2], v[4 * j + 3]);
}

template <int kLights>
__global__ void __launch_bounds__(256)
ssr_apply_kernel(int W, int H, int nrays_total, const float4* __restrict__ rays, const unsigned* __restrict__ offsets,
                 const uint2* __restrict__ entries, const float* __restrict__ nrm, const float* __restrict__ pos_map,
                 const float* __restrict__ rgb, const float* __restrict__ albedo_map, const float* __restrict__ metallic_map,
                 const float* __restrict__ F0_map, float* __restrict__ color, float* __restrict__ abd) {
  const size_t HW = (size_t)H * W;
  const size_t pix_id = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (pix_id >= HW) return;
  const v3 pos = {pos_map[pix_id], pos_map[HW + pix_id], pos_map[2 * HW + pix_id]};
  const Tbn tbn = make_tbn({nrm[pix_id], nrm[HW + pix_id], nrm[2 * HW + pix_id]});
  if constexpr (kLights > 1) {
    constexpr int kQuads = (3 * kLights + 3) / 4;
    v3 sum[kLights];
    // the five offsets of this pixel are one aligned 16-byte load and one more word (offsets is [4 N + 1])
    const uint4 o4 = *reinterpret_cast<const uint4*>(offsets + 4 * pix_id);
    const unsigned bound[5] = {o4.x, o4.y, o4.z, o4.w, offsets[4 * pix_id + 4]};
#pragma unroll
    for (int w = 0; w < 4; w++) {
      v3 d[kLights];
#pragma unroll
      for (int l = 0; l < kLights; l++) d[l] = {0, 0, 0};
      for (unsigned e = bound[w]; e < bound[w + 1]; e++) {
        const uint2 h = entries[e];
        const float cos_t = rays[2 * h.y].w, sin_t = rays[2 * h.y + 1].x;
        // all loads of the hit first: they do not depend on each other
        const float4* src = reinterpret_cast<const float4*>(rgb) + (size_t)h.x * kQuads;
        float c[4 * kQuads];
#pragma unroll
        for (int j = 0; j < kQuads; j++) {
          const float4 t = src[j];
          c[4 * j] = t.x; c[4 * j + 1] = t.y; c[4 * j + 2] = t.z; c[4 * j + 3] = t.w;
        }
#pragma unroll
        for (int l = 0; l < kLights; l++) {
          d[l].x += c[3 * l] * cos_t * sin_t;
          d[l].y += c[3 * l + 1] * cos_t * sin_t;
          d[l].z += c[3 * l + 2] * cos_t * sin_t;
        }
      }
#pragma unroll
      for (int l = 0; l < kLights; l++) {
        if (w == 0) sum[l] = d[l];
        else sum[l] = {sum[l].x + d[l].x, sum[l].y + d[l].y, sum[l].z + d[l].z};
      }
    }
#pragma unroll
    for (int l = 0; l < kLights; l++)
      ssr_finish(sum[l], tbn, pos, pix_id, HW, nrays_total, albedo_map, metallic_map, F0_map, color + (size_t)l * 3 * HW,
                 abd + (size_t)l * 3 * HW);
    return;
  }
  v3 part[4];
#pragma unroll
  for (int w = 0; w < 4; w++) {
    v3 d = {0, 0, 0};
    const unsigned e0 = offsets[4 * pix_id + w], e1 = offsets[4 * pix_id + w + 1];
    for (unsigned e = e0; e < e1; e++) {
      const uint2 h = entries[e];
      const float cos_t = rays[2 * h.y].w, sin_t = rays[2 * h.y + 1].x;
      d.x += rgb[h.x] * cos_t * sin_t;
      d.y += rgb[HW + h.x] * cos_t * sin_t;
      d.z += rgb[2 * HW + h.x] * cos_t * sin_t;
    }
    part[w] = d;
  }
  const v3 diffuse = {((part[0].x + part[1].x) + part[2].x) + part[3].x, ((part[0].y + part[1].y) + part[2].y) + part[3].y,
                      ((part[0].z + part[1].z) + part[2].z) + part[3].z};
  ssr_finish(diffuse, tbn, pos, pix_id, HW, nrays_total, albedo_map, metallic_map, F0_map, color, abd);
}

int launch_ssr_apply(int W, int H, float delta, const unsigned* offsets, const void* entries, const float* normal,
                     const float* pos, const float* rgb, const float* albedo, const float* metallic, const float* F0,
                     float* color, float* abd, hipStream_t s) {
  RayTable t;
  const int rc = get_ray_table(delta, s, t);
  if (rc) return rc;
  const size_t HW = (size_t)W * H;
  hipLaunchKernelGGL(ssr_apply_kernel<1>, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, s, W, H, t.nrays, t.dev, offsets,
                     (const uint2*)entries, normal, pos, rgb, albedo, metallic, F0, color, abd);
  return 0;
}

// K radiance planes over one hit list (gigs_ssr_apply_multi): passes of up to kSsrApplyLights planes, each a pack of its
// planes into `scratch` and one walk over the list (stream-ordered, so the passes share the buffer); a rest of one light is
// the single-light kernel on its plane.  6 kLights accumulators and 3 kLights values in flight per lane: see DESIGN.md,
// "Turntables", for the registers and the measurement; -DGIGS_SSR_APPLY_LIGHTS=4 builds the narrower pass it was compared with.
#ifndef GIGS_SSR_APPLY_LIGHTS
#define GIGS_SSR_APPLY_LIGHTS 8
#endif
constexpr int kSsrApplyLights = GIGS_SSR_APPLY_LIGHTS;
static_assert(kSsrApplyLights == 4 || kSsrApplyLights == 8, "passes of 4 or 8 lights");

size_t ssr_apply_multi_scratch_bytes(int n_lights, int W, int H) {
  const int widest = n_lights < kSsrApplyLights ? n_lights : kSsrApplyLights;
  return widest < 2 ? 0 : (size_t)W * H * ((3 * widest + 3) / 4) * sizeof(float4);
}

int launch_ssr_apply_multi(int n_lights, int W, int H, float delta, const unsigned* offsets, const void* entries,
                           const float* normal, const float* pos, const float* rgb, const float* albedo, const float* metallic,
                           const float* F0, float* color, float* abd, void* scratch, hipStream_t s) {
  RayTable t;
  const int rc = get_ray_table(delta, s, t);
  if (rc) return rc;
  const size_t HW = (size_t)W * H, plane = 3 * HW;
  const dim3 grid((unsigned)((HW + 255) / 256));
  auto pass = [&](auto tag, int l0) {
    constexpr int kLights = decltype(tag)::value;
    const float* src = rgb + l0 * plane;
    if constexpr (kLights > 1) {
      hipLaunchKernelGGL(ssr_pack_kernel<kLights>, grid, dim3(256), 0, s, HW, src, (float4*)scratch);
      src = (const float*)scratch;
    }
    hipLaunchKernelGGL(ssr_apply_kernel<kLights>, grid, dim3(256), 0, s, W, H, t.nrays, t.dev, offsets, (const uint2*)entries,
                       normal, pos, src, albedo, metallic, F0, color + l0 * plane, abd + l0 * plane);
  };
  for (int l0 = 0; l0 < n_lights;) {  // widest pass first
    const int n = n_lights - l0;
    int took;
    if (kSsrApplyLights == 8 && n >= 8) { pass(std::integral_constant<int, 8>{}, l0); took = 8; }
    else if (n >= 4) { pass(std::integral_constant<int, 4>{}, l0); took = 4; }
    else if (n == 3) { pass(std::integral_constant<int, 3>{}, l0); took = 3; }
    else if (n == 2) { pass(std::integral_constant<int, 2>{}, l0); took = 2; }
    else { pass(std::integral_constant<int, 1>{}, l0); took = 1; }
    l0 += took;
  }
  return 0;
}

}  // namespace gigs
