// shade.hip -- deferred split-sum shade of the G-buffer, forward (plain, with the G-buffer post-processing, under K
// lights) and backward.
//
// Reference behaviour restated:
//   pbr_shading                          pbr/shade.py:108-241
//   CubemapLight.get_mip                 pbr/light.py:142-152
// The three texture lookups of the shade go through cube.h's cube_taps / cube_sample.
//
// MI355X design
//   * shade forward/backward are ONE fused kernel each, one lane per pixel: the reference runs
//     ~40 small torch kernels + 3 texture ops over the same 640k pixels; fused, the pass reads
//     each G-buffer plane once (~80 B/pixel) and is bound by the gathers into the light
//     textures, which are small (diffuse 18 KB, specular mips 6.3 MB) and stay in L2;
//   * gradients of the light textures: the 16x16x6 diffuse map is accumulated per workgroup in
//     LDS (ds_add_f32, 18 KB) and flushed once, the specular mips take global float atomics.
#include <cmath>
#include <cstdlib>
#include <cstring>

#include "cube.h"

namespace gigs {

struct ShadeArgs {
  int H, W;
  const float *normals, *view_dirs, *albedo, *roughness;
  const uint8_t* mask;
  const float *occlusion, *metallic, *background;
  const float* diffuse; int diffuse_res;
  int L; const float* spec[8]; int spec_res[8];
  const float* lut; int lut_w, lut_h;
  int tone, gamma;
#ifdef GIGS_DIAG
  int ablate;  // -DGIGS_DIAG builds only (tools/gpu_ablate_shade.sh, env GIGS_ABLATE): bit 0 skips the diffuse-map atomics, bit 1 the specular ones
#endif
  // backward: gradient textures small enough to be accumulated per workgroup in LDS
  int lds_total;        // floats of dynamic LDS
  int lds_diffuse_off;  // offset (floats) of the diffuse-map accumulator, or -1
  int lds_spec_off[8];  // per specular level, or -1
  // forward outputs
  float *render_rgb, *diffuse_rgb, *specular_rgb, *diffuse_light;
  // backward inputs (may be null) and outputs
  const float *g_render, *g_diffuse_rgb, *g_specular_rgb, *g_diffuse_light;
  float *d_albedo, *d_roughness, *d_metallic, *d_diffuse;
  float* d_spec[8];
  // layout of normals / albedo and of every [H,W,3] output and gradient: element (p, c) at p * ps + c * cs
  // ([H,W,3]: ps = 3, cs = 1;  [3,H,W] planes: ps = 1, cs = H*W).  view_dirs is always [H,W,3].
  int ps, cs;
  // gigs_shade_ext (stage-2 fusion): roughness = raw * rough_scale + rough_bias, extra outputs / gradients
  float rough_scale, rough_bias;
  float *out_F0, *out_linear, *out_roughness;
  const float *g_albedo_mul_a, *g_albedo_mul_b, *g_roughness_add, *g_metallic_add;
  const float *g_scale, *lamb_mask, *lamb_acc4;
};

__device__ __forceinline__ float get_mip(float r, int L, float& dmip_dr) {  // pbr/light.py:142-152
  const float MINR = 0.08f, MAXR = 0.5f;
  if (r < MAXR) {
    const float c = fminf(fmaxf(r, MINR), MAXR);
    dmip_dr = (r >= MINR && r <= MAXR) ? (1.0f / (MAXR - MINR)) * (float)(L - 2) : 0.0f;
    return (c - MINR) / (MAXR - MINR) * (float)(L - 2);
  }
  const float c = fminf(fmaxf(r, MAXR), 1.0f);
  dmip_dr = (r >= MAXR && r <= 1.0f) ? 1.0f / (1.0f - MAXR) : 0.0f;
  return (c - MAXR) / (1.0f - MAXR) + (float)L - 2.0f;
}
__device__ __forceinline__ float aces(float x, float& d) {  // pbr/shade.py:33-47
  const float a = 2.51f, b = 0.03f, c = 2.43f, dd = 0.59f, e = 0.14f;
  const float num = x * (a * x + b), den = x * (c * x + dd) + e;
  d = ((2 * a * x + b) * den - num * (2 * c * x + dd)) / (den * den);
  return num / den;
}

// What the specular lookup of a pixel reads: the level pair of its roughness and the four bilinear taps of the reflected
// direction in each of the two levels.  shade_pixel_n samples through it and spec_tap_census_kernel marks through it: one
// function, so the texels the census lists are the texels the shade reads.
struct SpecTaps {
  float lf, dmdr;
  int l0, l1;
  bool lvl_inside;
  Taps t0, t1;
  bool has0, has1;  // has1 only where l1 != l0
};

// r: the shading roughness, n: the shading normal, v: the view direction.  The library is compiled with
// -ffp-contract=off (build.py: part of its numerical contract), so the expressions below are the same IEEE operations in
// every kernel this is inlined into: the census and the shade get the same taps from the same inputs, bit for bit.
__device__ __forceinline__ void spec_taps(int L, const int (&spec_res)[8], float r, v3 n, v3 v, SpecTaps& q) {
  const float ndv = n.x * v.x + n.y * v.y + n.z * v.z;
  const float c2 = 2.0f * fmaxf(ndv, 0.0f);
  const v3 ref = {c2 * n.x - v.x, c2 * n.y - v.y, c2 * n.z - v.z};
  const v3 rt = {-ref.y, ref.z, -ref.x};
  const float lvl_raw = get_mip(r, L, q.dmdr);
  const float lvl = fminf(fmaxf(lvl_raw, 0.0f), (float)(L - 1));
  q.lvl_inside = lvl_raw >= 0.0f && lvl_raw <= (float)(L - 1);
  q.l0 = min((int)floorf(lvl), L - 1);
  q.l1 = min(q.l0 + 1, L - 1);
  q.lf = lvl - (float)q.l0;
  q.has0 = cube_taps(spec_res[q.l0], rt.x, rt.y, rt.z, q.t0);
  q.has1 = false;
  if (q.l1 != q.l0) q.has1 = cube_taps(spec_res[q.l1], rt.x, rt.y, rt.z, q.t1);
}

// Everything both passes need, computed identically in forward and backward.
struct ShadePix : SpecTaps {
  v3 a, dl_raw, dl, drgb, sp, s0, s1, F0, refl, srgb;
  float r, occ, m, fgx, fgy, dfgx_dv, dfgy_dv;
  Taps td;
  bool has_d;
};

// n: the shading normal of pixel p (A.normals' value, or the one the caller has just formed in registers)
__device__ __forceinline__ void shade_pixel_n(const ShadeArgs& A, int p, v3 n, ShadePix& q) {
  const size_t e = (size_t)p * A.ps, cs = A.cs;
  const v3 v = {A.view_dirs[3 * p], A.view_dirs[3 * p + 1], A.view_dirs[3 * p + 2]};
  q.a = {A.albedo[e], A.albedo[e + cs], A.albedo[e + 2 * cs]};
  q.r = A.roughness[p] * A.rough_scale + A.rough_bias;  // scale 1, bias 0 (exact) unless the caller fuses the remap
  const v3 nt = {-n.y, n.z, -n.x}, vt = {-v.y, v.z, -v.x};
  q.has_d = cube_taps(A.diffuse_res, nt.x, nt.y, nt.z, q.td);
  q.dl_raw = q.has_d ? cube_sample(A.diffuse, q.td) : v3{0, 0, 0};
  q.occ = A.occlusion ? A.occlusion[p] : 1.0f;
  q.dl = A.occlusion ? q.dl_raw * q.occ : q.dl_raw;
  q.drgb = {q.dl.x * q.a.x, q.dl.y * q.a.y, q.dl.z * q.a.z};
  const float nov = fminf(fmaxf(nt.x * vt.x + nt.y * vt.y + nt.z * vt.z, 1e-4f), 1.0f);
  {
    const float fu = nov * (float)A.lut_w - 0.5f, fv = q.r * (float)A.lut_h - 0.5f;
    const float flu = floorf(fu), flv = floorf(fv);
    const float tu = fu - flu, tv = fv - flv;
    const int x0 = min(A.lut_w - 1, max(0, (int)flu)), x1 = min(A.lut_w - 1, max(0, (int)flu + 1));
    const int y0 = min(A.lut_h - 1, max(0, (int)flv)), y1 = min(A.lut_h - 1, max(0, (int)flv + 1));
    const float2 t00 = reinterpret_cast<const float2*>(A.lut)[(size_t)y0 * A.lut_w + x0];
    const float2 t10 = reinterpret_cast<const float2*>(A.lut)[(size_t)y0 * A.lut_w + x1];
    const float2 t01 = reinterpret_cast<const float2*>(A.lut)[(size_t)y1 * A.lut_w + x0];
    const float2 t11 = reinterpret_cast<const float2*>(A.lut)[(size_t)y1 * A.lut_w + x1];
    const float w00 = (1 - tu) * (1 - tv), w10 = tu * (1 - tv), w01 = (1 - tu) * tv, w11 = tu * tv;
    q.fgx = t00.x * w00 + t10.x * w10 + t01.x * w01 + t11.x * w11;
    q.fgy = t00.y * w00 + t10.y * w10 + t01.y * w01 + t11.y * w11;
    // d/dv of the bilinear blend (taps fixed), times dv/d(roughness) = lut_h
    q.dfgx_dv = ((t01.x - t00.x) * (1 - tu) + (t11.x - t10.x) * tu) * (float)A.lut_h;
    q.dfgy_dv = ((t01.y - t00.y) * (1 - tu) + (t11.y - t10.y) * tu) * (float)A.lut_h;
  }
  spec_taps(A.L, A.spec_res, q.r, n, v, q);
  q.s0 = q.has0 ? cube_sample(A.spec[q.l0], q.t0) : v3{0, 0, 0};
  q.s1 = {0, 0, 0};
  if (q.l1 != q.l0) {
    if (q.has1) q.s1 = cube_sample(A.spec[q.l1], q.t1);
    q.sp = {q.s0.x * (1 - q.lf) + q.s1.x * q.lf, q.s0.y * (1 - q.lf) + q.s1.y * q.lf, q.s0.z * (1 - q.lf) + q.s1.z * q.lf};
  } else {
    q.sp = q.s0;
  }
  if (A.metallic) {
    q.m = A.metallic[p];
    q.F0 = {(1.0f - q.m) * 0.04f + q.a.x * q.m, (1.0f - q.m) * 0.04f + q.a.y * q.m, (1.0f - q.m) * 0.04f + q.a.z * q.m};
  } else {
    q.m = 0.0f;
    q.F0 = {0.04f, 0.04f, 0.04f};
  }
  q.refl = {q.F0.x * q.fgx + q.fgy, q.F0.y * q.fgx + q.fgy, q.F0.z * q.fgx + q.fgy};
  q.srgb = {q.sp.x * q.refl.x, q.sp.y * q.refl.y, q.sp.z * q.refl.z};
}

__device__ __forceinline__ void shade_pixel(const ShadeArgs& A, int p, ShadePix& q) {
  const size_t e = (size_t)p * A.ps, cs = A.cs;
  shade_pixel_n(A, p, {A.normals[e], A.normals[e + cs], A.normals[e + 2 * cs]}, q);
}

// one channel of the rendered colour: gamma(clamp(tone(x)))
__device__ __forceinline__ float shade_tone_map(const ShadeArgs& A, float x) {
  float dd;
  if (A.tone) x = aces(x, dd);
  x = fminf(fmaxf(x, 0.0f), 1.0f);
  if (A.gamma) x = lin2srgb(x, dd);
  return x;
}

// the forward's epilogue: tone map / gamma, mask, every output plane (mk: the pixel's normal mask)
__device__ __forceinline__ void shade_fwd_store(const ShadeArgs& A, int p, const ShadePix& q, bool mk) {
  float rr[3] = {q.drgb.x + q.srgb.x, q.drgb.y + q.srgb.y, q.drgb.z + q.srgb.z};
  float dd;
#pragma unroll
  for (int c = 0; c < 3; c++) rr[c] = shade_tone_map(A, rr[c]);
  v3 drgb = q.drgb, srgb = q.srgb;
  if (A.gamma) {
    drgb = {lin2srgb(drgb.x, dd), lin2srgb(drgb.y, dd), lin2srgb(drgb.z, dd)};
    srgb = {lin2srgb(srgb.x, dd), lin2srgb(srgb.y, dd), lin2srgb(srgb.z, dd)};
  }
  const size_t e = (size_t)p * A.ps, cs = A.cs;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    rr[c] = mk ? rr[c] : (A.background ? A.background[e + c * cs] : 0.0f);
    A.render_rgb[e + c * cs] = rr[c];
  }
  if (A.diffuse_rgb) { A.diffuse_rgb[e] = drgb.x; A.diffuse_rgb[e + cs] = drgb.y; A.diffuse_rgb[e + 2 * cs] = drgb.z; }
  if (A.specular_rgb) { A.specular_rgb[e] = srgb.x; A.specular_rgb[e + cs] = srgb.y; A.specular_rgb[e + 2 * cs] = srgb.z; }
  if (A.diffuse_light) { A.diffuse_light[e] = q.dl.x; A.diffuse_light[e + cs] = q.dl.y; A.diffuse_light[e + 2 * cs] = q.dl.z; }
  if (A.out_F0) { A.out_F0[e] = q.F0.x; A.out_F0[e + cs] = q.F0.y; A.out_F0[e + 2 * cs] = q.F0.z; }
  if (A.out_linear) {
#pragma unroll
    for (int c = 0; c < 3; c++) A.out_linear[e + c * cs] = srgb2lin(rr[c]);
  }
  if (A.out_roughness) A.out_roughness[p] = q.r;
}

__global__ void __launch_bounds__(256)
shade_fwd_kernel(ShadeArgs A) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= A.H * A.W) return;
  ShadePix q;
  shade_pixel(A, p, q);
  shade_fwd_store(A, p, q, A.mask[p] != 0);
}

// gigs_shade_fwd_post: the G-buffer post-processing of stage2.hip's gbuffer_post_kernel<false> and shade_fwd_kernel in one
// launch (planar layout).  A workgroup (64 x 4 pixels) stages normalize_where(normal_map) and
// normalize_where(out_normal_view) for its tile and a 1-pixel halo in LDS -- each tap normalised once, not once per
// window it belongs to; padding taps are zero --, every lane forms its six medians, the rotation and the mask from
// there in gbuffer_post_kernel's expressions, stores normals_view / mask / onv (the backward and SSR read them) and
// shades its pixel from the normal and the mask it holds in registers.
struct ShadePostArgs {
  const float *normal_map, *out_normal_view, *vm;
  float* normals_view;
  uint8_t* mask_u8;
  float *mask_f, *onv;
};
constexpr int kPostW = 64, kPostH = 4;
typedef float PostTile[3][kPostH + 2][kPostW + 2];

// normalize_where(src) of the workgroup's 64 x 4 tile and its 1-pixel halo; taps outside the image are zero
__device__ __forceinline__ void post_stage(PostTile& s, const float* __restrict__ src, int H, int W) {
  const size_t HW = (size_t)H * W;
  constexpr int kHalo = (kPostH + 2) * (kPostW + 2);
  for (int r = threadIdx.x; r < kHalo; r += 256) {
    const int ty = r / (kPostW + 2), tx = r - ty * (kPostW + 2);
    const int yy = (int)blockIdx.y * kPostH - 1 + ty, xx = (int)blockIdx.x * kPostW - 1 + tx;
    v3 v = {0.0f, 0.0f, 0.0f};
    if (!(yy < 0 || yy >= H || xx < 0 || xx >= W)) {
      const size_t t = (size_t)yy * W + xx;
      v = normalize_where({src[t], src[HW + t], src[2 * HW + t]});
    }
    s[0][ty][tx] = v.x; s[1][ty][tx] = v.y; s[2][ty][tx] = v.z;
  }
}

// the three medians of the lane's 3 x 3 window; a NaN in the window -> NaN (median_of_normalized)
__device__ __forceinline__ void post_median(const PostTile& s, int lx, int ly, float (&med)[3]) {
#pragma unroll
  for (int c = 0; c < 3; c++) {
    float t[9];
    bool has_nan = false;
    int k = 0;
#pragma unroll
    for (int dy = 0; dy <= 2; dy++)
#pragma unroll
      for (int dx = 0; dx <= 2; dx++, k++) {
        t[k] = s[c][ly + dy][lx + dx];
        has_nan |= t[k] != t[k];
      }
    med[c] = has_nan ? __builtin_nanf("") : median9(t);
  }
}

// -(n @ R), R = viewmatrix[:3, :3] of the row-major 4x4 tensor
__device__ __forceinline__ v3 post_rotate(const float* __restrict__ vm, const float (&m)[3]) {
  return {-(m[0] * vm[0] + m[1] * vm[4] + m[2] * vm[8]),
          -(m[0] * vm[1] + m[1] * vm[5] + m[2] * vm[9]),
          -(m[0] * vm[2] + m[1] * vm[6] + m[2] * vm[10])};
}

// the normal mask of the stage-2 step: every channel of normal_map is nonzero
__device__ __forceinline__ bool post_mask(const float* __restrict__ normal_map, size_t HW, int p) {
  return normal_map[p] != 0.0f && normal_map[HW + p] != 0.0f && normal_map[2 * HW + p] != 0.0f;
}

__global__ void __launch_bounds__(256)
shade_fwd_post_kernel(ShadeArgs A, ShadePostArgs P) {
  __shared__ PostTile s_n[2];
  const int H = A.H, W = A.W;
  const size_t HW = (size_t)H * W;
  post_stage(s_n[0], P.normal_map, H, W);
  post_stage(s_n[1], P.out_normal_view, H, W);
  __syncthreads();
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const int x = blockIdx.x * kPostW + lx, y = blockIdx.y * kPostH + ly;
  if (x >= W || y >= H) return;
  const int p = y * W + x;
  const bool mk = post_mask(P.normal_map, HW, p);
  P.mask_u8[p] = mk ? 1 : 0;
  if (P.mask_f) P.mask_f[p] = mk ? 1.0f : 0.0f;
  float med[2][3];
  post_median(s_n[0], lx, ly, med[0]);
  post_median(s_n[1], lx, ly, med[1]);
  const v3 n = post_rotate(P.vm, med[0]);
  P.normals_view[p] = n.x; P.normals_view[HW + p] = n.y; P.normals_view[2 * HW + p] = n.z;
  P.onv[p] = med[1][0]; P.onv[HW + p] = med[1][1]; P.onv[2 * HW + p] = med[1][2];
  ShadePix q;
  shade_pixel_n(A, p, n, q);
  shade_fwd_store(A, p, q, mk);
}

// gigs_shade_fwd_multi: the planar forward under K lights.  shade_pixel runs once, with light 0; for every further light
// only the cube_sample reads and the arithmetic behind them are repeated, on the same taps, in shade_pixel's expressions,
// and the epilogue is shade_fwd_store's shade_tone_map (render_rgb and out_linear only) -- light k bit for bit as a
// single-light call.
constexpr int kShadeMaxLights = 16;  // GIGS_MAX_LIGHTS (include/gigs_hip.h)
struct ShadeLights {
  int K;
  const float* diffuse[kShadeMaxLights];
  const float* spec[kShadeMaxLights][8];
};

__device__ __forceinline__ void shade_relight(const ShadeArgs& A, const float* __restrict__ diffuse,
                                              const float* const* spec, ShadePix& q) {
  q.dl_raw = q.has_d ? cube_sample(diffuse, q.td) : v3{0, 0, 0};
  q.dl = A.occlusion ? q.dl_raw * q.occ : q.dl_raw;
  q.drgb = {q.dl.x * q.a.x, q.dl.y * q.a.y, q.dl.z * q.a.z};
  q.s0 = q.has0 ? cube_sample(spec[q.l0], q.t0) : v3{0, 0, 0};
  q.s1 = {0, 0, 0};
  if (q.l1 != q.l0) {
    if (q.has1) q.s1 = cube_sample(spec[q.l1], q.t1);
    q.sp = {q.s0.x * (1 - q.lf) + q.s1.x * q.lf, q.s0.y * (1 - q.lf) + q.s1.y * q.lf, q.s0.z * (1 - q.lf) + q.s1.z * q.lf};
  } else {
    q.sp = q.s0;
  }
  q.srgb = {q.sp.x * q.refl.x, q.sp.y * q.refl.y, q.sp.z * q.refl.z};
}

__global__ void __launch_bounds__(256)
shade_fwd_multi_kernel(ShadeArgs A, ShadeLights Ls) {
  const int p = blockIdx.x * 256 + threadIdx.x;
  if (p >= A.H * A.W) return;
  ShadePix q;
  shade_pixel(A, p, q);  // A.diffuse / A.spec are light 0's
  const bool mk = A.mask[p] != 0;
  const size_t plane = 3 * (size_t)A.cs;
  for (int k = 0; k < Ls.K; k++) {
    if (k > 0) shade_relight(A, Ls.diffuse[k], Ls.spec[k], q);
    float rr[3] = {q.drgb.x + q.srgb.x, q.drgb.y + q.srgb.y, q.drgb.z + q.srgb.z};
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float x = shade_tone_map(A, rr[c]);  // unconditionally: a select, not a branch on the mask
      rr[c] = mk ? x : 0.0f;
    }
    float* out = A.render_rgb + k * plane;
#pragma unroll
    for (int c = 0; c < 3; c++) out[p + c * (size_t)A.cs] = rr[c];
    if (A.out_linear) {
      float* lin = A.out_linear + k * plane;
#pragma unroll
      for (int c = 0; c < 3; c++) lin[p + c * (size_t)A.cs] = srgb2lin(rr[c]);
    }
  }
}

// gigs_spec_tap_census: which texels of the fine specular levels this view's shade reads.  One lane per pixel, 64 x 4
// tiles like shade_fwd_post_kernel; a pixel forms its shading normal (kPost: from normal_map, with that kernel's staging,
// medians and rotation; otherwise read from `normals`), its roughness and view direction as shade_pixel_n does, takes
// spec_taps and stores a 1 into channel 0 of every tap of a level that has a `needed` array ([6 res^2 3] floats, zero
// before the call, the level gradient's shape: specular_census_kernel lists it).  Every tap cube_sample would read is
// marked, whatever its weight.  Plain stores of one value: idempotent, no atomics.
// EVERY pixel marks, inside the normal mask or not: the shade kernels sample the levels for every pixel (a pixel outside
// the mask has its colour selected away afterwards, and specular_rgb and the gradients of gigs_shade_*_ex are defined
// there), so nothing the shade reads is left out of the list.  Only the entry point's optional `mask` (!kPost) skips
// pixels, for a caller that will not shade them.
struct TapCensusArgs {
  int H, W, L;
  int spec_res[8];
  float* needed[8];       // null: the level is not listed
  const float* normals;   // !kPost: element (p, c) at p * ps + c * cs
  int ps, cs;
  const float *normal_map, *vm;  // kPost ([3,H,W] planes, row-major 4x4)
  const uint8_t* mask;    // !kPost; null = every pixel (what the shade kernels sample)
  const float *view_dirs, *roughness;
  float rough_scale, rough_bias;
};

template <bool kPost>
__global__ void __launch_bounds__(256)
spec_tap_census_kernel(TapCensusArgs T) {
  __shared__ PostTile s_n;
  const int H = T.H, W = T.W;
  if (kPost) {
    post_stage(s_n, T.normal_map, H, W);
    __syncthreads();
  }
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const int x = blockIdx.x * kPostW + lx, y = blockIdx.y * kPostH + ly;
  if (x >= W || y >= H) return;
  const int p = y * W + x;
  v3 n;
  if (kPost) {
    float med[3];
    post_median(s_n, lx, ly, med);
    n = post_rotate(T.vm, med);
  } else {
    if (T.mask && T.mask[p] == 0) return;
    const size_t e = (size_t)p * T.ps, cs = T.cs;
    n = {T.normals[e], T.normals[e + cs], T.normals[e + 2 * cs]};
  }
  const v3 v = {T.view_dirs[3 * p], T.view_dirs[3 * p + 1], T.view_dirs[3 * p + 2]};
  const float r = T.roughness[p] * T.rough_scale + T.rough_bias;
  SpecTaps q;
  spec_taps(T.L, T.spec_res, r, n, v, q);
  float* const m0 = T.needed[q.l0];
  if (q.has0 && m0) {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (q.t0.idx[k] >= 0) m0[3 * (size_t)q.t0.idx[k]] = 1.0f;
  }
  float* const m1 = T.needed[q.l1];
  if (q.l1 != q.l0 && q.has1 && m1) {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (q.t1.idx[k] >= 0) m1[3 * (size_t)q.t1.idx[k]] = 1.0f;
  }
}

constexpr int kShadeBwdBlock = 1024;     // 16 waves share one set of LDS accumulators
constexpr int kShadeLdsBudget = 30 * 1024;  // floats (120 KB of the CU's 160 KB)

// Scatter-add of the specular entries that go to GLOBAL levels (8 per lane: 4 taps of l0, 4 of l1), one add per
// distinct (level, texel) of the whole wave.  key = (level << 24) | texel, or -1; v = the entry's three products as
// the caller formed them.  A round takes the first pending key of the first lane that has one, every lane sums its
// own entries with that key (in tap order), wave_sum63 sums the lanes, and lanes 0-2 add the three channels with ONE
// atomic instruction (a contiguous 12-byte request; non-zero sums only): the same products are added, in another
// order.  A wave whose 8x8 pixels see more than kWaveDedupRounds distinct texels (noisy normals) hands the rest to
// run_add3, so the cost per wave stays bounded and the result does not depend on how many keys there are.
// Must be called by all 64 lanes.
constexpr int kWaveDedupRounds = 24;
__device__ __forceinline__ void wave_dedup_add(float* const (&d_spec)[8], int (&key)[8], const float (&v)[8][3]) {
  const int lane = threadIdx.x & 63;
  for (int round = 0; round < kWaveDedupRounds; round++) {
    int first = -1;
#pragma unroll
    for (int k = 7; k >= 0; k--) first = key[k] >= 0 ? key[k] : first;
    const unsigned long long pend = __builtin_amdgcn_ballot_w64(first >= 0);
    if (pend == 0ull) return;
    const int K = __builtin_amdgcn_readlane(first, (int)__builtin_ctzll(pend));  // wave-uniform
    float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; k++) {
      const bool m = key[k] == K;
      s0 += m ? v[k][0] : 0.0f;
      s1 += m ? v[k][1] : 0.0f;
      s2 += m ? v[k][2] : 0.0f;
      key[k] = m ? -1 : key[k];
    }
    s0 = wave_sum63(s0); s1 = wave_sum63(s1); s2 = wave_sum63(s2);  // in lane 63
    const float c0 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s0), 63));
    const float c1 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s1), 63));
    const float c2 = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(s2), 63));
    const float s = lane == 0 ? c0 : (lane == 1 ? c1 : c2);
    if (lane < 3 && s != 0.0f) atomicAdd(d_spec[K >> 24] + 3 * (size_t)(K & 0xffffff) + lane, s);
  }
#pragma unroll
  for (int k = 0; k < 8; k++) {
    if (__builtin_amdgcn_ballot_w64(key[k] >= 0) == 0ull) continue;  // wave-uniform
    float* t = key[k] >= 0 ? d_spec[key[k] >> 24] + 3 * (size_t)(key[k] & 0xffffff) : nullptr;
    run_add3<false>(t, key[k], v[k][0], v[k][1], v[k][2]);
  }
}

// Gradients of the light textures: hundreds of thousands of pixels add into a few thousand texels of
// the coarse levels (16^2 diffuse, 16^2 / 32^2 specular), which serialises memory-side float atomics on
// the same addresses (measured: 0.72 of 0.77 ms).  Every level that fits is therefore accumulated per
// 1024-lane workgroup in LDS (up to 120 KB) and flushed once, non-zero entries only; larger levels take
// global atomics.  Neighbouring lanes hitting the same LDS texel are pre-summed (run_add3).
// kTiles (default): a chunk is a 32 x 32 pixel tile and each wave an 8 x 8 block of it, so that the reflected
// directions of a wave lie as close together as the surface allows, and the global levels get one add per distinct
// texel of the wave (wave_dedup_add).  !kTiles (gigs_options.shade_bwd_rows): row-major 1024-pixel chunks, run_add3
// for every level.  Every per-pixel output is the same in both; the light gradients differ by summation order only.
template <bool kTiles>
__global__ void __launch_bounds__(kShadeBwdBlock)
shade_bwd_kernel(ShadeArgs A) {
  extern __shared__ __align__(16) float s_lds[];
  for (int i = threadIdx.x; i < A.lds_total; i += kShadeBwdBlock) s_lds[i] = 0.0f;
  __syncthreads();
  // persistent workgroups: each keeps its LDS accumulators across several 1024-pixel chunks, so the zero-fill
  // and the flush (and the flush's global atomics) are paid once per workgroup, not once per chunk
  const int tiles_x = (A.W + 31) / 32;
  const int n_chunks = kTiles ? tiles_x * ((A.H + 31) / 32) : (A.H * A.W + kShadeBwdBlock - 1) / kShadeBwdBlock;
  for (int chunk = blockIdx.x; chunk < n_chunks; chunk += gridDim.x) {
  int pg;
  bool live;
  if (kTiles) {
    const int wv = threadIdx.x >> 6, ln = threadIdx.x & 63;
    const int x = (chunk % tiles_x) * 32 + (wv & 3) * 8 + (ln & 7);
    const int y = (chunk / tiles_x) * 32 + (wv >> 2) * 8 + (ln >> 3);
    live = x < A.W && y < A.H;
    pg = y * A.W + x;
  } else {
    pg = chunk * kShadeBwdBlock + threadIdx.x;
    live = pg < A.H * A.W;
  }
  const int p = live ? pg : 0;  // dead lanes shade pixel 0 and add nothing: the DPP scans need every lane
  ShadePix q;
  shade_pixel(A, p, q);
  float g_dl[3] = {0, 0, 0}, g_sp[3] = {0, 0, 0};
  if (live) {
    const bool mk = A.mask[p] != 0;
    const size_t e = (size_t)p * A.ps, cs = A.cs;
    const float gscale = A.g_scale ? A.g_scale[0] : 1.0f;  // x * 1.0f is exact: the plain operator is unchanged
    float g_d[3] = {0, 0, 0}, g_s[3] = {0, 0, 0};  // grads w.r.t. linear diffuse_rgb / specular_rgb
    const float pre_d[3] = {q.drgb.x, q.drgb.y, q.drgb.z}, pre_s[3] = {q.srgb.x, q.srgb.y, q.srgb.z};
#pragma unroll
    for (int c = 0; c < 3; c++) {
      // render = where(mask, gamma(clamp(tone(d + s))), bg)
      float g = (A.g_render && mk) ? A.g_render[e + c * cs] * gscale : 0.0f;
      if (g != 0.0f) {
        float x = pre_d[c] + pre_s[c], d_tone = 1.0f, d_gam = 1.0f;
        if (A.tone) x = aces(x, d_tone);
        const float xc = fminf(fmaxf(x, 0.0f), 1.0f);
        const float d_clamp = (x >= 0.0f && x <= 1.0f) ? 1.0f : 0.0f;
        if (A.gamma) lin2srgb(xc, d_gam);
        g = g * d_gam * d_clamp * d_tone;
      }
      float gd = A.g_diffuse_rgb ? A.g_diffuse_rgb[e + c * cs] : 0.0f;
      float gs = A.g_specular_rgb ? A.g_specular_rgb[e + c * cs] : 0.0f;
      if (A.gamma) {
        float d1, d2;
        lin2srgb(pre_d[c], d1);
        lin2srgb(pre_s[c], d2);
        gd *= d1;
        gs *= d2;
      }
      g_d[c] = g + gd;
      g_s[c] = g + gs;
    }
    const float av[3] = {q.a.x, q.a.y, q.a.z}, dlv[3] = {q.dl.x, q.dl.y, q.dl.z};
    const float spv[3] = {q.sp.x, q.sp.y, q.sp.z}, F0v[3] = {q.F0.x, q.F0.y, q.F0.z};
    const float reflv[3] = {q.refl.x, q.refl.y, q.refl.z};
    const float s0v[3] = {q.s0.x, q.s0.y, q.s0.z}, s1v[3] = {q.s1.x, q.s1.y, q.s1.z};
    float d_alb[3], d_m = 0.0f, d_fgx = 0.0f, d_fgy = 0.0f, d_lvl = 0.0f;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      d_alb[c] = g_d[c] * dlv[c];
      g_dl[c] = g_d[c] * av[c] + (A.g_diffuse_light ? A.g_diffuse_light[e + c * cs] : 0.0f);
      g_sp[c] = g_s[c] * reflv[c];
      const float g_refl = g_s[c] * spv[c];
      const float dF0 = g_refl * q.fgx;
      d_fgx += g_refl * F0v[c];
      d_fgy += g_refl;
      if (A.metallic) {
        d_m += dF0 * (av[c] - 0.04f);
        d_alb[c] += dF0 * q.m;
      }
      if (q.l1 != q.l0) d_lvl += g_sp[c] * (s1v[c] - s0v[c]);
    }
#pragma unroll
    for (int c = 0; c < 3; c++) {
      if (A.g_albedo_mul_a) d_alb[c] += (A.g_albedo_mul_a[e + c * cs] * gscale) * A.g_albedo_mul_b[e + c * cs];
      A.d_albedo[e + c * cs] = d_alb[c];
    }
    float add_r = A.g_roughness_add ? A.g_roughness_add[p] : 0.0f, add_m = A.g_metallic_add ? A.g_metallic_add[p] : 0.0f;
    if (A.lamb_mask) {  // stage2_loss_bwd_kernel's two lines
      const float m = A.lamb_mask[p], cnt = A.lamb_acc4[3];
      add_r += -m / cnt * (0.001f * gscale);
      add_m += m / cnt * (0.001f * gscale);
    }
    if (A.d_metallic) A.d_metallic[p] = d_m + add_m;
    const float d_r = d_fgx * q.dfgx_dv + d_fgy * q.dfgy_dv + (q.lvl_inside ? d_lvl * q.dmdr : 0.0f);
    A.d_roughness[p] = (d_r + add_r) * A.rough_scale;
  }
  // ---- light textures (wave-uniform control flow from here on) ----
#ifdef GIGS_DIAG
#define GIGS_ABLATED(bit) (A.ablate & (bit))
#else
#define GIGS_ABLATED(bit) 0  // the shipped kernel has no result-changing switch
#endif
  if (A.d_diffuse && !GIGS_ABLATED(1)) {
    float* base = A.lds_diffuse_off >= 0 ? s_lds + A.lds_diffuse_off : A.d_diffuse;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int idx = (live && q.has_d) ? q.td.idx[k] : -1;
      const float w = idx >= 0 ? q.td.w[k] * q.occ : 0.0f;
      run_add3<false>(base + 3 * (size_t)max(idx, 0), idx, g_dl[0] * w, g_dl[1] * w, g_dl[2] * w);
    }
  }
  if (!GIGS_ABLATED(2)) {
    const float wl = (q.l1 != q.l0) ? (1 - q.lf) : 1.0f;
    float* t0 = A.lds_spec_off[q.l0] >= 0 ? s_lds + A.lds_spec_off[q.l0] : A.d_spec[q.l0];
    float* t1 = A.lds_spec_off[q.l1] >= 0 ? s_lds + A.lds_spec_off[q.l1] : A.d_spec[q.l1];
    if (!A.d_spec[q.l0]) t0 = nullptr;
    if (!A.d_spec[q.l1]) t1 = nullptr;
    // diagnostic (GIGS_ABLATE bit 2 / 3): drop the adds that go to LDS-resident / to global levels
#ifdef GIGS_DIAG
    if (((A.ablate & 4) && A.lds_spec_off[q.l0] >= 0) || ((A.ablate & 8) && A.lds_spec_off[q.l0] < 0)) t0 = nullptr;
    if (((A.ablate & 4) && A.lds_spec_off[q.l1] >= 0) || ((A.ablate & 8) && A.lds_spec_off[q.l1] < 0)) t1 = nullptr;
#endif
    if (kTiles) {
      // entries of LDS-resident levels: run_add3 as below; entries of global levels are collected (an entry whose
      // three products are 0 adds nothing in either formulation) and added once per distinct texel of the wave
      const bool glob0 = A.lds_spec_off[q.l0] < 0, glob1 = A.lds_spec_off[q.l1] < 0;
      int gkey[8];
      float gv[8][3];
#pragma unroll
      for (int k = 0; k < 8; k++) {
        const bool first = k < 4;
        const int idx = first ? ((live && q.has0 && t0) ? q.t0.idx[k] : -1)
                              : ((live && q.l1 != q.l0 && q.has1 && t1) ? q.t1.idx[k - 4] : -1);
        const float w = idx >= 0 ? (first ? q.t0.w[k] * wl : q.t1.w[k - 4] * q.lf) : 0.0f;
        const float v0 = g_sp[0] * w, v1 = g_sp[1] * w, v2 = g_sp[2] * w;
        const int key = idx >= 0 ? ((first ? q.l0 : q.l1) << 24) | idx : -1;
        const bool glob = first ? glob0 : glob1;
        gkey[k] = (glob && (v0 != 0.0f || v1 != 0.0f || v2 != 0.0f)) ? key : -1;
        gv[k][0] = v0; gv[k][1] = v1; gv[k][2] = v2;
        const int lkey = glob ? -1 : key;
        if (__builtin_amdgcn_ballot_w64(lkey >= 0) != 0ull)  // wave-uniform
          run_add3<false>(lkey >= 0 ? (first ? t0 : t1) + 3 * (size_t)idx : nullptr, lkey, v0, v1, v2);
      }
      wave_dedup_add(A.d_spec, gkey, gv);
    } else {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int idx = (live && q.has0 && t0) ? q.t0.idx[k] : -1;
      const float w = idx >= 0 ? q.t0.w[k] * wl : 0.0f;
      run_add3<false>(t0 ? t0 + 3 * (size_t)max(idx, 0) : nullptr, idx >= 0 ? (q.l0 << 24) | idx : -1, g_sp[0] * w, g_sp[1] * w, g_sp[2] * w);
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int idx = (live && q.l1 != q.l0 && q.has1 && t1) ? q.t1.idx[k] : -1;
      const float w = idx >= 0 ? q.t1.w[k] * q.lf : 0.0f;
      run_add3<false>(t1 ? t1 + 3 * (size_t)max(idx, 0) : nullptr, idx >= 0 ? (q.l1 << 24) | idx : -1, g_sp[0] * w, g_sp[1] * w, g_sp[2] * w);
    }
    }
  }
  }  // chunk loop
  if (A.lds_total > 0) {
    __syncthreads();
    if (A.lds_diffuse_off >= 0 && A.d_diffuse) {
      const int n = 6 * A.diffuse_res * A.diffuse_res * 3;
      for (int i = threadIdx.x; i < n; i += kShadeBwdBlock) {
        const float val = s_lds[A.lds_diffuse_off + i];
        if (val != 0.0f) atomicAdd(A.d_diffuse + i, val);
      }
    }
    for (int l = 0; l < A.L; l++) {
      if (A.lds_spec_off[l] < 0 || !A.d_spec[l]) continue;
      const int n = 6 * A.spec_res[l] * A.spec_res[l] * 3;
      for (int i = threadIdx.x; i < n; i += kShadeBwdBlock) {
        const float val = s_lds[A.lds_spec_off[l] + i];
        if (val != 0.0f) atomicAdd(A.d_spec[l] + i, val);
      }
    }
  }
}

}  // namespace gigs

// ------------------------------------------------------------------------------------------
// C ABI (declared in include/gigs_hip.h)
// ------------------------------------------------------------------------------------------
#include "gigs_internal.h"

extern "C" {

static int fill_shade(gigs::ShadeArgs& A, int H, int W, const float* normals, const float* view_dirs,
                      const float* albedo, const float* roughness, const uint8_t* mask,
                      const float* occlusion, const float* metallic, const float* background,
                      const float* diffuse, int diffuse_res, int n_levels, const float* const* spec,
                      const int* spec_res, const float* lut, int lut_w, int lut_h, int tone, int gamma) {
  if (H <= 0 || W <= 0 || !normals || !view_dirs || !albedo || !roughness || !mask || !diffuse || !spec || !spec_res || !lut)
    return gigs_internal_fail(GIGS_ERR_INVALID, "shade: null required input");
  if (n_levels < 2 || n_levels > 8 || diffuse_res <= 0 || lut_w <= 0 || lut_h <= 0)
    return gigs_internal_fail(GIGS_ERR_INVALID, "shade: needs 2..8 specular levels and positive texture sizes");
  memset(&A, 0, sizeof(A));
  A.H = H; A.W = W; A.normals = normals; A.view_dirs = view_dirs; A.albedo = albedo; A.roughness = roughness;
  A.mask = mask; A.occlusion = occlusion; A.metallic = metallic; A.background = background;
  A.diffuse = diffuse; A.diffuse_res = diffuse_res; A.L = n_levels;
  for (int i = 0; i < n_levels; i++) {
    if (!spec[i] || spec_res[i] <= 0) return gigs_internal_fail(GIGS_ERR_INVALID, "shade: bad specular level");
    A.spec[i] = spec[i];
    A.spec_res[i] = spec_res[i];
  }
  A.lut = lut; A.lut_w = lut_w; A.lut_h = lut_h; A.tone = tone; A.gamma = gamma;
#ifdef GIGS_DIAG
  const char* ab = getenv("GIGS_ABLATE");
  A.ablate = ab ? atoi(ab) : 0;
#endif
  A.ps = 3; A.cs = 1; A.rough_scale = 1.0f; A.rough_bias = 0.0f;
  return 0;
}

static int apply_shade_ext(gigs::ShadeArgs& A, const gigs_shade_ext* ext, bool backward) {
  if (!ext) return 0;
  if (ext->planar) { A.ps = 1; A.cs = A.H * A.W; }
  A.rough_scale = ext->rough_scale; A.rough_bias = ext->rough_bias;
  if (!backward) {
    A.out_F0 = ext->out_F0; A.out_linear = ext->out_linear; A.out_roughness = ext->out_roughness;
  } else {
    if ((ext->g_albedo_mul_a == nullptr) != (ext->g_albedo_mul_b == nullptr))
      return gigs_internal_fail(GIGS_ERR_INVALID, "shade_bwd: g_albedo_mul_a/b must be given together");
    A.g_albedo_mul_a = ext->g_albedo_mul_a; A.g_albedo_mul_b = ext->g_albedo_mul_b;
    A.g_roughness_add = ext->g_roughness_add; A.g_metallic_add = ext->g_metallic_add;
    if ((ext->lamb_mask == nullptr) != (ext->lamb_acc4 == nullptr))
      return gigs_internal_fail(GIGS_ERR_INVALID, "shade_bwd: lamb_mask / lamb_acc4 must be given together");
    A.g_scale = ext->g_scale; A.lamb_mask = ext->lamb_mask; A.lamb_acc4 = ext->lamb_acc4;
  }
  return 0;
}

int gigs_shade_fwd(int H, int W, const float* normals, const float* view_dirs, const float* albedo,
                   const float* roughness, const uint8_t* mask, const float* occlusion,
                   const float* metallic, const float* background, const float* diffuse, int diffuse_res,
                   int n_levels, const float* const* spec, const int* spec_res, const float* lut,
                   int lut_w, int lut_h, int tone, int gamma, float* render_rgb, float* diffuse_rgb,
                   float* specular_rgb, float* diffuse_light, void* stream) {
  return gigs_shade_fwd_ex(nullptr, H, W, normals, view_dirs, albedo, roughness, mask, occlusion, metallic, background, diffuse,
                           diffuse_res, n_levels, spec, spec_res, lut, lut_w, lut_h, tone, gamma, render_rgb,
                           diffuse_rgb, specular_rgb, diffuse_light, nullptr, stream);
}

int gigs_shade_fwd_ex(gigs_ctx* ctx, int H, int W, const float* normals, const float* view_dirs, const float* albedo,
                      const float* roughness, const uint8_t* mask, const float* occlusion,
                      const float* metallic, const float* background, const float* diffuse, int diffuse_res,
                      int n_levels, const float* const* spec, const int* spec_res, const float* lut,
                      int lut_w, int lut_h, int tone, int gamma, float* render_rgb, float* diffuse_rgb,
                      float* specular_rgb, float* diffuse_light, const gigs_shade_ext* ext, void* stream) {
  (void)ctx;  // the forward reads no option; the parameter keeps the two _ex entries alike
  gigs::ShadeArgs A;
  const int rc = fill_shade(A, H, W, normals, view_dirs, albedo, roughness, mask, occlusion, metallic, background,
                            diffuse, diffuse_res, n_levels, spec, spec_res, lut, lut_w, lut_h, tone, gamma);
  if (rc) return rc;
  if (!render_rgb || (!ext && (!diffuse_rgb || !specular_rgb || !diffuse_light)))
    return gigs_internal_fail(GIGS_ERR_INVALID, "shade_fwd: null output");
  if (apply_shade_ext(A, ext, false)) return GIGS_ERR_INVALID;
  A.render_rgb = render_rgb; A.diffuse_rgb = diffuse_rgb; A.specular_rgb = specular_rgb; A.diffuse_light = diffuse_light;
  gigs::StageTimer timer(gigs::Stage::kShadeFwd, stream);
  hipLaunchKernelGGL(gigs::shade_fwd_kernel, dim3((H * W + 255) / 256), dim3(256), 0, (hipStream_t)stream, A);
  return gigs_internal_check_launch("shade_fwd");
}

int gigs_shade_fwd_post(gigs_ctx* ctx, int H, int W, const float* normal_map, const float* out_normal_view,
                        const float* viewmatrix, float* normals_view, uint8_t* normal_mask, float* normal_mask_f,
                        float* out_normal_view_filtered, const float* view_dirs, const float* albedo,
                        const float* roughness, const float* occlusion, const float* metallic, const float* diffuse,
                        int diffuse_res, int n_levels, const float* const* spec, const int* spec_res, const float* lut,
                        int lut_w, int lut_h, int tone, int gamma, float* render_rgb, const gigs_shade_ext* ext,
                        void* stream) {
  (void)ctx;
  if (!normal_map || !out_normal_view || !viewmatrix || !normals_view || !normal_mask || !out_normal_view_filtered)
    return gigs_internal_fail(GIGS_ERR_INVALID, "shade_fwd_post: bad argument");
  if (!ext || !ext->planar) return gigs_internal_fail(GIGS_ERR_INVALID, "shade_fwd_post: needs the planar layout (ext->planar)");
  gigs::ShadeArgs A;
  const int rc = fill_shade(A, H, W, normals_view, view_dirs, albedo, roughness, normal_mask, occlusion, metallic, nullptr,
                            diffuse, diffuse_res, n_levels, spec, spec_res, lut, lut_w, lut_h, tone, gamma);
  if (rc) return rc;
  if (!render_rgb) return gigs_internal_fail(GIGS_ERR_INVALID, "shade_fwd_post: null output");
  if (apply_shade_ext(A, ext, false)) return GIGS_ERR_INVALID;
  A.render_rgb = render_rgb;
  const gigs::ShadePostArgs P{normal_map, out_normal_view, viewmatrix, normals_view, normal_mask, normal_mask_f,
                              out_normal_view_filtered};
  gigs::StageTimer timer(gigs::Stage::kShadeFwd, stream);
  hipLaunchKernelGGL(gigs::shade_fwd_post_kernel, dim3((W + gigs::kPostW - 1) / gigs::kPostW, (H + gigs::kPostH - 1) / gigs::kPostH),
                     dim3(256), 0, (hipStream_t)stream, A, P);
  return gigs_internal_check_launch("shade_fwd_post");
}

int gigs_shade_fwd_multi(gigs_ctx* ctx, int n_lights, int H, int W, const float* normals, const float* view_dirs,
                         const float* albedo, const float* roughness, const uint8_t* mask, const float* occlusion,
                         const float* metallic, const float* const* diffuse, int diffuse_res, int n_levels,
                         const float* const* spec, const int* spec_res, const float* lut, int lut_w, int lut_h, int tone,
                         int gamma, float* render_rgb, float* out_linear, void* stream) {
  (void)ctx;
  if (n_lights < 1 || n_lights > GIGS_MAX_LIGHTS || !diffuse || !spec)
    return gigs_internal_fail(GIGS_ERR_INVALID, "shade_fwd_multi: n_lights outside 1..GIGS_MAX_LIGHTS or no diffuse / spec arrays");
  static_assert(gigs::kShadeMaxLights == GIGS_MAX_LIGHTS, "one light limit");
  gigs::ShadeArgs A;
  const int rc = fill_shade(A, H, W, normals, view_dirs, albedo, roughness, mask, occlusion, metallic, nullptr, diffuse[0],
                            diffuse_res, n_levels, spec, spec_res, lut, lut_w, lut_h, tone, gamma);
  if (rc) return rc;
  if (!render_rgb) return gigs_internal_fail(GIGS_ERR_INVALID, "shade_fwd_multi: null output");
  gigs::ShadeLights Ls;
  memset(&Ls, 0, sizeof(Ls));
  Ls.K = n_lights;
  for (int k = 0; k < n_lights; k++) {
    if (!diffuse[k]) return gigs_internal_fail(GIGS_ERR_INVALID, "shade_fwd_multi: null diffuse map");
    Ls.diffuse[k] = diffuse[k];
    for (int l = 0; l < n_levels; l++) {
      if (!spec[k * n_levels + l]) return gigs_internal_fail(GIGS_ERR_INVALID, "shade_fwd_multi: null specular level");
      Ls.spec[k][l] = spec[k * n_levels + l];
    }
  }
  A.ps = 1; A.cs = H * W;  // planar, rough_scale 1, rough_bias 0 (fill_shade)
  A.render_rgb = render_rgb; A.out_linear = out_linear;
  gigs::StageTimer timer(gigs::Stage::kShadeFwd, stream);
  hipLaunchKernelGGL(gigs::shade_fwd_multi_kernel, dim3((H * W + 255) / 256), dim3(256), 0, (hipStream_t)stream, A, Ls);
  return gigs_internal_check_launch("shade_fwd_multi");
}

int gigs_spec_tap_census(gigs_ctx* ctx, int H, int W, const float* normals, int planar, const float* normal_map,
                         const float* viewmatrix, const float* view_dirs, const float* roughness, const uint8_t* mask,
                         float rough_scale, float rough_bias, int n_levels, const int* spec_res, float* const* needed,
                         void* stream) {
  (void)ctx;
  if (H <= 0 || W <= 0 || !view_dirs || !roughness || !spec_res || !needed || n_levels < 2 || n_levels > 8)
    return gigs_internal_fail(GIGS_ERR_INVALID, "spec_tap_census: bad argument");
  if ((normals == nullptr) == (normal_map == nullptr) || (normal_map && !viewmatrix))
    return gigs_internal_fail(GIGS_ERR_INVALID, "spec_tap_census: give either normals or normal_map with viewmatrix");
  gigs::TapCensusArgs T;
  memset(&T, 0, sizeof(T));
  T.H = H; T.W = W; T.L = n_levels;
  for (int i = 0; i < n_levels; i++) {
    if (spec_res[i] <= 0 || spec_res[i] > 4096) return gigs_internal_fail(GIGS_ERR_INVALID, "spec_tap_census: bad level");
    T.spec_res[i] = spec_res[i];
    T.needed[i] = needed[i];
  }
  T.normals = normals; T.ps = planar ? 1 : 3; T.cs = planar ? H * W : 1;
  T.normal_map = normal_map; T.vm = viewmatrix; T.mask = mask;
  T.view_dirs = view_dirs; T.roughness = roughness; T.rough_scale = rough_scale; T.rough_bias = rough_bias;
  // no StageTimer: the call is made for a second stream beside the SSAO march, where a pair of events times the march's
  // shadow (23 us there, 17 us alone), not this kernel
  const dim3 grid((W + gigs::kPostW - 1) / gigs::kPostW, (H + gigs::kPostH - 1) / gigs::kPostH);
  if (normal_map) hipLaunchKernelGGL(gigs::spec_tap_census_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, T);
  else hipLaunchKernelGGL(gigs::spec_tap_census_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, T);
  return gigs_internal_check_launch("spec_tap_census");
}

int gigs_shade_bwd(int H, int W, const float* normals, const float* view_dirs, const float* albedo,
                   const float* roughness, const uint8_t* mask, const float* occlusion,
                   const float* metallic, const float* diffuse, int diffuse_res, int n_levels,
                   const float* const* spec, const int* spec_res, const float* lut, int lut_w, int lut_h,
                   int tone, int gamma, const float* g_render, const float* g_diffuse_rgb,
                   const float* g_specular_rgb, const float* g_diffuse_light, float* d_albedo,
                   float* d_roughness, float* d_metallic, float* d_diffuse, float* const* d_spec,
                   void* stream) {
  return gigs_shade_bwd_ex(nullptr, H, W, normals, view_dirs, albedo, roughness, mask, occlusion, metallic, diffuse, diffuse_res,
                           n_levels, spec, spec_res, lut, lut_w, lut_h, tone, gamma, g_render, g_diffuse_rgb,
                           g_specular_rgb, g_diffuse_light, d_albedo, d_roughness, d_metallic, d_diffuse, d_spec, nullptr,
                           stream);
}

int gigs_shade_bwd_ex(gigs_ctx* ctx, int H, int W, const float* normals, const float* view_dirs, const float* albedo,
                      const float* roughness, const uint8_t* mask, const float* occlusion,
                      const float* metallic, const float* diffuse, int diffuse_res, int n_levels,
                      const float* const* spec, const int* spec_res, const float* lut, int lut_w, int lut_h,
                      int tone, int gamma, const float* g_render, const float* g_diffuse_rgb,
                      const float* g_specular_rgb, const float* g_diffuse_light, float* d_albedo,
                      float* d_roughness, float* d_metallic, float* d_diffuse, float* const* d_spec,
                      const gigs_shade_ext* ext, void* stream) {
  gigs::ShadeArgs A;
  const int rc = fill_shade(A, H, W, normals, view_dirs, albedo, roughness, mask, occlusion, metallic, nullptr,
                            diffuse, diffuse_res, n_levels, spec, spec_res, lut, lut_w, lut_h, tone, gamma);
  if (rc) return rc;
  if (apply_shade_ext(A, ext, true)) return GIGS_ERR_INVALID;
  if (!d_albedo || !d_roughness) return gigs_internal_fail(GIGS_ERR_INVALID, "shade_bwd: null output");
  A.g_render = g_render; A.g_diffuse_rgb = g_diffuse_rgb; A.g_specular_rgb = g_specular_rgb; A.g_diffuse_light = g_diffuse_light;
  A.d_albedo = d_albedo; A.d_roughness = d_roughness; A.d_metallic = d_metallic; A.d_diffuse = d_diffuse;
  for (int i = 0; i < n_levels; i++) A.d_spec[i] = d_spec ? d_spec[i] : nullptr;
  // LDS plan: the diffuse map first, then specular levels from the coarsest up while they fit
  int used = 0;
  A.lds_diffuse_off = -1;
  for (int i = 0; i < 8; i++) A.lds_spec_off[i] = -1;
  const int n_dd = 6 * diffuse_res * diffuse_res * 3;
  const gigs::Options& o = *gigs_internal_options(ctx);
  // gigs_options.shade_lds_floats: tuning knob (smaller budget -> more workgroups per CU)
  const int lds_budget = o.shade_lds_floats < 0 ? 0 : (o.shade_lds_floats > gigs::kShadeLdsBudget ? gigs::kShadeLdsBudget : o.shade_lds_floats);
  if (d_diffuse && n_dd <= lds_budget) { A.lds_diffuse_off = 0; used = n_dd; }
  for (int i = n_levels - 1; i >= 0; i--) {
    const int n = 6 * spec_res[i] * spec_res[i] * 3;
    if (A.d_spec[i] && used + n <= lds_budget) { A.lds_spec_off[i] = used; used += n; }
  }
  A.lds_total = used;
  // gigs_options.shade_bwd_rows: the previous pixel mapping and scatter (same per-pixel bits; the checker of the default)
  const bool rows = o.shade_bwd_rows != 0;
  const void* fn = rows ? reinterpret_cast<const void*>(gigs::shade_bwd_kernel<false>)
                        : reinterpret_cast<const void*>(gigs::shade_bwd_kernel<true>);
  static bool attr_set[2] = {false, false};
  if (!attr_set[rows]) {
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, gigs::kShadeLdsBudget * (int)sizeof(float)) != hipSuccess)
      return gigs_internal_fail(GIGS_ERR_HIP, "shade_bwd: cannot raise the dynamic LDS limit");
    attr_set[rows] = true;
  }
  gigs::StageTimer timer(gigs::Stage::kShadeBwd, stream);
  const int n_chunks = rows ? (H * W + gigs::kShadeBwdBlock - 1) / gigs::kShadeBwdBlock : ((W + 31) / 32) * ((H + 31) / 32);
  static const int n_cus = [] {  // one workgroup per CU (120 KB of LDS each); gigs_options.shade_bwd_blocks overrides
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) == hipSuccess) hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    return cus;
  }();
  const int max_blocks = o.shade_bwd_blocks > 0 ? o.shade_bwd_blocks : n_cus;
  const int blocks = (n_chunks < max_blocks) ? n_chunks : max_blocks;
  if (rows)
    hipLaunchKernelGGL(gigs::shade_bwd_kernel<false>, dim3(blocks), dim3(gigs::kShadeBwdBlock), (size_t)used * sizeof(float),
                       (hipStream_t)stream, A);
  else
    hipLaunchKernelGGL(gigs::shade_bwd_kernel<true>, dim3(blocks), dim3(gigs::kShadeBwdBlock), (size_t)used * sizeof(float),
                       (hipStream_t)stream, A);
  return gigs_internal_check_launch("shade_bwd");
}

}  // extern "C"
