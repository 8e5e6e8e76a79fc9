// cube.h -- cube-map geometry, bilinear cube taps and the DPP lane moves shared by the light filters
// (light_filter.hip), the cube / panorama textures (cube_texture.hip) and the deferred shade (shade.hip).
// Device-inline code and plain structs only: no kernel, no state.
//
// The three texture lookups of the shade are nvdiffrast `dr.texture` calls in the reference (third party,
// unpinned -> parity unpinned); the sampling rule implemented by cube_face_uv / cube_taps is written down in
// include/gigs_hip.h and oracle/pbr_oracle.cpp.  "RU/" is pbr/renderutils/c_src/.
#pragma once

#include "gigs_common.h"
#include "pixel_ops.h"

namespace gigs {

// ------------------------------------------------------------------------------------------
// texel <-> direction
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ v3 safe_normalize(v3 v) {  // RU/vec3f.h:90-94
  const float l = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
  return l > 0.0f ? v3{v.x / l, v.y / l, v.z / l} : v3{0, 0, 0};
}
__device__ __forceinline__ v3 cube_dir_raw(float fx, float fy, int side) {
  switch (side) {
    case 0: return {1, -fy, -fx};
    case 1: return {-1, -fy, fx};
    case 2: return {fx, 1, fy};
    case 3: return {fx, -1, -fy};
    case 4: return {fx, -fy, 1};
    default: return {-fx, -fy, -1};
  }
}
__device__ __forceinline__ v3 cube_to_dir(int x, int y, int side, int N) {  // RU/cubemap.cu:33-47
  const float fx = 2.0f * (((float)x + 0.5f) / (float)N) - 1.0f;
  const float fy = 2.0f * (((float)y + 0.5f) / (float)N) - 1.0f;
  return safe_normalize(cube_dir_raw(fx, fy, side));
}

// ------------------------------------------------------------------------------------------
// DPP lane moves
// ------------------------------------------------------------------------------------------
// The value of the lane that kCtrl names; lanes without a source (or outside kRowMask) get 0 / `old`.
template <int kCtrl, int kRowMask = 0xf>
__device__ __forceinline__ float row_f(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), kCtrl, kRowMask, 0xf, false));
}
template <int kCtrl>
__device__ __forceinline__ int row_i(int old, int v) {
  return __builtin_amdgcn_update_dpp(old, v, kCtrl, 0xf, 0xf, false);
}

// Sum over the 64 lanes of a wave (DPP, no LDS); total valid in lane 63.
__device__ __forceinline__ float wave_sum63(float v) {
  v += row_f<0xb1>(v);
  v += row_f<0x4e>(v);
  v += row_f<0x124>(v);
  v += row_f<0x128>(v);
  v += row_f<0x142, 0xa>(v);
  v += row_f<0x143, 0xc>(v);
  return v;
}

// Scatter-add of one RGB triple per lane into a texture gradient, with neighbouring lanes that
// hit the SAME texel summed first: neighbouring pixels usually share bilinear taps, and 64
// same-address float atomics serialise.  Runs of equal keys inside each 16-lane DPP row are
// reduced with a segmented scan (row_shr 1/2/4/8, in registers); only the last lane of a run
// issues the three atomics.  Must be called by all 64 lanes (key < 0 = nothing to add).
template <bool kLds>
__device__ __forceinline__ void run_add3(float* target, int key, float v0, float v1, float v2) {
  const int head = (row_i<0x111>(~key, key) != key) ? 1 : 0;  // row_shr:1; lane 0 of a row is a head
  int f = head;
#define GIGS_SEG_STEP(CTRL)                                            \
  {                                                                    \
    const float u0 = row_f<CTRL>(v0), u1 = row_f<CTRL>(v1), u2 = row_f<CTRL>(v2); \
    const int fu = row_i<CTRL>(1, f);                                  \
    if (!f) { v0 += u0; v1 += u1; v2 += u2; }                          \
    f |= fu;                                                           \
  }
  GIGS_SEG_STEP(0x111) GIGS_SEG_STEP(0x112) GIGS_SEG_STEP(0x114) GIGS_SEG_STEP(0x118)
#undef GIGS_SEG_STEP
  const int tail = row_i<0x101>(1, head);  // row_shl:1 -> head flag of the next lane; 1 at the row end
  if (key >= 0 && tail && target) {
    if (v0 != 0.0f) atomicAdd(target, v0);
    if (v1 != 0.0f) atomicAdd(target + 1, v1);
    if (v2 != 0.0f) atomicAdd(target + 2, v2);
  }
}

// ------------------------------------------------------------------------------------------
// cube texture sampling
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ int cube_face_uv(float x, float y, float z, float& u, float& v) {
  const float ax = fabsf(x), ay = fabsf(y), az = fabsf(z);
  int idx;
  float c;
  if (az > fmaxf(ax, ay)) { idx = 4; c = z; }
  else if (ay > ax) { idx = 2; c = y; y = z; }
  else { idx = 0; c = x; x = z; }
  if (c < 0.f) idx += 1;
  const float m = (1.0f / fabsf(c)) * 0.5f;
  const float m0 = (idx == 0 || idx == 5) ? -m : m;
  const float m1 = (idx != 2) ? -m : m;
  u = x * m0 + 0.5f;
  v = y * m1 + 0.5f;
  if (!isfinite(u) || !isfinite(v)) return -1;
  u = fminf(fmaxf(u, 0.f), 1.f);
  v = fminf(fmaxf(v, 0.f), 1.f);
  return idx;
}

struct Taps { int idx[4]; float w[4]; };

__device__ __forceinline__ bool cube_taps(int res, float dx, float dy, float dz, Taps& t) {
  float u, v;
  const int face = cube_face_uv(dx, dy, dz, u, v);
  if (face < 0) return false;
  const float fu = u * (float)res - 0.5f, fv = v * (float)res - 0.5f;
  const float flu = floorf(fu), flv = floorf(fv);
  const int iu0 = (int)flu, iv0 = (int)flv;
  const float tu = fu - flu, tv = fv - flv;
  float wsum = 0.0f;
  bool dropped = false;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int ox = k & 1, oy = k >> 1;
    const int ix = iu0 + ox, iy = iv0 + oy;
    const float w = (ox ? tu : 1.0f - tu) * (oy ? tv : 1.0f - tv);
    const bool out_x = ix < 0 || ix >= res, out_y = iy < 0 || iy >= res;
    int idx;
    if (!out_x && !out_y) {
      idx = (face * res + iy) * res + ix;
    } else if (out_x && out_y) {
      idx = -1;
      dropped = true;
    } else {
      const float a = 2.0f * (((float)ix + 0.5f) / (float)res) - 1.0f;
      const float b = 2.0f * (((float)iy + 0.5f) / (float)res) - 1.0f;
      const v3 d = cube_dir_raw(a, b, face);
      float u2, v2;
      const int f2 = cube_face_uv(d.x, d.y, d.z, u2, v2);
      const int x2 = min(res - 1, max(0, (int)floorf(u2 * (float)res)));
      const int y2 = min(res - 1, max(0, (int)floorf(v2 * (float)res)));
      idx = (f2 * res + y2) * res + x2;
    }
    t.idx[k] = idx;
    t.w[k] = w;
    if (idx >= 0) wsum += w;
  }
  if (dropped) {
#pragma unroll
    for (int k = 0; k < 4; k++) t.w[k] = t.idx[k] >= 0 ? t.w[k] / wsum : 0.0f;
  }
  return true;
}

// cube_taps with the texel coordinates formed in double (gigs_cube_texture_fwd_precise; resampling a light onto another
// cube grid, relight.rotate_light).  In float the coordinate u * res - 0.5 carries half an ulp of a value up to res -- 1.9e-6
// texels at res 64, 7.6e-6 at 256 -- on top of res times the roundings of u, which a resample of a light writes into every
// texel as noise; in double the weights are exact to float rounding.  Face choice and tap indices are cube_taps' (the
// comparisons of float inputs are exact either way, and a wrapped tap's index comes from the same float path).
__device__ __forceinline__ bool cube_taps_precise(int res, float dx, float dy, float dz, Taps& t) {
  double x = dx, y = dy, z = dz;
  const double ax = fabs(x), ay = fabs(y), az = fabs(z);
  int face;
  double c;
  if (az > fmax(ax, ay)) { face = 4; c = z; }
  else if (ay > ax) { face = 2; c = y; y = z; }
  else { face = 0; c = x; x = z; }
  if (c < 0.0) face += 1;
  const double m = (1.0 / fabs(c)) * 0.5;
  const double m0 = (face == 0 || face == 5) ? -m : m;
  const double m1 = (face != 2) ? -m : m;
  double u = x * m0 + 0.5, v = y * m1 + 0.5;
  if (!isfinite(u) || !isfinite(v)) return false;
  u = fmin(fmax(u, 0.0), 1.0);
  v = fmin(fmax(v, 0.0), 1.0);
  const double fu = u * (double)res - 0.5, fv = v * (double)res - 0.5;
  const double flu = floor(fu), flv = floor(fv);
  const int iu0 = (int)flu, iv0 = (int)flv;
  const double tu = fu - flu, tv = fv - flv;
  double w[4], wsum = 0.0;
  bool dropped = false;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int ox = k & 1, oy = k >> 1;
    const int ix = iu0 + ox, iy = iv0 + oy;
    w[k] = (ox ? tu : 1.0 - tu) * (oy ? tv : 1.0 - tv);
    const bool out_x = ix < 0 || ix >= res, out_y = iy < 0 || iy >= res;
    int idx;
    if (!out_x && !out_y) {
      idx = (face * res + iy) * res + ix;
    } else if (out_x && out_y) {
      idx = -1;
      dropped = true;
    } else {  // the neighbouring face's texel, as cube_taps finds it
      const float a = 2.0f * (((float)ix + 0.5f) / (float)res) - 1.0f;
      const float b = 2.0f * (((float)iy + 0.5f) / (float)res) - 1.0f;
      const v3 d = cube_dir_raw(a, b, face);
      float u2, v2;
      const int f2 = cube_face_uv(d.x, d.y, d.z, u2, v2);
      const int x2 = min(res - 1, max(0, (int)floorf(u2 * (float)res)));
      const int y2 = min(res - 1, max(0, (int)floorf(v2 * (float)res)));
      idx = (f2 * res + y2) * res + x2;
    }
    t.idx[k] = idx;
    if (idx >= 0) wsum += w[k];
  }
#pragma unroll
  for (int k = 0; k < 4; k++) t.w[k] = t.idx[k] < 0 ? 0.0f : (float)(dropped ? w[k] / wsum : w[k]);
  return true;
}

__device__ __forceinline__ v3 cube_sample(const float* __restrict__ tex, const Taps& t) {
  v3 r = {0, 0, 0};
#pragma unroll
  for (int k = 0; k < 4; k++)
    if (t.idx[k] >= 0) {
      const float* p = tex + 3 * (size_t)t.idx[k];
      r.x += p[0] * t.w[k];
      r.y += p[1] * t.w[k];
      r.z += p[2] * t.w[k];
    }
  return r;
}

// torch.linspace(start, end, n)[i]: start + i * step below the middle, end - (n - 1 - i) * step above
__device__ __forceinline__ float torch_linspace(float start, float end, int n, int i) {
  if (n <= 1) return start;
  const float step = (end - start) / (float)(n - 1);
  return (i < n / 2) ? start + step * (float)i : end - step * (float)(n - 1 - i);
}

}  // namespace gigs
