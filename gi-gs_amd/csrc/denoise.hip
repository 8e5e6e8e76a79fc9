// denoise.hip -- an edge-avoiding a-trous wavelet filter for the ray-traced planes (denoise.atrous): a single-frame filter in
// the manner of Dammertz 2010 / SVGF, guided by the prepared points and normals the tracers return.  include/gigs_hip.h,
// "Denoising ray-traced planes", states every quantity and tests/denoise_ref.py restates them in numpy float32.
//
//   arithmetic    float32, + - * / only, built with -ffp-contract=off: every product and sum is rounded on its own in the
//                 stated order.  No exp, pow or sqrt: the edge-stopping functions are compact-support polynomials, so the numpy
//                 restatement agrees bit for bit and a weight across a real edge is exactly 0.  Every max(a, b) is written
//                 (a > b) ? a : b.
//   layout        gigs_denoise_pack turns the planes into pixel-major records once: a guide record of kGuide = 8 floats
//                 (point, normal, roughness, live flag) and a signal record of S = 4 ceil((C + G) / 4) floats (the C values,
//                 then the G variances, then padding).  A tap is then two float4 loads plus S / 4, not 7 + C + G scattered
//                 dwords.
//   scheme        ONE kernel shape for every step: the sub-lattice form.  The pixels of equal (x mod s, y mod s) form an image
//                 of ceil(W / s) x ceil(H / s) on which the step-s filter is a dense 5 x 5; a block takes 16 x 16 pixels of one
//                 sub-lattice and stages the 20 x 20 records around them in LDS, so the halo is 2 lattice pixels at any step
//                 and no step needs a second code path ("Denoising ray-traced planes").  The variance launch is the
//                 same staging at s = 1.
//   addresses     Every global index is y W + x of a pixel whose coordinates were compared with [0, W) x [0, H) first; a tile
//                 entry outside the image is marked not live and nothing is read for it.
//   determinism   One pixel per thread, no atomics, one barrier after the staging, no thread waits on another: the result is a
//                 pure function of the inputs.
#include <cfloat>

#include "gigs_internal.h"

namespace gigs {
namespace denoise {

constexpr int kTile = 16, kHalo = 2, kSide = kTile + 2 * kHalo, kCells = kSide * kSide, kGuide = 8;
constexpr int kMaxChannels = GIGS_DENOISE_MAX_CHANNELS;

struct Args {
  int W, H, C, G, S;        // S: floats of a signal record
  int step, tiles_x, tiles_y;
  int e, use_rough;         // normal_power = 2^e
  float inv_plane2, inv_rough2, sigma_l2, eps;
  const float* guide;       // [H W, kGuide]
  const float* in;          // [H W, S]
  float* out;               // [H W, S], never `in`
  unsigned char size[kMaxChannels];  // the channels of each group, 1 or 3
};

__device__ __forceinline__ bool finite(float v) { return fabsf(v) <= FLT_MAX; }

__global__ __launch_bounds__(256) void pack_kernel(int W, int H, int C, int G, int S, const float* __restrict__ signal,
                                                   const float* __restrict__ points, const float* __restrict__ normals,
                                                   const unsigned char* __restrict__ mask, const float* __restrict__ roughness,
                                                   float* __restrict__ guide, float* __restrict__ record) {
  const size_t n = (size_t)W * H, q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  float g[kGuide];
  bool live = mask[q] != 0;
#pragma unroll
  for (int c = 0; c < 3; c++) {
    g[c] = points[3 * q + c];
    g[3 + c] = normals[3 * q + c];
    live = live && finite(g[c]) && finite(g[3 + c]);
  }
  g[6] = roughness ? roughness[q] : 0.0f;
  live = live && finite(g[6]);
  float* rec = record + q * S;
  for (int c = 0; c < C; c++) {
    const float x = signal[(size_t)c * n + q];
    live = live && finite(x);
    rec[c] = x;
  }
  for (int c = C; c < S; c++) rec[c] = 0.0f;
  g[7] = live ? 1.0f : 0.0f;
  float4* gq = reinterpret_cast<float4*>(guide + q * kGuide);
  gq[0] = make_float4(g[0], g[1], g[2], g[3]);
  gq[1] = make_float4(g[4], g[5], g[6], g[7]);
}

__global__ __launch_bounds__(256) void unpack_kernel(int W, int H, int C, int G, int S, const float* __restrict__ record,
                                                     float* __restrict__ filtered, float* __restrict__ variance) {
  const size_t n = (size_t)W * H, q = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (q >= n) return;
  const float* rec = record + q * S;
  for (int c = 0; c < C; c++) filtered[(size_t)c * n + q] = rec[c];
  for (int j = 0; j < G; j++) variance[(size_t)j * n + q] = rec[C + j];
}

// The value of a group: x_0, or (x_0 + x_1) + x_2.
__device__ __forceinline__ float value(const float* x, int nc) { return nc == 1 ? x[0] : (x[0] + x[1]) + x[2]; }

// kVariance: launch A (step 1: the values of `in` with their variances); otherwise one a-trous step.  in -> out.
template <bool kVariance>
__global__ __launch_bounds__(256) void filter_kernel(Args a) {
  extern __shared__ float4 lds4[];
  float* lg = reinterpret_cast<float*>(lds4);  // [kCells][kGuide]
  float* ls = lg + kCells * kGuide;            // [kCells][S]
  const int s = a.step, S = a.S;
  const int tile_x = blockIdx.x / s, ox = blockIdx.x - tile_x * s;
  const int tile_y = blockIdx.y / s, oy = blockIdx.y - tile_y * s;
  const int tid = threadIdx.x;
  for (int t = tid; t < kCells; t += 256) {
    const int j = t / kSide, i = t - j * kSide;
    const int u = tile_x * kTile + i - kHalo, v = tile_y * kTile + j - kHalo;  // lattice coordinates
    const int x = u * s + ox, y = v * s + oy;
    float4* dg = reinterpret_cast<float4*>(lg + t * kGuide);
    if (u >= 0 && v >= 0 && x < a.W && y < a.H) {
      const size_t q = (size_t)y * a.W + x;
      const float4* sg = reinterpret_cast<const float4*>(a.guide + q * kGuide);
      dg[0] = sg[0];
      dg[1] = sg[1];
      const float4* sr = reinterpret_cast<const float4*>(a.in + q * S);
      float4* dr = reinterpret_cast<float4*>(ls + t * S);
      for (int k = 0; k < S / 4; k++) dr[k] = sr[k];
    } else {  // outside the image: not live, nothing read
      dg[0] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      dg[1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
  }
  __syncthreads();
  const int ty = tid / kTile, tx = tid - ty * kTile;
  const int x = (tile_x * kTile + tx) * s + ox, y = (tile_y * kTile + ty) * s + oy;
  if (x >= a.W || y >= a.H) return;
  const int tc = (ty + kHalo) * kSide + tx + kHalo;
  const size_t q = (size_t)y * a.W + x;
  const float* gp = lg + tc * kGuide;
  const float* xp = ls + tc * S;
  if (gp[7] == 0.0f) {  // not live: keeps its bits, variance 0 (written by the pack)
    for (int k = 0; k < S; k++) a.out[q * S + k] = xp[k];
    return;
  }
  // the geometry weights of the 25 taps, row-major; `alive` has bit k set for a live tap inside the image
  float g[25];
  unsigned alive = 0u;
#pragma unroll
  for (int dy = 0; dy < 5; dy++) {
#pragma unroll
    for (int dx = 0; dx < 5; dx++) {
      const int k = dy * 5 + dx;
      const float* gq = lg + (tc + (dy - kHalo) * kSide + (dx - kHalo)) * kGuide;
      g[k] = 0.0f;
      if (gq[7] != 0.0f) {
        alive |= 1u << k;
        float c = (gp[3] * gq[3] + gp[4] * gq[4]) + gp[5] * gq[5];
        c = (c > 0.0f) ? c : 0.0f;
        for (int i = 0; i < a.e; i++) c = c * c;
        const float d = ((gq[0] - gp[0]) * gp[3] + (gq[1] - gp[1]) * gp[4]) + (gq[2] - gp[2]) * gp[5];
        float z = 1.0f - (d * d) * a.inv_plane2;
        z = (z > 0.0f) ? z : 0.0f;
        float w = c * (z * z);
        if (a.use_rough) {
          const float dr = gq[6] - gp[6];
          float r = 1.0f - (dr * dr) * a.inv_rough2;
          r = (r > 0.0f) ? r : 0.0f;
          w = w * (r * r);
        }
        g[k] = w;
      }
    }
  }
  int c0 = 0;
  for (int j = 0; j < a.G; j++) {
    const int nc = a.size[j];
    const float yp = value(xp + c0, nc);
    if (kVariance) {
      float G = 0.0f, sum = 0.0f;
#pragma unroll
      for (int k = 0; k < 25; k++) {
        if (alive >> k & 1u) {
          const float* xq = ls + (tc + (k / 5 - kHalo) * kSide + (k % 5 - kHalo)) * S + c0;
          G += g[k];
          sum += g[k] * (value(xq, nc) - yp);
        }
      }
      float var = 0.0f;
      if (G > 0.0f) {
        const float m = yp + sum / G;
        float dev = 0.0f;
#pragma unroll
        for (int k = 0; k < 25; k++) {
          if (alive >> k & 1u) {
            const float* xq = ls + (tc + (k / 5 - kHalo) * kSide + (k % 5 - kHalo)) * S + c0;
            const float t = value(xq, nc) - m;
            dev += g[k] * (t * t);
          }
        }
        var = dev / G;
      }
      a.out[q * S + a.C + j] = var;
    } else {
      const float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
      const float r = 1.0f / (a.sigma_l2 * xp[a.C + j] + a.eps);
      float Wsum = 0.0f, V = 0.0f, D[3] = {0.0f, 0.0f, 0.0f};
#pragma unroll
      for (int k = 0; k < 25; k++) {
        if (alive >> k & 1u) {
          const float* rq = ls + (tc + (k / 5 - kHalo) * kSide + (k % 5 - kHalo)) * S;
          const float* xq = rq + c0;
          const float delta = value(xq, nc) - yp;
          float wl = 1.0f - (delta * delta) * r;
          wl = (wl > 0.0f) ? wl : 0.0f;
          const float w = ((h[k / 5] * h[k % 5]) * g[k]) * (wl * wl);
          Wsum += w;
#pragma unroll
          for (int c = 0; c < 3; c++)
            if (c < nc) D[c] += w * (xq[c] - xp[c0 + c]);
          V += (w * w) * rq[a.C + j];
        }
      }
      if (Wsum > 0.0f) {
#pragma unroll
        for (int c = 0; c < 3; c++)
          if (c < nc) a.out[q * S + c0 + c] = xp[c0 + c] + D[c] / Wsum;
        a.out[q * S + a.C + j] = V / (Wsum * Wsum);
      } else {
        for (int c = 0; c < nc; c++) a.out[q * S + c0 + c] = xp[c0 + c];
        a.out[q * S + a.C + j] = xp[a.C + j];
      }
    }
    c0 += nc;
  }
  if (kVariance)
    for (int c = 0; c < a.C; c++) a.out[q * S + c] = xp[c];
  for (int k = a.C + a.G; k < S; k++) a.out[q * S + k] = 0.0f;
}

// Shape and groups, checked as one: fills the common part of Args.  0 on a bad argument.
bool make_args(int width, int height, int channels, int n_groups, const int* groups, Args* a) {
  if (width < 0 || height < 0 || channels < 1 || channels > kMaxChannels || n_groups < 1 || n_groups > channels || !groups) return false;
  if ((long long)width * height > 0x7fffffffLL) return false;
  int sum = 0;
  for (int j = 0; j < n_groups; j++) {
    if (groups[j] != 1 && groups[j] != 3) return false;
    a->size[j] = (unsigned char)groups[j];
    sum += groups[j];
  }
  if (sum != channels) return false;
  a->W = width, a->H = height, a->C = channels, a->G = n_groups, a->S = 4 * ((channels + n_groups + 3) / 4);
  return true;
}

template <bool kVariance>
int launch(Args& a, int step, hipStream_t s, const char* entry) {
  a.step = step;
  a.tiles_x = ((a.W + step - 1) / step + kTile - 1) / kTile;
  a.tiles_y = ((a.H + step - 1) / step + kTile - 1) / kTile;
  if ((long long)a.tiles_x * step > 0x7fffffffLL || (long long)a.tiles_y * step > 65535LL)
    return gigs_internal_fail(GIGS_ERR_INVALID, "denoise: the image is too large for one launch");
  const size_t lds = (size_t)kCells * (kGuide + a.S) * sizeof(float);  // at most 400 (8 + 32) 4 = 64000 bytes
  hipLaunchKernelGGL(filter_kernel<kVariance>, dim3((unsigned)(a.tiles_x * step), (unsigned)(a.tiles_y * step)), dim3(256), lds, s, a);
  return gigs_internal_check_launch(entry);
}

}  // namespace denoise
}  // namespace gigs

extern "C" {

int gigs_denoise_pack(int width, int height, int channels, int n_groups, const int* groups, const float* signal,
                      const float* points, const float* normals, const unsigned char* mask, const float* roughness,
                      float* guide, float* record, void* stream) {
  using namespace gigs::denoise;
  Args a;
  if (!make_args(width, height, channels, n_groups, groups, &a)) return gigs_internal_fail(GIGS_ERR_INVALID, "denoise_pack: bad argument");
  const long long n = (long long)width * height;
  if (n == 0) return 0;
  if (!signal || !points || !normals || !mask || !guide || !record) return gigs_internal_fail(GIGS_ERR_INVALID, "denoise_pack: NULL array");
  hipLaunchKernelGGL(pack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a.W, a.H, a.C, a.G, a.S, signal,
                     points, normals, mask, roughness, guide, record);
  return gigs_internal_check_launch("denoise_pack");
}

int gigs_denoise_variance(int width, int height, int channels, int n_groups, const int* groups, int normal_exponent,
                          float inv_plane2, int use_roughness, float inv_rough2, const float* guide, const float* record_in,
                          float* record_out, void* stream) {
  using namespace gigs::denoise;
  Args a;
  if (!make_args(width, height, channels, n_groups, groups, &a) || normal_exponent < 0 || normal_exponent > 7 || !(inv_plane2 >= 0.0f) ||
      !(inv_plane2 <= FLT_MAX) || (use_roughness && (!(inv_rough2 >= 0.0f) || !(inv_rough2 <= FLT_MAX))) ||
      record_in == record_out)
    return gigs_internal_fail(GIGS_ERR_INVALID, "denoise_variance: bad argument");
  if ((long long)width * height == 0) return 0;
  if (!guide || !record_in || !record_out) return gigs_internal_fail(GIGS_ERR_INVALID, "denoise_variance: NULL array");
  a.e = normal_exponent, a.use_rough = use_roughness ? 1 : 0, a.inv_plane2 = inv_plane2, a.inv_rough2 = inv_rough2;
  a.sigma_l2 = 0.0f, a.eps = 0.0f, a.guide = guide, a.in = record_in, a.out = record_out;
  return launch<true>(a, 1, (hipStream_t)stream, "denoise_variance");
}

int gigs_denoise_atrous(int width, int height, int channels, int n_groups, const int* groups, int step, int normal_exponent,
                        float inv_plane2, int use_roughness, float inv_rough2, float sigma_l2, float eps, const float* guide,
                        const float* record_in, float* record_out, void* stream) {
  using namespace gigs::denoise;
  Args a;
  const bool pow2 = step >= 1 && step <= GIGS_DENOISE_MAX_STEP && (step & (step - 1)) == 0;
  if (!make_args(width, height, channels, n_groups, groups, &a) || !pow2 || normal_exponent < 0 || normal_exponent > 7 ||
      !(inv_plane2 >= 0.0f) || !(inv_plane2 <= FLT_MAX) || (use_roughness && (!(inv_rough2 >= 0.0f) || !(inv_rough2 <= FLT_MAX))) ||
      !(sigma_l2 >= 0.0f) || !(sigma_l2 <= FLT_MAX) || !(eps > 0.0f) || record_in == record_out)
    return gigs_internal_fail(GIGS_ERR_INVALID, "denoise_atrous: bad argument");
  if ((long long)width * height == 0) return 0;
  if (!guide || !record_in || !record_out) return gigs_internal_fail(GIGS_ERR_INVALID, "denoise_atrous: NULL array");
  a.e = normal_exponent, a.use_rough = use_roughness ? 1 : 0, a.inv_plane2 = inv_plane2, a.inv_rough2 = inv_rough2;
  a.sigma_l2 = sigma_l2, a.eps = eps, a.guide = guide, a.in = record_in, a.out = record_out;
  return launch<false>(a, step, (hipStream_t)stream, "denoise_atrous");
}

int gigs_denoise_unpack(int width, int height, int channels, int n_groups, const int* groups, const float* record, float* filtered,
                        float* variance, void* stream) {
  using namespace gigs::denoise;
  Args a;
  if (!make_args(width, height, channels, n_groups, groups, &a)) return gigs_internal_fail(GIGS_ERR_INVALID, "denoise_unpack: bad argument");
  const long long n = (long long)width * height;
  if (n == 0) return 0;
  if (!record || !filtered || !variance) return gigs_internal_fail(GIGS_ERR_INVALID, "denoise_unpack: NULL array");
  hipLaunchKernelGGL(unpack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, a.W, a.H, a.C, a.G, a.S, record,
                     filtered, variance);
  return gigs_internal_check_launch("denoise_unpack");
}
}  // extern "C"
