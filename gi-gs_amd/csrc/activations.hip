// activations.hip -- parameter activations (scene/gaussian_model.py:48-58, 178-263).
//
// get_features = cat(f_dc, f_rest), get_opacity / albedo / roughness / metallic = sigmoid, get_scaling = exp,
// get_rotation / get_normal = F.normalize(dim=-1, eps=1e-12): eight getters, ~10 torch kernels forward and ~20 backward
// per iteration; here one launch each way (the SH concatenation in 64-Gaussian tiles, then the sixteen small attributes
// one Gaussian per lane).
#include <cstring>

#include "gigs_internal.h"

namespace gigs {

struct ActPtrs {
  const float *f_dc, *f_rest, *opacity, *normal, *albedo, *roughness, *metallic, *scaling, *rotation;  // raw
  float *shs, *o_opacity, *o_normal, *o_albedo, *o_roughness, *o_metallic, *o_scales, *o_rotations;    // fwd outputs
  const float *g_shs, *g_opacity, *g_normal, *g_albedo, *g_roughness, *g_metallic, *g_scales, *g_rotations;  // bwd inputs
  float *d_f_dc, *d_f_rest, *d_opacity, *d_normal, *d_albedo, *d_roughness, *d_metallic, *d_scaling, *d_rotation;
};
__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

template <int N>
__device__ __forceinline__ void normalize_fwd(const float* __restrict__ v, float* __restrict__ o) {
  float n2 = 0.0f;
#pragma unroll
  for (int k = 0; k < N; k++) n2 += v[k] * v[k];
  const float d = fmaxf(sqrtf(n2), 1e-12f);
#pragma unroll
  for (int k = 0; k < N; k++) o[k] = v[k] / d;
}
// d/dv of v / max(|v|, eps): below eps the denominator is the constant eps
template <int N>
__device__ __forceinline__ void normalize_bwd(const float* __restrict__ v, const float* __restrict__ g,
                                              float* __restrict__ d) {
  float n2 = 0.0f, vg = 0.0f;
#pragma unroll
  for (int k = 0; k < N; k++) { n2 += v[k] * v[k]; vg += v[k] * g[k]; }
  const float n = sqrtf(n2);
  if (n > 1e-12f) {
    const float s = vg / (n2 * n);
#pragma unroll
    for (int k = 0; k < N; k++) d[k] = g[k] / n - v[k] * s;
  } else {
#pragma unroll
    for (int k = 0; k < N; k++) d[k] = g[k] / 1e-12f;
  }
}

// The SH concatenation cat(f_dc [P,1,3], f_rest [P,K-1,3]) -> shs [P,K,3] (and its backward, the split) moves 24*K bytes
// per Gaussian: a tile of 64 Gaussians is contiguous in all three arrays, so it is read with 16-byte loads, re-laid out in
// LDS (which holds the tile in the concatenated layout) and written with 16-byte stores.  One float per lane with a
// division for its (row, column) ran at 3 TB/s; pointers that are not 16-byte aligned (views into a gradient slab) take
// the scalar form of the same loops.
constexpr int kActRows = 64;
constexpr int kActMaxRowF = 48;  // K <= 16 (SH degree 3)

__device__ __forceinline__ int act_div_small(int x, float inv) {  // x / d for 0 <= x < 2^12, inv = 1 / d
  return (int)(((float)x + 0.5f) * inv);
}
__device__ __forceinline__ bool act_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// global [n] (contiguous) -> LDS rows of `stride` floats starting at column `col0`, `width` floats per row
__device__ __forceinline__ void act_tile_in(const float* __restrict__ src, int n, int width, float* tile, int stride, int col0) {
  const float inv = 1.0f / (float)width;
  const int n4 = act_aligned16(src) ? n / 4 : 0;
  for (int j = threadIdx.x; j < n4; j += 256) {
    const float4 v = reinterpret_cast<const float4*>(src)[j];
    const float e4[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int e = 4 * j + k, r = act_div_small(e, inv);
      tile[r * stride + col0 + (e - r * width)] = e4[k];
    }
  }
  for (int e = 4 * n4 + threadIdx.x; e < n; e += 256) {
    const int r = act_div_small(e, inv);
    tile[r * stride + col0 + (e - r * width)] = src[e];
  }
}
// LDS rows -> global [n] (contiguous)
__device__ __forceinline__ void act_tile_out(float* __restrict__ dst, int n, int width, const float* tile, int stride, int col0) {
  const float inv = 1.0f / (float)width;
  const int n4 = act_aligned16(dst) ? n / 4 : 0;
  for (int j = threadIdx.x; j < n4; j += 256) {
    float e4[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int e = 4 * j + k, r = act_div_small(e, inv);
      e4[k] = tile[r * stride + col0 + (e - r * width)];
    }
    reinterpret_cast<float4*>(dst)[j] = make_float4(e4[0], e4[1], e4[2], e4[3]);
  }
  for (int e = 4 * n4 + threadIdx.x; e < n; e += 256) {
    const int r = act_div_small(e, inv);
    dst[e] = tile[r * stride + col0 + (e - r * width)];
  }
}

__device__ __forceinline__ void act_sh_tile_fwd(int P, int row_f, const ActPtrs& A, int tile_id, float* tile) {
  const int r0 = tile_id * kActRows, rows = min(kActRows, P - r0);
  act_tile_in(A.f_dc + 3 * (size_t)r0, rows * 3, 3, tile, row_f, 0);
  if (row_f > 3) act_tile_in(A.f_rest + (size_t)r0 * (row_f - 3), rows * (row_f - 3), row_f - 3, tile, row_f, 3);
  __syncthreads();
  act_tile_out(A.shs + (size_t)r0 * row_f, rows * row_f, row_f, tile, row_f, 0);
}
__device__ __forceinline__ void act_sh_tile_bwd(int P, int row_f, const ActPtrs& A, int tile_id, float* tile) {
  const int r0 = tile_id * kActRows, rows = min(kActRows, P - r0);
  if (A.g_shs) act_tile_in(A.g_shs + (size_t)r0 * row_f, rows * row_f, row_f, tile, row_f, 0);
  else for (int e = threadIdx.x; e < rows * row_f; e += 256) tile[e] = 0.0f;
  __syncthreads();
  if (A.d_f_dc) act_tile_out(A.d_f_dc + 3 * (size_t)r0, rows * 3, 3, tile, row_f, 0);
  if (row_f > 3 && A.d_f_rest) act_tile_out(A.d_f_rest + (size_t)r0 * (row_f - 3), rows * (row_f - 3), row_f - 3, tile, row_f, 3);
}

// grid: the SH tiles first, then one block per 256 Gaussians for the sixteen small attributes
__global__ void __launch_bounds__(256)
activate_fwd_kernel(int P, int K, ActPtrs A, int sh_tiles) {
  __shared__ __align__(16) float tile[kActRows * kActMaxRowF];
  if ((int)blockIdx.x < sh_tiles) {
    act_sh_tile_fwd(P, 3 * K, A, blockIdx.x, tile);
    return;
  }
  const int i = ((int)blockIdx.x - sh_tiles) * 256 + threadIdx.x;
  if (i >= P) return;
  A.o_opacity[i] = sigmoidf(A.opacity[i]);
  A.o_roughness[i] = sigmoidf(A.roughness[i]);
  A.o_metallic[i] = sigmoidf(A.metallic[i]);
#pragma unroll
  for (int k = 0; k < 3; k++) {
    A.o_albedo[3 * i + k] = sigmoidf(A.albedo[3 * i + k]);
    A.o_scales[3 * i + k] = expf(A.scaling[3 * i + k]);
  }
  normalize_fwd<3>(A.normal + 3 * i, A.o_normal + 3 * i);
  normalize_fwd<4>(A.rotation + 4 * i, A.o_rotations + 4 * i);
}

__global__ void __launch_bounds__(256)
activate_bwd_kernel(int P, int K, ActPtrs A, int sh_tiles) {
  __shared__ __align__(16) float tile[kActRows * kActMaxRowF];
  if ((int)blockIdx.x < sh_tiles) {
    act_sh_tile_bwd(P, 3 * K, A, blockIdx.x, tile);
    return;
  }
  const int i = ((int)blockIdx.x - sh_tiles) * 256 + threadIdx.x;
  if (i >= P) return;
  // a NULL output (gigs_activate_bwd: the caller keeps no tensor for a gradient it knows to be zero) is neither computed nor written
  if (A.d_opacity) {
    const float s = sigmoidf(A.opacity[i]);
    A.d_opacity[i] = A.g_opacity ? A.g_opacity[i] * (s * (1.0f - s)) : 0.0f;
  }
  if (A.d_roughness) {
    const float r = sigmoidf(A.roughness[i]);
    A.d_roughness[i] = A.g_roughness ? A.g_roughness[i] * (r * (1.0f - r)) : 0.0f;
  }
  if (A.d_metallic) {
    const float m = sigmoidf(A.metallic[i]);
    A.d_metallic[i] = A.g_metallic ? A.g_metallic[i] * (m * (1.0f - m)) : 0.0f;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    if (A.d_albedo) {
      const float a = sigmoidf(A.albedo[3 * i + k]);
      A.d_albedo[3 * i + k] = A.g_albedo ? A.g_albedo[3 * i + k] * (a * (1.0f - a)) : 0.0f;
    }
    if (A.d_scaling) A.d_scaling[3 * i + k] = A.g_scales ? A.g_scales[3 * i + k] * expf(A.scaling[3 * i + k]) : 0.0f;
  }
  const float z4[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (A.d_normal) normalize_bwd<3>(A.normal + 3 * i, A.g_normal ? A.g_normal + 3 * i : z4, A.d_normal + 3 * i);
  if (A.d_rotation) normalize_bwd<4>(A.rotation + 4 * i, A.g_rotations ? A.g_rotations + 4 * i : z4, A.d_rotation + 4 * i);
}

}  // namespace gigs

static bool act_raw_ok(const gigs_activation_raw* r, int K) {
  return r && r->f_dc && (K == 1 || r->f_rest) && r->opacity && r->normal && r->albedo && r->roughness && r->metallic &&
         r->scaling && r->rotation;
}
static void act_fill_raw(gigs::ActPtrs& A, const gigs_activation_raw* r) {
  A.f_dc = r->f_dc; A.f_rest = r->f_rest; A.opacity = r->opacity; A.normal = r->normal; A.albedo = r->albedo;
  A.roughness = r->roughness; A.metallic = r->metallic; A.scaling = r->scaling; A.rotation = r->rotation;
}

extern "C" {

int gigs_activate_fwd(int P, int K, const gigs_activation_raw* raw, const gigs_activation_out* out, void* stream) {
  if (P < 0 || K < 1 || 3 * K > gigs::kActMaxRowF || (P > 0 && (!act_raw_ok(raw, K) || !out || !out->opacities || !out->normal ||
                                   !out->albedo || !out->roughness || !out->metallic || !out->scales || !out->rotations)))
    return gigs_internal_fail(GIGS_ERR_INVALID, "activate_fwd: bad argument");
  if (P == 0) return 0;
  gigs::ActPtrs A;
  memset(&A, 0, sizeof(A));
  act_fill_raw(A, raw);
  A.shs = out->shs; A.o_opacity = out->opacities; A.o_normal = out->normal; A.o_albedo = out->albedo;
  A.o_roughness = out->roughness; A.o_metallic = out->metallic; A.o_scales = out->scales; A.o_rotations = out->rotations;
  gigs::StageTimer timer(gigs::Stage::kActivateFwd, stream);
  const int sh_tiles = A.shs ? (P + gigs::kActRows - 1) / gigs::kActRows : 0;  // no concatenation without an output for it
  hipLaunchKernelGGL(gigs::activate_fwd_kernel, dim3((unsigned)(sh_tiles + (P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P, K,
                     A, sh_tiles);
  return gigs_internal_check_launch("activate_fwd");
}

int gigs_activate_bwd(int P, int K, const gigs_activation_raw* raw, const gigs_activation_out* grad_out,
                      const gigs_activation_raw_grad* grad_raw, void* stream) {
  if (P < 0 || K < 1 || 3 * K > gigs::kActMaxRowF || (P > 0 && (!act_raw_ok(raw, K) || !grad_out || !grad_raw)))
    return gigs_internal_fail(GIGS_ERR_INVALID, "activate_bwd: bad argument");
  if (P == 0) return 0;
  gigs::ActPtrs A;
  memset(&A, 0, sizeof(A));
  act_fill_raw(A, raw);
  A.g_shs = grad_out->shs; A.g_opacity = grad_out->opacities; A.g_normal = grad_out->normal; A.g_albedo = grad_out->albedo;
  A.g_roughness = grad_out->roughness; A.g_metallic = grad_out->metallic; A.g_scales = grad_out->scales;
  A.g_rotations = grad_out->rotations;
  A.d_f_dc = grad_raw->f_dc; A.d_f_rest = grad_raw->f_rest; A.d_opacity = grad_raw->opacity; A.d_normal = grad_raw->normal;
  A.d_albedo = grad_raw->albedo; A.d_roughness = grad_raw->roughness; A.d_metallic = grad_raw->metallic;
  A.d_scaling = grad_raw->scaling; A.d_rotation = grad_raw->rotation;
  gigs::StageTimer timer(gigs::Stage::kActivateBwd, stream);
  // no SH tile when neither SH gradient is wanted
  const int sh_tiles = (A.d_f_dc || A.d_f_rest) ? (P + gigs::kActRows - 1) / gigs::kActRows : 0;
  hipLaunchKernelGGL(gigs::activate_bwd_kernel, dim3((unsigned)(sh_tiles + (P + 255) / 256)), dim3(256), 0, (hipStream_t)stream, P, K,
                     A, sh_tiles);
  return gigs_internal_check_launch("activate_bwd");
}

}  // extern "C"
