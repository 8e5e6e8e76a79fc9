// stage2.hip -- the tensor glue of one stage-2 ("PBR + indirect") iteration as three kernels.
//
// The reference expresses these steps as a few dozen torch elementwise / reduction ops in
// gaussian_renderer/__init__.py:157-199 (G-buffer post-processing) and train.py:382-402 (loss); on
// an MI355X each of those ops is a 3-10 us launch over 0.6 M pixels, ~1.8 ms per iteration in total.
// Here they are one pass each.  Results agree with the torch formulation to fp32 rounding (the same
// formulas; tests/test_gpu_pbr.py compares them).
//
//   gbuffer_post_kernel   masks, F.normalize, 3x3 median and the rotation of the shading normal into
//                         view space, for normal_map and out_normal_view (no gradient: train.py detaches
//                         both before they are used in stage 2)
//   stage2_loss_fwd       IRR -> sRGB -> 3x3 median -> + direct -> L1 vs ground truth, plus the masked
//                         sums of the "lamb" regulariser; block-reduced, 4 atomics per workgroup
//   stage2_loss_bwd       the gradient of that loss w.r.t. render_direct, IRR (through the median's tap
//                         selection and the sRGB curve) and the roughness / metallic maps
// All planes are [C,H,W] fp32, the rasterizer's layout.  HBM-bound streaming kernels.
#include <cstdint>

#include "block_reduce.h"
#include "gigs_internal.h"
#include "pixel_ops.h"

namespace gigs {

// opacity of gaussian_renderer/__init__.py:160-169 (pad_normal): < 0.004 -> 0, then > 1 - 0.004 -> 1 (fp32 thresholds,
// as torch compares an fp32 tensor with a Python scalar)
__device__ __forceinline__ float pad_opacity(float a) {
  a = a < 0.004f ? 0.0f : a;
  return a > (float)(1.0 - 0.004) ? 1.0f : a;
}

// pad_normal's blend over the background normal (0, 0, 1): n * a + (1 - a) * bg, per channel as torch rounds it
__device__ __forceinline__ v3 pad_normal_over_bg(v3 n, float a) {
  const float r = 1.0f - a;
  return {n.x * a + r * 0.0f, n.y * a + r * 0.0f, n.z * a + r * 1.0f};
}

// per-channel 3x3 median of normalize_where(src) with zero padding; NaN window -> NaN (as median3x3_kernel).
// opacity != NULL: every tap is first blended over the background normal (pad_normal); padding taps stay zero.
template <bool kPad>
__device__ __forceinline__ v3 median_of_normalized(const float* __restrict__ src, const float* __restrict__ opacity,
                                                   int H, int W, int y, int x) {
  const size_t HW = (size_t)H * W;
  float t0[9], t1[9], t2[9];
  bool n0 = false, n1 = false, n2 = false;
  int k = 0;
#pragma unroll
  for (int dy = -1; dy <= 1; dy++)
#pragma unroll
    for (int dx = -1; dx <= 1; dx++, k++) {
      const int yy = y + dy, xx = x + dx;
      v3 v = {0.0f, 0.0f, 0.0f};
      if (!(yy < 0 || yy >= H || xx < 0 || xx >= W)) {
        const size_t q = (size_t)yy * W + xx;
        v = {src[q], src[HW + q], src[2 * HW + q]};
        if (kPad) v = pad_normal_over_bg(v, pad_opacity(opacity[q]));
        v = normalize_where(v);
      }
      t0[k] = v.x; t1[k] = v.y; t2[k] = v.z;
      n0 |= v.x != v.x; n1 |= v.y != v.y; n2 |= v.z != v.z;
    }
  const float nan = __builtin_nanf("");
  return {n0 ? nan : median9(t0), n1 ? nan : median9(t1), n2 ? nan : median9(t2)};
}

// Optional outputs (pad_normal, render.py:212): kPad blends normal_map over the background normal by the thresholded
// opacity before it is normalised and filtered (the mask still comes from the unpadded map) and also writes
// normal_world (the filtered world-space map), the padded + normalised normal_map_from_depth and the opacity itself.
struct GbufferPad {
  const float* opacity;
  const float* nfd;
  float* normal_world;
  float* nfd_out;
  float* opacity_out;
};

template <bool kPad>
__global__ void __launch_bounds__(256)
gbuffer_post_kernel(int H, int W, const float* __restrict__ normal_map, const float* __restrict__ out_normal_view,
                    const float* __restrict__ vm, float* __restrict__ normals_view, uint8_t* __restrict__ mask_u8,
                    float* __restrict__ mask_f, float* __restrict__ onv, GbufferPad pad) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const size_t HW = (size_t)H * W, p = (size_t)y * W + x;
  const bool mk = normal_map[p] != 0.0f && normal_map[HW + p] != 0.0f && normal_map[2 * HW + p] != 0.0f;
  if (mask_u8) mask_u8[p] = mk ? 1 : 0;
  if (mask_f) mask_f[p] = mk ? 1.0f : 0.0f;
  const v3 n = median_of_normalized<kPad>(normal_map, pad.opacity, H, W, y, x);
  // -(n @ R), R = viewmatrix[:3, :3] of the row-major 4x4 tensor
  normals_view[p] = -(n.x * vm[0] + n.y * vm[4] + n.z * vm[8]);
  normals_view[HW + p] = -(n.x * vm[1] + n.y * vm[5] + n.z * vm[9]);
  normals_view[2 * HW + p] = -(n.x * vm[2] + n.y * vm[6] + n.z * vm[10]);
  const v3 o = median_of_normalized<false>(out_normal_view, nullptr, H, W, y, x);
  onv[p] = o.x; onv[HW + p] = o.y; onv[2 * HW + p] = o.z;
  if (kPad) {
    if (pad.normal_world) { pad.normal_world[p] = n.x; pad.normal_world[HW + p] = n.y; pad.normal_world[2 * HW + p] = n.z; }
    if (pad.opacity_out) pad.opacity_out[p] = pad_opacity(pad.opacity[p]);
    if (pad.nfd_out) {
      // mask_from_depth = (v == 0).all(0): v * (1 - m) + m * bg, then normalize_where
      v3 d = {pad.nfd[p], pad.nfd[HW + p], pad.nfd[2 * HW + p]};
      const float m = (d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) ? 1.0f : 0.0f;
      d = {d.x * (1.0f - m) + m * 0.0f, d.y * (1.0f - m) + m * 0.0f, d.z * (1.0f - m) + m * 1.0f};
      d = normalize_where(d);
      pad.nfd_out[p] = d.x; pad.nfd_out[HW + p] = d.y; pad.nfd_out[2 * HW + p] = d.z;
    }
  }
}

// ---- backward of the normal post-processing (stage 1: train.py:327-328 differentiates through
// gaussian_renderer/__init__.py:160-186) ---------------------------------------------------------------------------
// normals_view = -(median3x3(normalize_where(normal_map)) @ R).  Pass 1, one lane per output pixel: rotate the
// incoming gradient back, g_med[c] = -sum_j R[c][j] g[j], and hand it to the tap the median selected (first tap in
// row-major order equal to the median, as median3x3_bwd_kernel; padding taps and NaN windows drop it).  Pass 2, one
// lane per source pixel: the derivative of normalize_where.
__global__ void __launch_bounds__(256)
gbuffer_post_bwd_scatter_kernel(int H, int W, const float* __restrict__ normal_map, const float* __restrict__ vm,
                                const float* __restrict__ g_nv, float* __restrict__ g_hat) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63);
  const int y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const size_t HW = (size_t)H * W, p = (size_t)y * W + x;
  const float g0 = g_nv[p], g1 = g_nv[HW + p], g2 = g_nv[2 * HW + p];
  float gm[3];
#pragma unroll
  for (int c = 0; c < 3; c++) gm[c] = -(vm[4 * c] * g0 + vm[4 * c + 1] * g1 + vm[4 * c + 2] * g2);
  if (gm[0] == 0.0f && gm[1] == 0.0f && gm[2] == 0.0f) return;
  float t[3][9];
  bool nan[3] = {false, false, false};
  int k = 0;
#pragma unroll
  for (int dy = -1; dy <= 1; dy++)
#pragma unroll
    for (int dx = -1; dx <= 1; dx++, k++) {
      const int yy = y + dy, xx = x + dx;
      v3 v = {0.0f, 0.0f, 0.0f};
      if (!(yy < 0 || yy >= H || xx < 0 || xx >= W)) {
        const size_t q = (size_t)yy * W + xx;
        v = normalize_where({normal_map[q], normal_map[HW + q], normal_map[2 * HW + q]});
      }
      t[0][k] = v.x; t[1][k] = v.y; t[2][k] = v.z;
      nan[0] |= v.x != v.x; nan[1] |= v.y != v.y; nan[2] |= v.z != v.z;
    }
#pragma unroll
  for (int c = 0; c < 3; c++) {
    if (nan[c] || gm[c] == 0.0f) continue;
    float srt[9];
#pragma unroll
    for (int j = 0; j < 9; j++) srt[j] = t[c][j];
    const float med = median9(srt);
    int sel = -1;
#pragma unroll
    for (int j = 8; j >= 0; j--)
      if (t[c][j] == med) sel = j;  // ends on the first match
    if (sel < 0) continue;
    const int yy = y + sel / 3 - 1, xx = x + sel % 3 - 1;
    if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;  // a zero-padding tap was the median
    atomicAdd(g_hat + c * HW + (size_t)yy * W + xx, gm[c]);
  }
}

__global__ void __launch_bounds__(256)
gbuffer_post_bwd_finish_kernel(size_t HW, const float* __restrict__ normal_map, const float* __restrict__ g_hat,
                               float* __restrict__ g_normal_map) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const float vx = normal_map[p], vy = normal_map[HW + p], vz = normal_map[2 * HW + p];
  const float gx = g_hat[p], gy = g_hat[HW + p], gz = g_hat[2 * HW + p];
  const float n2 = vx * vx + vy * vy + vz * vz;
  const float n = sqrtf(n2);
  float ox = gx, oy = gy, oz = gz;  // |v| == 0 (or NaN): torch.where passes v itself
  if (n > 0.0f) {
    if (n > 1e-12f) {
      const float s = (vx * gx + vy * gy + vz * gz) / (n2 * n);
      ox = gx / n - vx * s; oy = gy / n - vy * s; oz = gz / n - vz * s;
    } else {
      ox = gx / 1e-12f; oy = gy / 1e-12f; oz = gz / 1e-12f;
    }
  }
  g_normal_map[p] = ox; g_normal_map[HW + p] = oy; g_normal_map[2 * HW + p] = oz;
}

// normal_map_from_depth of gaussian_renderer/__init__.py:157-163: mask = (v != 0).all(0), v <- normalize_where(v)
__global__ void __launch_bounds__(256)
normalize_mask_kernel(size_t HW, const float* __restrict__ in, float* __restrict__ out, uint8_t* __restrict__ mask) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  const v3 v = {in[p], in[HW + p], in[2 * HW + p]};
  if (mask) mask[p] = (v.x != 0.0f && v.y != 0.0f && v.z != 0.0f) ? 1 : 0;
  const v3 o = normalize_where(v);
  out[p] = o.x; out[HW + p] = o.y; out[2 * HW + p] = o.z;
}

// mask = (v != 0).all(0) of a [3,H,W] plane set as floats (gaussian_renderer/__init__.py:158; the masked TV's weight):
// torch's `!=` + `.all(0)` + `.float()` are a compare, a fill, a reduction and a cast
__global__ void __launch_bounds__(256)
nonzero_mask_kernel(size_t HW, const float* __restrict__ in, float* __restrict__ mask) {
  const size_t p = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= HW) return;
  mask[p] = (in[p] != 0.0f && in[HW + p] != 0.0f && in[2 * HW + p] != 0.0f) ? 1.0f : 0.0f;
}

// ---- loss -------------------------------------------------------------------------------------
// acc[0] = sum |render_rgb - gt|, acc[1] = sum (1 - roughness) * mask, acc[2] = sum metallic * mask,
// acc[3] = sum mask;  loss = acc0 / (3 H W) + 0.001 * (acc1 / acc3 + acc2 / acc3)   (train.py:396-402)
// linear_to_srgb is a powf per texel; the 3x3 median needs it for 9 taps per pixel and channel.  A workgroup
// (64 x 4 pixels) therefore converts its (64+2) x (4+2) halo tile once per channel into LDS (1.5 powf per pixel
// and channel instead of 9) and the taps are read from there.  Out-of-image taps are 0 (median_blur pads zeros).
constexpr int kTileW = 64, kTileH = 4, kHaloW = kTileW + 2, kHaloH = kTileH + 2;
constexpr int kAccSlots = 256;  // rows of partial sums (gigs_stage2_loss_fwd's acc buffer holds 4 + 4 * kAccSlots floats)
struct LossTaps {
  float v[9];
  bool has_nan;
};
__device__ __forceinline__ void srgb_tile(const float* __restrict__ irr, int H, int W, float (*s_t)[kHaloH][kHaloW]) {
  const size_t HW = (size_t)H * W;
  const int x0 = blockIdx.x * kTileW - 1, y0 = blockIdx.y * kTileH - 1;
  for (int i = threadIdx.x; i < 3 * kHaloH * kHaloW; i += 256) {
    const int c = i / (kHaloH * kHaloW), r = i - c * (kHaloH * kHaloW);
    const int ty = r / kHaloW, tx = r - ty * kHaloW;
    const int yy = y0 + ty, xx = x0 + tx;
    float v = 0.0f, d;
    if (!(yy < 0 || yy >= H || xx < 0 || xx >= W)) v = lin2srgb(irr[c * HW + (size_t)yy * W + xx], d);
    s_t[c][ty][tx] = v;
  }
  __syncthreads();
}
__device__ __forceinline__ LossTaps srgb_taps(const float (*s_c)[kHaloW], int ly, int lx) {
  LossTaps t;
  t.has_nan = false;
  int k = 0;
#pragma unroll
  for (int dy = 0; dy <= 2; dy++)
#pragma unroll
    for (int dx = 0; dx <= 2; dx++, k++) {
      const float s = s_c[ly + dy][lx + dx];
      t.v[k] = s;
      t.has_nan |= s != s;
    }
  return t;
}

__global__ void __launch_bounds__(256)
stage2_loss_fwd_kernel(int H, int W, const float* __restrict__ direct, const float* __restrict__ irr,
                       const float* __restrict__ gt, const float* __restrict__ mask_f,
                       const float* __restrict__ roughness, const float* __restrict__ metallic,
                       float* __restrict__ render_rgb, float* __restrict__ acc, float* __restrict__ d_direct_unit,
                       float* __restrict__ d_irr_unit) {
  __shared__ float s_red[4];
  __shared__ float s_t[3][kHaloH][kHaloW];
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const int x = blockIdx.x * kTileW + lx;
  const int y = blockIdx.y * kTileH + ly;
  const bool live = x < W && y < H;
  const size_t HW = (size_t)H * W, p = live ? (size_t)y * W + x : 0;
  float l1 = 0.0f, rs = 0.0f, ms = 0.0f, cnt = 0.0f;
  srgb_tile(irr, H, W, s_t);
  if (live) {
#pragma unroll
    for (int c = 0; c < 3; c++) {
      LossTaps t = srgb_taps(s_t[c], ly, lx);
      float sorted[9];
#pragma unroll
      for (int k = 0; k < 9; k++) sorted[k] = t.v[k];
      const float med = t.has_nan ? __builtin_nanf("") : median9(sorted);
      const float r = direct[c * HW + p] + med;
      if (render_rgb) render_rgb[c * HW + p] = r;
      const float diff = r - gt[c * HW + p];
      l1 += fabsf(diff);
      if (d_direct_unit) {
        // stage2_loss_bwd_kernel's work for a unit upstream gradient, on the tile and the median this pass already has
        const float gs = 1.0f / (3.0f * (float)H * (float)W);
        const float sgn = diff > 0.0f ? gs : (diff < 0.0f ? -gs : 0.0f);  // d|x| = sign(x), 0 at 0 and for NaN
        d_direct_unit[c * HW + p] = sgn;
        if (!(t.has_nan || sgn == 0.0f)) {
          // the whole gradient goes to the first tap (row-major) equal to the median (median3x3_bwd_kernel)
          int k = 0;
          bool routed = false;
          for (int dy = -1; dy <= 1 && !routed; dy++)
            for (int dx = -1; dx <= 1; dx++, k++) {
              if (t.v[k] == med) {
                const int yy = y + dy, xx = x + dx;
                if (!(yy < 0 || yy >= H || xx < 0 || xx >= W)) {
                  const size_t q = (size_t)yy * W + xx;
                  float d;
                  lin2srgb(irr[c * HW + q], d);
                  if (d != 0.0f) atomicAdd(d_irr_unit + c * HW + q, sgn * d);
                }
                routed = true;  // a padding tap selected: the gradient is dropped
                break;
              }
            }
        }
      }
    }
    const float m = mask_f[p];
    rs = (1.0f - roughness[p]) * m;
    ms = metallic[p] * m;
    cnt = m;
  }
  l1 = block_sum(l1, s_red);
  rs = block_sum(rs, s_red);
  ms = block_sum(ms, s_red);
  cnt = block_sum(cnt, s_red);
  // Thousands of workgroups adding to the same four floats serialise in L2 (measured: 0.1 ms of a 0.14 ms
  // kernel), so the partial sums are spread over kAccSlots rows and the finish kernel adds the rows up.
  if (threadIdx.x == 0) {
    float* row = acc + 4 * ((blockIdx.y * gridDim.x + blockIdx.x) % kAccSlots);
    atomicAdd(row + 0, l1);
    atomicAdd(row + 1, rs);
    atomicAdd(row + 2, ms);
    atomicAdd(row + 3, cnt);
  }
}

// one wave: column sums of the kAccSlots x 4 partial rows -> acc4 (kept for the backward) and the loss
__global__ void __launch_bounds__(64)
stage2_loss_finish_kernel(int H, int W, const float* __restrict__ rows, float* __restrict__ acc4, float* __restrict__ loss) {
  float v[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int r = threadIdx.x; r < kAccSlots; r += 64)
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] += rows[4 * r + k];
#pragma unroll
  for (int k = 0; k < 4; k++)
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_down(v[k], off);
  if (threadIdx.x == 0) {
    const float n = 3.0f * (float)H * (float)W;
    const float l1 = v[0] / n;
    const float lamb = v[1] / v[3] + v[2] / v[3];
    loss[0] = l1 + lamb * 0.001f;
#pragma unroll
    for (int k = 0; k < 4; k++) acc4[k] = v[k];
  }
}

// ---- loss forward + unit gradients as a gather (gigs_stage2_loss_gather) ---------------------------------------
// stage2_loss_fwd_kernel routes the median's gradient with one global float atomic per pixel and channel, so its
// target plane and its partial-sum rows must be cleared first.  Here a workgroup evaluates the median, the sign and
// the selected tap for its tile AND the 1-pixel ring around it (from lin2srgb(IRR) staged with a 2-pixel halo), keeps
// {selected tap, sign} as one byte per pixel and channel in LDS, and every tile pixel q then collects, in row-major
// order of its <= 9 neighbours p, sgn_p * d_q from the p whose selected tap is q: one plain store per texel, no
// cleared buffer, the same result on every run.  The four sums are formed in double (per lane, per workgroup, and
// over the workgroups' rows in the finish) and rounded to fp32 once: the order of a double sum of fp32 terms shows
// only far below fp32 rounding.
// 64 x 8 pixels per workgroup of 256 lanes (measured: 33.3 us at 800 x 800 against 35.6 for 64 x 4 and 39.6 for 64 x 16)
constexpr int kGatherW = 64, kGatherH = 8;
__global__ void __launch_bounds__(256)
stage2_loss_gather_kernel(int H, int W, const float* __restrict__ direct, const float* __restrict__ irr,
                          const float* __restrict__ gt, const float* __restrict__ mask_f,
                          const float* __restrict__ roughness, const float* __restrict__ metallic,
                          float* __restrict__ render_rgb, double* __restrict__ rows, float* __restrict__ d_direct_unit,
                          float* __restrict__ d_irr_unit) {
  constexpr int TH = kGatherH, SW = kGatherW + 4, SH = TH + 4;  // sRGB tile with its 2-pixel halo
  constexpr int RW = kGatherW + 2, RH = TH + 2;  // tile + 1-pixel ring: the pixels whose selection a tile pixel can receive
  __shared__ float s_t[3][SH][SW];
  __shared__ float s_d[3][TH][kGatherW];  // d lin2srgb / d irr of the tile pixels
  __shared__ uint8_t s_sel[3][RH][RW + 2];  // 0 = selects nothing, else (tap + 1) | (diff < 0 ? 16 : 0)
  __shared__ double s_red[4];
  const size_t HW = (size_t)H * W;
  const int x0 = blockIdx.x * kGatherW, y0 = blockIdx.y * TH;
  for (int i = threadIdx.x; i < 3 * SH * SW; i += 256) {
    const int c = i / (SH * SW), r = i - c * (SH * SW);
    const int ty = r / SW, tx = r - ty * SW;
    const int yy = y0 - 2 + ty, xx = x0 - 2 + tx;
    float v = 0.0f, d = 0.0f;
    if (!(yy < 0 || yy >= H || xx < 0 || xx >= W)) v = lin2srgb(irr[c * HW + (size_t)yy * W + xx], d);
    s_t[c][ty][tx] = v;
    if (ty >= 2 && ty < TH + 2 && tx >= 2 && tx < kGatherW + 2) s_d[c][ty - 2][tx - 2] = d;
  }
  __syncthreads();
  const float gs = 1.0f / (3.0f * (float)H * (float)W);
  double l1 = 0.0, rs = 0.0, ms = 0.0, cnt = 0.0;
  for (int i = threadIdx.x; i < RH * RW; i += 256) {
    const int ry = i / RW, rx = i - ry * RW;
    const int y = y0 - 1 + ry, x = x0 - 1 + rx;
    const bool inside = !(y < 0 || y >= H || x < 0 || x >= W);
    const bool tile = inside && ry >= 1 && ry <= TH && rx >= 1 && rx <= kGatherW;
    const size_t p = inside ? (size_t)y * W + x : 0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      uint8_t code = 0;  // a pixel outside the image has no window
      if (inside) {
        float tap[9], sorted[9];
        bool has_nan = false;
        int k = 0;
#pragma unroll
        for (int dy = 0; dy <= 2; dy++)
#pragma unroll
          for (int dx = 0; dx <= 2; dx++, k++) {
            const float s = s_t[c][ry + dy][rx + dx];
            tap[k] = s; sorted[k] = s;
            has_nan |= s != s;
          }
        const float med = has_nan ? __builtin_nanf("") : median9(sorted);
        const float r = direct[c * HW + p] + med;
        const float diff = r - gt[c * HW + p];
        const float sgn = diff > 0.0f ? gs : (diff < 0.0f ? -gs : 0.0f);  // d|x| = sign(x), 0 at 0 and for NaN
        if (tile) {
          if (render_rgb) render_rgb[c * HW + p] = r;
          d_direct_unit[c * HW + p] = sgn;
          l1 += fabsf(diff);
        }
        if (!(has_nan || sgn == 0.0f)) {
          int sel = -1;
#pragma unroll
          for (int j = 8; j >= 0; j--)
            if (tap[j] == med) sel = j;  // ends on the first match (row-major)
          if (sel >= 0) code = (uint8_t)((sel + 1) | (diff < 0.0f ? 16 : 0));
        }
      }
      s_sel[c][ry][rx] = code;
    }
    if (tile) {
      const float m = mask_f[p];
      rs += (1.0f - roughness[p]) * m;
      ms += metallic[p] * m;
      cnt += m;
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < TH * kGatherW; i += 256) {
    const int ty = i / kGatherW, tx = i - ty * kGatherW;
    const int y = y0 + ty, x = x0 + tx;
    if (y >= H || x >= W) continue;
    const size_t p = (size_t)y * W + x;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float d = s_d[c][ty][tx];
      float acc = 0.0f;
      int j = 0;
#pragma unroll
      for (int dy = 0; dy <= 2; dy++)
#pragma unroll
        for (int dx = 0; dx <= 2; dx++, j++) {
          // neighbour j's tap 8 - j is this pixel; a selected padding tap matches no pixel and drops its gradient
          const int code = s_sel[c][ty + dy][tx + dx];
          if ((code & 15) == 9 - j) acc += __fmul_rn((code & 16) ? -gs : gs, d);  // the atomic's operand, rounded alike
        }
      d_irr_unit[c * HW + p] = d != 0.0f ? acc : 0.0f;
    }
  }
  l1 = block_sum(l1, s_red);
  rs = block_sum(rs, s_red);
  ms = block_sum(ms, s_red);
  cnt = block_sum(cnt, s_red);
  if (threadIdx.x == 0) {
    double* row = rows + 4 * ((size_t)blockIdx.y * gridDim.x + blockIdx.x);
    row[0] = l1; row[1] = rs; row[2] = ms; row[3] = cnt;
  }
}

// one workgroup: column sums of the [n_rows][4] per-workgroup rows in a fixed order -> acc4 (rounded to fp32 once) and
// the loss, stage2_loss_finish_kernel's formula evaluated in double and rounded once
__global__ void __launch_bounds__(256)
stage2_loss_gather_finish_kernel(int H, int W, int n_rows, const double* __restrict__ rows, float* __restrict__ acc4,
                                 float* __restrict__ loss) {
  __shared__ double s_v[4][256];
  double v[4] = {0.0, 0.0, 0.0, 0.0};
  for (int r = threadIdx.x; r < n_rows; r += 256) {
#pragma unroll
    for (int k = 0; k < 4; k++) v[k] += rows[4 * (size_t)r + k];
  }
#pragma unroll
  for (int k = 0; k < 4; k++) s_v[k][threadIdx.x] = v[k];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off)
#pragma unroll
      for (int k = 0; k < 4; k++) s_v[k][threadIdx.x] += s_v[k][threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const double n = 3.0 * (double)H * (double)W;
    const double lamb = s_v[1][0] / s_v[3][0] + s_v[2][0] / s_v[3][0];
    loss[0] = (float)(s_v[0][0] / n + lamb * (double)0.001f);
#pragma unroll
    for (int k = 0; k < 4; k++) acc4[k] = (float)s_v[k][0];
  }
}

__global__ void __launch_bounds__(256)
stage2_loss_bwd_kernel(int H, int W, const float* __restrict__ direct, const float* __restrict__ irr,
                       const float* __restrict__ gt, const float* __restrict__ mask_f, const float* __restrict__ acc,
                       const float* __restrict__ g_loss, float* __restrict__ d_direct, float* __restrict__ d_irr,
                       float* __restrict__ d_roughness, float* __restrict__ d_metallic) {
  __shared__ float s_t[3][kHaloH][kHaloW];
  const int lx = threadIdx.x & 63, ly = threadIdx.x >> 6;
  const int x = blockIdx.x * kTileW + lx;
  const int y = blockIdx.y * kTileH + ly;
  srgb_tile(irr, H, W, s_t);
  if (x >= W || y >= H) return;
  const size_t HW = (size_t)H * W, p = (size_t)y * W + x;
  const float gl = g_loss ? g_loss[0] : 1.0f;
  const float gs = gl / (3.0f * (float)H * (float)W);
#pragma unroll
  for (int c = 0; c < 3; c++) {
    const float* src = irr + c * HW;
    LossTaps t = srgb_taps(s_t[c], ly, lx);
    float sorted[9];
#pragma unroll
    for (int k = 0; k < 9; k++) sorted[k] = t.v[k];
    const float med = t.has_nan ? __builtin_nanf("") : median9(sorted);
    const float diff = direct[c * HW + p] + med - gt[c * HW + p];
    const float s = diff > 0.0f ? gs : (diff < 0.0f ? -gs : 0.0f);  // d|x| = sign(x), 0 at 0 and for NaN
    d_direct[c * HW + p] = s;
    if (t.has_nan || s == 0.0f) continue;
    // the whole gradient goes to the first tap (row-major) equal to the median (median3x3_bwd_kernel)
    int k = 0;
    bool routed = false;
    for (int dy = -1; dy <= 1 && !routed; dy++)
      for (int dx = -1; dx <= 1; dx++, k++) {
        if (t.v[k] == med) {
          const int yy = y + dy, xx = x + dx;
          if (!(yy < 0 || yy >= H || xx < 0 || xx >= W)) {
            const size_t q = (size_t)yy * W + xx;
            float d;
            lin2srgb(src[q], d);
            if (d != 0.0f) atomicAdd(d_irr + c * HW + q, s * d);
          }
          routed = true;  // a padding tap selected: the gradient is dropped
          break;
        }
      }
  }
  const float m = mask_f[p], cnt = acc[3];
  d_roughness[p] = -m / cnt * (0.001f * gl);
  d_metallic[p] = m / cnt * (0.001f * gl);
}

// plain zero-fill (a kernel node rather than a memset node when the caller captures into a hipGraph)
__global__ void __launch_bounds__(256) zero_kernel(float* __restrict__ p, size_t n) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) p[i] = 0.0f;
}
static void launch_zero(float* p, size_t n, hipStream_t s) {
  const unsigned blocks = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(zero_kernel, dim3(blocks), dim3(256), 0, s, p, n);
}
// two buffers, one node (the small one rides along: a node of its own costs ~5 us on the step's critical path)
__global__ void __launch_bounds__(256) zero2_kernel(float* __restrict__ a, size_t na, float* __restrict__ b, size_t nb) {
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < na + nb; i += (size_t)gridDim.x * 256) {
    if (i < na) a[i] = 0.0f;
    else b[i - na] = 0.0f;
  }
}
static void launch_zero2(float* a, size_t na, float* b, size_t nb, hipStream_t s) {
  const size_t n = na + nb;
  const unsigned blocks = (unsigned)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
  hipLaunchKernelGGL(zero2_kernel, dim3(blocks), dim3(256), 0, s, a, na, b, nb);
}

}  // namespace gigs

extern "C" {

int gigs_gbuffer_post(int height, int width, const float* normal_map, const float* out_normal_view,
                      const float* viewmatrix, float* normals_view, uint8_t* normal_mask, float* normal_mask_f,
                      float* out_normal_view_filtered, void* stream) {
  if (height <= 0 || width <= 0 || !normal_map || !out_normal_view || !viewmatrix || !normals_view ||
      !out_normal_view_filtered)
    return gigs_internal_fail(GIGS_ERR_INVALID, "gbuffer_post: bad argument");
  gigs::StageTimer timer(gigs::Stage::kGbufferPost, stream);
  hipLaunchKernelGGL(gigs::gbuffer_post_kernel<false>, dim3((width + 63) / 64, (height + 3) / 4), dim3(256), 0,
                     (hipStream_t)stream, height, width, normal_map, out_normal_view, viewmatrix, normals_view,
                     normal_mask, normal_mask_f, out_normal_view_filtered, gigs::GbufferPad{});
  return gigs_internal_check_launch("gbuffer_post");
}

int gigs_gbuffer_post_pad(int height, int width, const float* normal_map, const float* normal_map_from_depth,
                          const float* opacity_map, const float* out_normal_view, const float* viewmatrix,
                          uint8_t* normal_mask, float* normal_mask_f, float* normal_world, float* normals_view,
                          float* out_normal_view_filtered, float* normal_map_from_depth_out, float* opacity_out,
                          void* stream) {
  if (height <= 0 || width <= 0 || !normal_map || !opacity_map || !out_normal_view || !viewmatrix || !normals_view ||
      !out_normal_view_filtered || (normal_map_from_depth_out && !normal_map_from_depth))
    return gigs_internal_fail(GIGS_ERR_INVALID, "gbuffer_post_pad: bad argument");
  const gigs::GbufferPad pad{opacity_map, normal_map_from_depth, normal_world, normal_map_from_depth_out, opacity_out};
  gigs::StageTimer timer(gigs::Stage::kGbufferPost, stream);
  hipLaunchKernelGGL(gigs::gbuffer_post_kernel<true>, dim3((width + 63) / 64, (height + 3) / 4), dim3(256), 0,
                     (hipStream_t)stream, height, width, normal_map, out_normal_view, viewmatrix, normals_view,
                     normal_mask, normal_mask_f, out_normal_view_filtered, pad);
  return gigs_internal_check_launch("gbuffer_post_pad");
}

int gigs_gbuffer_post_bwd(int height, int width, const float* normal_map, const float* viewmatrix,
                          const float* g_normals_view, float* scratch3, float* g_normal_map, void* stream) {
  if (height <= 0 || width <= 0 || !normal_map || !viewmatrix || !g_normals_view || !scratch3 || !g_normal_map)
    return gigs_internal_fail(GIGS_ERR_INVALID, "gbuffer_post_bwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const size_t HW = (size_t)height * width;
  gigs::StageTimer timer(gigs::Stage::kGbufferPost, stream);
  gigs::launch_zero(scratch3, 3 * HW, s);
  hipLaunchKernelGGL(gigs::gbuffer_post_bwd_scatter_kernel, dim3((width + 63) / 64, (height + 3) / 4), dim3(256), 0, s,
                     height, width, normal_map, viewmatrix, g_normals_view, scratch3);
  hipLaunchKernelGGL(gigs::gbuffer_post_bwd_finish_kernel, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, s, HW,
                     normal_map, scratch3, g_normal_map);
  return gigs_internal_check_launch("gbuffer_post_bwd");
}

int gigs_normalize_mask(int height, int width, const float* in, float* out, uint8_t* mask, void* stream) {
  if (height <= 0 || width <= 0 || !in || !out) return gigs_internal_fail(GIGS_ERR_INVALID, "normalize_mask: bad argument");
  const size_t HW = (size_t)height * width;
  gigs::StageTimer timer(gigs::Stage::kGbufferPost, stream);
  hipLaunchKernelGGL(gigs::normalize_mask_kernel, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, (hipStream_t)stream, HW,
                     in, out, mask);
  return gigs_internal_check_launch("normalize_mask");
}

int gigs_nonzero_mask(int height, int width, const float* in, float* mask, void* stream) {
  if (height <= 0 || width <= 0 || !in || !mask) return gigs_internal_fail(GIGS_ERR_INVALID, "nonzero_mask: bad argument");
  const size_t HW = (size_t)height * width;
  hipLaunchKernelGGL(gigs::nonzero_mask_kernel, dim3((unsigned)((HW + 255) / 256)), dim3(256), 0, (hipStream_t)stream, HW, in, mask);
  return gigs_internal_check_launch("nonzero_mask");
}

int gigs_stage2_loss_fwd(int height, int width, const float* render_direct, const float* irr_linear,
                         const float* gt_image, const float* normal_mask_f, const float* roughness,
                         const float* metallic, float* render_rgb, float* acc4, float* loss, void* stream) {
  if (height <= 0 || width <= 0 || !render_direct || !irr_linear || !gt_image || !normal_mask_f || !roughness ||
      !metallic || !acc4 || !loss)
    return gigs_internal_fail(GIGS_ERR_INVALID, "stage2_loss_fwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  gigs::StageTimer timer(gigs::Stage::kLossFwd, stream);
  float* rows = acc4 + 4;  // [kAccSlots][4] partial sums behind the four totals
  gigs::launch_zero(rows, 4 * gigs::kAccSlots, s);
  hipLaunchKernelGGL(gigs::stage2_loss_fwd_kernel, dim3((width + 63) / 64, (height + 3) / 4), dim3(256), 0, s, height,
                     width, render_direct, irr_linear, gt_image, normal_mask_f, roughness, metallic, render_rgb, rows,
                     (float*)nullptr, (float*)nullptr);
  hipLaunchKernelGGL(gigs::stage2_loss_finish_kernel, dim3(1), dim3(64), 0, s, height, width, rows, acc4, loss);
  return gigs_internal_check_launch("stage2_loss_fwd");
}

int gigs_stage2_loss_fwd_grad(int height, int width, const float* render_direct, const float* irr_linear,
                              const float* gt_image, const float* normal_mask_f, const float* roughness,
                              const float* metallic, float* render_rgb, float* acc4, float* loss,
                              float* d_render_direct_unit, float* d_irr_linear_unit, void* stream) {
  if (height <= 0 || width <= 0 || !render_direct || !irr_linear || !gt_image || !normal_mask_f || !roughness ||
      !metallic || !acc4 || !loss || !d_render_direct_unit || !d_irr_linear_unit)
    return gigs_internal_fail(GIGS_ERR_INVALID, "stage2_loss_fwd_grad: bad argument");
  hipStream_t s = (hipStream_t)stream;
  gigs::StageTimer timer(gigs::Stage::kLossFwd, stream);
  float* rows = acc4 + 4;
  gigs::launch_zero2(rows, 4 * gigs::kAccSlots, d_irr_linear_unit, 3 * (size_t)height * width, s);
  hipLaunchKernelGGL(gigs::stage2_loss_fwd_kernel, dim3((width + 63) / 64, (height + 3) / 4), dim3(256), 0, s, height,
                     width, render_direct, irr_linear, gt_image, normal_mask_f, roughness, metallic, render_rgb, rows,
                     d_render_direct_unit, d_irr_linear_unit);
  hipLaunchKernelGGL(gigs::stage2_loss_finish_kernel, dim3(1), dim3(64), 0, s, height, width, rows, acc4, loss);
  return gigs_internal_check_launch("stage2_loss_fwd_grad");
}

// rows of the gather's scratch: one per workgroup
static size_t stage2_gather_rows(int height, int width) {
  return (size_t)((width + gigs::kGatherW - 1) / gigs::kGatherW) * (size_t)((height + gigs::kGatherH - 1) / gigs::kGatherH);
}

size_t gigs_stage2_loss_gather_scratch_bytes(int height, int width) {
  if (height <= 0 || width <= 0) return 0;
  return stage2_gather_rows(height, width) * 4 * sizeof(double);
}

int gigs_stage2_loss_gather(int height, int width, const float* render_direct, const float* irr_linear,
                            const float* gt_image, const float* normal_mask_f, const float* roughness,
                            const float* metallic, float* render_rgb, float* acc4, float* loss,
                            float* d_render_direct_unit, float* d_irr_linear_unit, void* scratch, size_t scratch_bytes,
                            void* stream) {
  if (height <= 0 || width <= 0 || !render_direct || !irr_linear || !gt_image || !normal_mask_f || !roughness ||
      !metallic || !acc4 || !loss || !d_render_direct_unit || !d_irr_linear_unit || !scratch)
    return gigs_internal_fail(GIGS_ERR_INVALID, "stage2_loss_gather: bad argument");
  if (scratch_bytes < gigs_stage2_loss_gather_scratch_bytes(height, width) || ((uintptr_t)scratch & 15))
    return gigs_internal_fail(GIGS_ERR_INVALID, "stage2_loss_gather: scratch smaller than gigs_stage2_loss_gather_scratch_bytes or not 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  double* rows = (double*)scratch;
  const dim3 grid((width + gigs::kGatherW - 1) / gigs::kGatherW, (height + gigs::kGatherH - 1) / gigs::kGatherH);
  gigs::StageTimer timer(gigs::Stage::kLossFwd, stream);
  hipLaunchKernelGGL(gigs::stage2_loss_gather_kernel, grid, dim3(256), 0, s, height, width, render_direct, irr_linear,
                     gt_image, normal_mask_f, roughness, metallic, render_rgb, rows, d_render_direct_unit,
                     d_irr_linear_unit);
  hipLaunchKernelGGL(gigs::stage2_loss_gather_finish_kernel, dim3(1), dim3(256), 0, s, height, width,
                     (int)(grid.x * grid.y), rows, acc4, loss);
  return gigs_internal_check_launch("stage2_loss_gather");
}

int gigs_stage2_loss_bwd(int height, int width, const float* render_direct, const float* irr_linear,
                         const float* gt_image, const float* normal_mask_f, const float* acc4, const float* g_loss,
                         float* d_render_direct, float* d_irr_linear, float* d_roughness, float* d_metallic,
                         void* stream) {
  if (height <= 0 || width <= 0 || !render_direct || !irr_linear || !gt_image || !normal_mask_f || !acc4 ||
      !d_render_direct || !d_irr_linear || !d_roughness || !d_metallic)
    return gigs_internal_fail(GIGS_ERR_INVALID, "stage2_loss_bwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  gigs::StageTimer timer(gigs::Stage::kLossBwd, stream);
  gigs::launch_zero(d_irr_linear, 3 * (size_t)height * width, s);
  hipLaunchKernelGGL(gigs::stage2_loss_bwd_kernel, dim3((width + 63) / 64, (height + 3) / 4), dim3(256), 0, s, height,
                     width, render_direct, irr_linear, gt_image, normal_mask_f, acc4, g_loss, d_render_direct,
                     d_irr_linear, d_roughness, d_metallic);
  return gigs_internal_check_launch("stage2_loss_bwd");
}

}  // extern "C"
