// ssim.h -- what the training loss (image_loss.hip) and the evaluator (eval_metrics.hip) share of SSIM: the tiling, the
// Gaussian window, the launch geometry and the forward kernel, of which each unit instantiates one form
// (utils/loss_utils.py:42-98).
#pragma once
#include <cmath>

#include "block_reduce.h"

namespace gigs {

constexpr int kSsimTile = 32;                      // outputs per workgroup side
constexpr int kSsimR = 5;                          // window radius: window_size 11 (loss_utils.py:56)
constexpr int kSsimHalo = kSsimTile + 2 * kSsimR;  // 42
struct SsimWindow { float w[2 * kSsimR + 1]; };

// utils/loss_utils.py:72-98 (`_ssim`, zero-padded depthwise conv, C1 = 0.01^2, C2 = 0.03^2) and :19-20 (l1_loss);
// combined as train.py:320.
// kEval (gigs_image_metrics): the same ssim_map, plus the squared error of the channel and the masked squared error
// with its element count, summed in double into four partials per workgroup (eval_d); no L1, no derivative planes.
template <bool kEval>
__global__ void __launch_bounds__(256)
l1_ssim_fwd_kernel(int H, int W, const float* __restrict__ img, const float* __restrict__ gt, SsimWindow win,
                   float* __restrict__ d_mu1, float* __restrict__ d_e11, float* __restrict__ d_e12,
                   float* __restrict__ partials, const uint8_t* __restrict__ mask, double* __restrict__ eval_d) {
  __shared__ float s_x[kSsimHalo][kSsimHalo + 1], s_y[kSsimHalo][kSsimHalo + 1];
  __shared__ float s_h[5][kSsimHalo][kSsimTile + 1];
  __shared__ float s_red[4];
  __shared__ double s_red_d[4];
  double e_ss = 0.0, e_se = 0.0, e_sem = 0.0, e_cnt = 0.0;
  const size_t plane = (size_t)blockIdx.z * H * W;
  const int x0 = blockIdx.x * kSsimTile - kSsimR, y0 = blockIdx.y * kSsimTile - kSsimR;
  {
    // all of a thread's halo loads are issued before the first LDS store: one global-memory latency, not seven
    constexpr int kIters = (kSsimHalo * kSsimHalo + 255) / 256;
    float va[kIters], vb[kIters];
#pragma unroll
    for (int j = 0; j < kIters; j++) {
      const int i = threadIdx.x + 256 * j;
      const int ty = i / kSsimHalo, tx = i - ty * kSsimHalo;
      const int yy = y0 + ty, xx = x0 + tx;
      va[j] = 0.0f;
      vb[j] = 0.0f;
      if (i < kSsimHalo * kSsimHalo && yy >= 0 && yy < H && xx >= 0 && xx < W) {
        const size_t q = plane + (size_t)yy * W + xx;
        va[j] = img[q];
        vb[j] = gt[q];
      }
    }
#pragma unroll
    for (int j = 0; j < kIters; j++) {
      const int i = threadIdx.x + 256 * j;
      const int ty = i / kSsimHalo, tx = i - ty * kSsimHalo;
      if (i < kSsimHalo * kSsimHalo) {
        s_x[ty][tx] = va[j];
        s_y[ty][tx] = vb[j];
      }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kSsimHalo * kSsimTile; i += 256) {
    const int ty = i >> 5, tx = i & 31;
    float a = 0.0f, b = 0.0f, aa = 0.0f, bb = 0.0f, ab = 0.0f;
#pragma unroll
    for (int k = 0; k <= 2 * kSsimR; k++) {
      const float xv = s_x[ty][tx + k], yv = s_y[ty][tx + k], w = win.w[k];
      a += w * xv;
      b += w * yv;
      aa += w * (xv * xv);
      bb += w * (yv * yv);
      ab += w * (xv * yv);
    }
    s_h[0][ty][tx] = a; s_h[1][ty][tx] = b; s_h[2][ty][tx] = aa; s_h[3][ty][tx] = bb; s_h[4][ty][tx] = ab;
  }
  __syncthreads();
  const float C1 = 0.0001f, C2 = 0.0009f;
  float l1 = 0.0f, ss = 0.0f;
  const int tx = threadIdx.x & 31;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int ty = (threadIdx.x >> 5) + 8 * r;
    float mu1 = 0.0f, mu2 = 0.0f, e11 = 0.0f, e22 = 0.0f, e12 = 0.0f;
#pragma unroll
    for (int k = 0; k <= 2 * kSsimR; k++) {
      const float w = win.w[k];
      mu1 += w * s_h[0][ty + k][tx];
      mu2 += w * s_h[1][ty + k][tx];
      e11 += w * s_h[2][ty + k][tx];
      e22 += w * s_h[3][ty + k][tx];
      e12 += w * s_h[4][ty + k][tx];
    }
    const int x = blockIdx.x * kSsimTile + tx, y = blockIdx.y * kSsimTile + ty;
    if (x < W && y < H) {
      const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu1_mu2 = mu1 * mu2;
      const float sigma1_sq = e11 - mu1_sq, sigma2_sq = e22 - mu2_sq, sigma12 = e12 - mu1_mu2;
      const float A = 2.0f * mu1_mu2 + C1, B = 2.0f * sigma12 + C2;
      const float Cc = mu1_sq + mu2_sq + C1, D = sigma1_sq + sigma2_sq + C2;
      const float den = Cc * D;
      const float s = (A * B) / den;
      if (kEval) {
        const double d = (double)s_x[ty + kSsimR][tx + kSsimR] - (double)s_y[ty + kSsimR][tx + kSsimR];
        e_ss += (double)s;
        e_se += d * d;
        if (mask && mask[(size_t)y * W + x]) { e_sem += d * d; e_cnt += 1.0; }
        continue;
      }
      ss += s;
      l1 += fabsf(s_x[ty + kSsimR][tx + kSsimR] - s_y[ty + kSsimR][tx + kSsimR]);
      if (d_mu1) {
        // d ssim / d(mu1, E[x^2], E[xy]) at this window centre; the backward spreads them through the window
        const size_t q = plane + (size_t)y * W + x;
        d_mu1[q] = (2.0f * mu2 * (B - A) - 2.0f * mu1 * s * (D - Cc)) / den;
        d_e11[q] = -s / D;
        d_e12[q] = 2.0f * A / den;
      }
    }
  }
  if (kEval) {
    e_ss = block_sum(e_ss, s_red_d);
    e_se = block_sum(e_se, s_red_d);
    e_sem = block_sum(e_sem, s_red_d);
    e_cnt = block_sum(e_cnt, s_red_d);
    if (threadIdx.x == 0) {
      const size_t b = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
      eval_d[4 * b] = e_ss; eval_d[4 * b + 1] = e_se; eval_d[4 * b + 2] = e_sem; eval_d[4 * b + 3] = e_cnt;
    }
    return;
  }
  l1 = block_sum(l1, s_red);
  ss = block_sum(ss, s_red);
  if (threadIdx.x == 0) {
    const size_t b = ((size_t)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partials[2 * b] = l1;
    partials[2 * b + 1] = ss;
  }
}

static inline SsimWindow make_window() {
  // loss_utils.py:42-46: exp() in double per tap, stored as fp32, divided by the fp32 sum (sigma 1.5)
  SsimWindow w;
  float sum = 0.0f;
  for (int i = 0; i <= 2 * kSsimR; i++) {
    w.w[i] = (float)exp(-(double)((i - kSsimR) * (i - kSsimR)) / (2.0 * 1.5 * 1.5));
    sum += w.w[i];
  }
  for (int i = 0; i <= 2 * kSsimR; i++) w.w[i] /= sum;
  return w;
}

// one workgroup per kSsimTile x kSsimTile outputs of a channel
static inline dim3 ssim_grid(int H, int W, int C) {
  return dim3((W + kSsimTile - 1) / kSsimTile, (H + kSsimTile - 1) / kSsimTile, C);
}
static inline unsigned ssim_blocks(int H, int W) { return ssim_grid(H, W, 1).x * ssim_grid(H, W, 1).y; }  // per channel

}  // namespace gigs
