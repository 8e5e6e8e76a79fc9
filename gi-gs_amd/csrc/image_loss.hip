// image_loss.hip -- SURVEY 8(f) rank 1: the image losses of the training loop.
//
// The reference writes these as chains of torch ops: `ssim` is six depthwise 11x11 conv2d calls plus a dozen
// elementwise kernels (utils/loss_utils.py:55-98), the TV regularisers are ~20 slicing / pow / exp / mean ops each
// (train.py:83-142), and the masked normal loss indexes with a boolean mask (train.py:327).  Here each is one pass:
//
//   l1_ssim_fwd/bwd     (1-l)*mean|x-y| + l*(1-mean(ssim_map)) with a separable window staged through LDS; the
//                       forward (ssim.h, shared with the evaluator) keeps three derivative planes per channel, the
//                       backward is one more separable pass
//   tv_fwd/bwd          get_tv_loss / get_masked_tv_loss: edge-aware squared differences of a [C,H,W] stack
//   masked_l1_fwd/bwd   F.l1_loss(a[:, mask], b[:, mask])
//
// All image planes are [C,H,W] fp32.  Every reduction goes through per-workgroup partial sums that a one-block
// finish kernel adds in a fixed order, so losses are bit-reproducible run to run.  The kernels are HBM-streaming (a few
// planes each).  The three losses share one unit because gigs_loss_scratch_floats sizes one scratch buffer for all.
#include "block_reduce.h"
#include "gigs_internal.h"
#include "ssim.h"

namespace gigs {

// ---- L1 + SSIM (utils/loss_utils.py:19-20, 72-98; train.py:320) -----------------------------------------------
// out = {loss, mean|x-y|, mean ssim}
__global__ void __launch_bounds__(256)
l1_ssim_finish_kernel(const float* __restrict__ partials, int nrows, float count, float lambda, float* __restrict__ out) {
  __shared__ float s_red[4];
  float tot[2];
  reduce_rows<2>(partials, nrows, s_red, tot);
  if (threadIdx.x == 0) {
    const float l1 = tot[0] / count, ssim = tot[1] / count;
    out[0] = (1.0f - lambda) * l1 + lambda * (1.0f - ssim);
    out[1] = l1;
    out[2] = ssim;
  }
}

__global__ void __launch_bounds__(256)
l1_ssim_bwd_kernel(int H, int W, const float* __restrict__ img, const float* __restrict__ gt, SsimWindow win,
                   const float* __restrict__ d_mu1, const float* __restrict__ d_e11, const float* __restrict__ d_e12,
                   const float* __restrict__ g_loss, float l1_scale, float ssim_scale, float* __restrict__ g_img) {
  __shared__ float s_m[3][kSsimHalo][kSsimHalo + 1];
  __shared__ float s_h[3][kSsimHalo][kSsimTile + 1];
  const size_t plane = (size_t)blockIdx.z * H * W;
  const int x0 = blockIdx.x * kSsimTile - kSsimR, y0 = blockIdx.y * kSsimTile - kSsimR;
  {
    constexpr int kIters = (kSsimHalo * kSsimHalo + 255) / 256;
    float va[kIters], vb[kIters], vc[kIters];
#pragma unroll
    for (int j = 0; j < kIters; j++) {
      const int i = threadIdx.x + 256 * j;
      const int ty = i / kSsimHalo, tx = i - ty * kSsimHalo;
      const int yy = y0 + ty, xx = x0 + tx;
      va[j] = vb[j] = vc[j] = 0.0f;
      if (i < kSsimHalo * kSsimHalo && yy >= 0 && yy < H && xx >= 0 && xx < W) {
        const size_t q = plane + (size_t)yy * W + xx;
        va[j] = d_mu1[q];
        vb[j] = d_e11[q];
        vc[j] = d_e12[q];
      }
    }
#pragma unroll
    for (int j = 0; j < kIters; j++) {
      const int i = threadIdx.x + 256 * j;
      const int ty = i / kSsimHalo, tx = i - ty * kSsimHalo;
      if (i < kSsimHalo * kSsimHalo) { s_m[0][ty][tx] = va[j]; s_m[1][ty][tx] = vb[j]; s_m[2][ty][tx] = vc[j]; }
    }
  }
  __syncthreads();
  for (int i = threadIdx.x; i < kSsimHalo * kSsimTile; i += 256) {
    const int ty = i >> 5, tx = i & 31;
    float a = 0.0f, b = 0.0f, c = 0.0f;
#pragma unroll
    for (int k = 0; k <= 2 * kSsimR; k++) {
      const float w = win.w[k];
      a += w * s_m[0][ty][tx + k];
      b += w * s_m[1][ty][tx + k];
      c += w * s_m[2][ty][tx + k];
    }
    s_h[0][ty][tx] = a; s_h[1][ty][tx] = b; s_h[2][ty][tx] = c;
  }
  __syncthreads();
  const float g = g_loss ? *g_loss : 1.0f;
  const int tx = threadIdx.x & 31;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int ty = (threadIdx.x >> 5) + 8 * r;
    const int x = blockIdx.x * kSsimTile + tx, y = blockIdx.y * kSsimTile + ty;
    if (x >= W || y >= H) continue;
    float a = 0.0f, b = 0.0f, c = 0.0f;
#pragma unroll
    for (int k = 0; k <= 2 * kSsimR; k++) {
      const float w = win.w[k];
      a += w * s_h[0][ty + k][tx];
      b += w * s_h[1][ty + k][tx];
      c += w * s_h[2][ty + k][tx];
    }
    const size_t q = plane + (size_t)y * W + x;
    const float xv = img[q], yv = gt[q];
    const float d = xv - yv;
    const float sgn = d > 0.0f ? 1.0f : (d < 0.0f ? -1.0f : 0.0f);  // torch's abs backward: sgn(0) = 0
    g_img[q] = g * (l1_scale * sgn + ssim_scale * (a + 2.0f * xv * b + yv * c));
  }
}

// ---- edge-aware TV (train.py:83-142) --------------------------------------------------------------------------
// weight of the (p, p+s) pair along one axis: exp(-mean_c |gt(p+s) - gt(p)|) [* mask(p+s) * mask(p)]
__device__ __forceinline__ float tv_weight(const float* __restrict__ gt, const float* __restrict__ mask, size_t HW,
                                           size_t p, size_t q) {
  float w = 1.0f;  // no guide image: the plain TV of train.py:419-421
  if (gt) {
    const float d = fabsf(gt[q] - gt[p]) + fabsf(gt[HW + q] - gt[HW + p]) + fabsf(gt[2 * HW + q] - gt[2 * HW + p]);
    w = expf(-(d / 3.0f));
  }
  if (mask) w *= mask[q] * mask[p];
  return w;
}

// both TV kernels: a workgroup covers 64 x 4 pixels, one per thread
static inline dim3 tv_grid(int H, int W) { return dim3((W + 63) / 64, (H + 3) / 4); }

__global__ void __launch_bounds__(256)
tv_fwd_kernel(int C, int H, int W, int step, const float* __restrict__ gt, const float* __restrict__ pred,
              const float* __restrict__ mask, float* __restrict__ partials) {
  __shared__ float s_red[4];
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  const size_t HW = (size_t)H * W;
  float acc = 0.0f;
  if (x < W && y < H) {
    const size_t p = (size_t)y * W + x;
    for (int s = 1; s <= step; s++) {
      if (y + s < H) {
        const size_t q = p + (size_t)s * W;
        float t = 0.0f;
        for (int c = 0; c < C; c++) {
          const float d = pred[c * HW + q] - pred[c * HW + p];
          t += d * d;
        }
        acc += t * tv_weight(gt, mask, HW, p, q) / ((float)C * (float)(H - s) * (float)W);
      }
      if (x + s < W) {
        const size_t q = p + s;
        float t = 0.0f;
        for (int c = 0; c < C; c++) {
          const float d = pred[c * HW + q] - pred[c * HW + p];
          t += d * d;
        }
        acc += t * tv_weight(gt, mask, HW, p, q) / ((float)C * (float)H * (float)(W - s));
      }
    }
  }
  acc = block_sum(acc, s_red);
  if (threadIdx.x == 0) partials[blockIdx.y * gridDim.x + blockIdx.x] = acc;
}

__global__ void __launch_bounds__(256)
sum_finish_kernel(const float* __restrict__ partials, int nrows, float* __restrict__ out) {
  __shared__ float s_red[4];
  float tot[1];
  reduce_rows<1>(partials, nrows, s_red, tot);
  if (threadIdx.x == 0) out[0] = tot[0];
}

__global__ void __launch_bounds__(256)
tv_bwd_kernel(int C, int H, int W, int step, const float* __restrict__ gt, const float* __restrict__ pred,
              const float* __restrict__ mask, const float* __restrict__ g_loss, float* __restrict__ g_pred) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  const size_t HW = (size_t)H * W;
  const size_t p = (size_t)y * W + x;
  const float g = 2.0f * (g_loss ? *g_loss : 1.0f);
  // the four neighbours' pair weights per offset s, then one pass over the channels
  for (int c = 0; c < C; c++) g_pred[c * HW + p] = 0.0f;
  for (int s = 1; s <= step; s++) {
    const float nh = g / ((float)C * (float)(H - s) * (float)W), nw = g / ((float)C * (float)H * (float)(W - s));
    const bool dn = y + s < H, up = y - s >= 0, rt = x + s < W, lf = x - s >= 0;
    const size_t qd = p + (size_t)s * W, qu = p - (size_t)s * W, qr = p + s, ql = p - s;
    const float wd = dn ? nh * tv_weight(gt, mask, HW, p, qd) : 0.0f;
    const float wu = up ? nh * tv_weight(gt, mask, HW, qu, p) : 0.0f;
    const float wr = rt ? nw * tv_weight(gt, mask, HW, p, qr) : 0.0f;
    const float wl = lf ? nw * tv_weight(gt, mask, HW, ql, p) : 0.0f;
    for (int c = 0; c < C; c++) {
      const float* pc = pred + c * HW;
      const float v = pc[p];
      float a = 0.0f;
      if (dn) a -= wd * (pc[qd] - v);
      if (up) a += wu * (v - pc[qu]);
      if (rt) a -= wr * (pc[qr] - v);
      if (lf) a += wl * (v - pc[ql]);
      g_pred[c * HW + p] += a;
    }
  }
}

// ---- masked L1 (train.py:327: F.l1_loss(normal_map[:, mask], normal_map_from_depth[:, mask])) -----------------
static inline unsigned stream_blocks(size_t HW) {  // grid-stride kernels over the pixels
  const size_t b = (HW + 255) / 256;
  return (unsigned)(b < 2048 ? b : 2048);
}

__global__ void __launch_bounds__(256)
masked_l1_fwd_kernel(int C, size_t HW, const float* __restrict__ a, const float* __restrict__ b,
                     const uint8_t* __restrict__ mask, float* __restrict__ partials) {
  __shared__ float s_red[4];
  float sum = 0.0f, cnt = 0.0f;
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < HW; p += (size_t)gridDim.x * 256) {
    if (!mask[p]) continue;
    cnt += 1.0f;
    for (int c = 0; c < C; c++) sum += fabsf(a[c * HW + p] - b[c * HW + p]);
  }
  sum = block_sum(sum, s_red);
  cnt = block_sum(cnt, s_red);
  if (threadIdx.x == 0) {
    partials[2 * blockIdx.x] = sum;
    partials[2 * blockIdx.x + 1] = cnt;
  }
}

// out = {loss, count}; an empty mask gives 0/0 = NaN like torch's mean of an empty tensor
__global__ void __launch_bounds__(256)
masked_l1_finish_kernel(const float* __restrict__ partials, int nrows, int C, float* __restrict__ out) {
  __shared__ float s_red[4];
  float tot[2];
  reduce_rows<2>(partials, nrows, s_red, tot);
  if (threadIdx.x == 0) {
    out[0] = tot[0] / ((float)C * tot[1]);
    out[1] = tot[1];
  }
}

__global__ void __launch_bounds__(256)
masked_l1_bwd_kernel(int C, size_t HW, const float* __restrict__ a, const float* __restrict__ b,
                     const uint8_t* __restrict__ mask, const float* __restrict__ loss_count,
                     const float* __restrict__ g_loss, float* __restrict__ g_a, float* __restrict__ g_b) {
  const float g = (g_loss ? *g_loss : 1.0f) / ((float)C * loss_count[1]);
  for (size_t p = (size_t)blockIdx.x * 256 + threadIdx.x; p < HW; p += (size_t)gridDim.x * 256) {
    const bool m = mask[p] != 0;
    for (int c = 0; c < C; c++) {
      float v = 0.0f;
      if (m) {
        const float d = a[c * HW + p] - b[c * HW + p];
        v = d > 0.0f ? g : (d < 0.0f ? -g : 0.0f);
      }
      if (g_a) g_a[c * HW + p] = v;
      if (g_b) g_b[c * HW + p] = -v;
    }
  }
}

}  // namespace gigs

extern "C" {

size_t gigs_loss_scratch_floats(int channels, int height, int width) {
  if (channels <= 0 || height <= 0 || width <= 0) return 0;
  const dim3 tvg = gigs::tv_grid(height, width);
  const size_t ssim = 2 * (size_t)channels * gigs::ssim_blocks(height, width);
  const size_t tv = (size_t)tvg.x * tvg.y;
  const size_t ml1 = 2 * (size_t)gigs::stream_blocks((size_t)height * width);
  size_t m = ssim > tv ? ssim : tv;
  if (ml1 > m) m = ml1;
  return m + 8;
}

int gigs_l1_ssim_fwd(int channels, int height, int width, const float* image, const float* gt, float lambda_dssim,
                     float* d_mu1, float* d_e11, float* d_e12, float* scratch, float* out3, void* stream) {
  if (channels <= 0 || height <= 0 || width <= 0 || !image || !gt || !scratch || !out3 ||
      ((d_mu1 != nullptr) != (d_e11 != nullptr)) || ((d_mu1 != nullptr) != (d_e12 != nullptr)))
    return gigs_internal_fail(GIGS_ERR_INVALID, "l1_ssim_fwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  gigs::StageTimer timer(gigs::Stage::kL1SsimFwd, stream);
  const dim3 grid = gigs::ssim_grid(height, width, channels);
  hipLaunchKernelGGL(gigs::l1_ssim_fwd_kernel<false>, grid, dim3(256), 0, s, height, width, image, gt,
                     gigs::make_window(), d_mu1, d_e11, d_e12, scratch, nullptr, nullptr);
  hipLaunchKernelGGL(gigs::l1_ssim_finish_kernel, dim3(1), dim3(256), 0, s, scratch, (int)(grid.x * grid.y * grid.z),
                     (float)channels * (float)height * (float)width, lambda_dssim, out3);
  return gigs_internal_check_launch("l1_ssim_fwd");
}

int gigs_l1_ssim_bwd(int channels, int height, int width, const float* image, const float* gt, float lambda_dssim,
                     const float* d_mu1, const float* d_e11, const float* d_e12, const float* g_loss, float* g_image,
                     void* stream) {
  if (channels <= 0 || height <= 0 || width <= 0 || !image || !gt || !d_mu1 || !d_e11 || !d_e12 || !g_image)
    return gigs_internal_fail(GIGS_ERR_INVALID, "l1_ssim_bwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  gigs::StageTimer timer(gigs::Stage::kL1SsimBwd, stream);
  const float count = (float)channels * (float)height * (float)width;
  hipLaunchKernelGGL(gigs::l1_ssim_bwd_kernel, gigs::ssim_grid(height, width, channels), dim3(256), 0, s, height, width,
                     image, gt, gigs::make_window(), d_mu1, d_e11, d_e12, g_loss, (1.0f - lambda_dssim) / count,
                     -lambda_dssim / count, g_image);
  return gigs_internal_check_launch("l1_ssim_bwd");
}

int gigs_tv_loss_fwd(int channels, int height, int width, int step, const float* gt, const float* prediction,
                     const float* mask_f, float* scratch, float* loss, void* stream) {
  if (channels <= 0 || height <= 0 || width <= 0 || step < 1 || step >= height || step >= width ||
      !prediction || !scratch || !loss)
    return gigs_internal_fail(GIGS_ERR_INVALID, "tv_loss_fwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  gigs::StageTimer timer(gigs::Stage::kTvFwd, stream);
  const dim3 grid = gigs::tv_grid(height, width);
  hipLaunchKernelGGL(gigs::tv_fwd_kernel, grid, dim3(256), 0, s, channels, height, width, step, gt, prediction,
                     mask_f, scratch);
  hipLaunchKernelGGL(gigs::sum_finish_kernel, dim3(1), dim3(256), 0, s, scratch, (int)(grid.x * grid.y), loss);
  return gigs_internal_check_launch("tv_loss_fwd");
}

int gigs_tv_loss_bwd(int channels, int height, int width, int step, const float* gt, const float* prediction,
                     const float* mask_f, const float* g_loss, float* g_prediction, void* stream) {
  if (channels <= 0 || height <= 0 || width <= 0 || step < 1 || step >= height || step >= width ||
      !prediction || !g_prediction)
    return gigs_internal_fail(GIGS_ERR_INVALID, "tv_loss_bwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  gigs::StageTimer timer(gigs::Stage::kTvBwd, stream);
  hipLaunchKernelGGL(gigs::tv_bwd_kernel, gigs::tv_grid(height, width), dim3(256), 0, s, channels, height, width, step,
                     gt, prediction, mask_f, g_loss, g_prediction);
  return gigs_internal_check_launch("tv_loss_bwd");
}

int gigs_masked_l1_fwd(int channels, int height, int width, const float* a, const float* b, const uint8_t* mask,
                       float* scratch, float* loss_count, void* stream) {
  if (channels <= 0 || height <= 0 || width <= 0 || !a || !b || !mask || !scratch || !loss_count)
    return gigs_internal_fail(GIGS_ERR_INVALID, "masked_l1_fwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  gigs::StageTimer timer(gigs::Stage::kMaskedL1, stream);
  const size_t HW = (size_t)height * width;
  const unsigned blocks = gigs::stream_blocks(HW);
  hipLaunchKernelGGL(gigs::masked_l1_fwd_kernel, dim3(blocks), dim3(256), 0, s, channels, HW, a, b, mask, scratch);
  hipLaunchKernelGGL(gigs::masked_l1_finish_kernel, dim3(1), dim3(256), 0, s, scratch, (int)blocks, channels,
                     loss_count);
  return gigs_internal_check_launch("masked_l1_fwd");
}

int gigs_masked_l1_bwd(int channels, int height, int width, const float* a, const float* b, const uint8_t* mask,
                       const float* loss_count, const float* g_loss, float* g_a, float* g_b, void* stream) {
  if (channels <= 0 || height <= 0 || width <= 0 || !a || !b || !mask || !loss_count || (!g_a && !g_b))
    return gigs_internal_fail(GIGS_ERR_INVALID, "masked_l1_bwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  gigs::StageTimer timer(gigs::Stage::kMaskedL1, stream);
  const size_t HW = (size_t)height * width;
  hipLaunchKernelGGL(gigs::masked_l1_bwd_kernel, dim3(gigs::stream_blocks(HW)), dim3(256), 0, s, channels, HW, a, b,
                     mask, loss_count, g_loss, g_a, g_b);
  return gigs_internal_check_launch("masked_l1_bwd");
}

}  // extern "C"
