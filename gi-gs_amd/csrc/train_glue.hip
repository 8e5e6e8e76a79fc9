// train_glue.hip -- SURVEY 8(f) rank 1: the image losses of the training loop and the Adam step.
//
// The reference writes these as chains of torch ops: `ssim` is six depthwise 11x11 conv2d calls plus a dozen
// elementwise kernels (utils/loss_utils.py:55-98), the TV regularisers are ~20 slicing / pow / exp / mean ops each
// (train.py:83-142), the masked normal loss indexes with a boolean mask (train.py:327), and Adam runs once per
// parameter group over ten groups (scene/gaussian_model.py:325-346).  Here each is one pass:
//
//   l1_ssim_fwd/bwd     (1-l)*mean|x-y| + l*(1-mean(ssim_map)) with a separable window staged through LDS; the
//                       forward keeps three derivative planes per channel, the backward is one more separable pass
//   tv_fwd/bwd          get_tv_loss / get_masked_tv_loss: edge-aware squared differences of a [C,H,W] stack
//   masked_l1_fwd/bwd   F.l1_loss(a[:, mask], b[:, mask])
//   adam_step           torch.optim.Adam's update for up to 16 parameter groups in one launch
//
// All image planes are [C,H,W] fp32.  Every reduction goes through per-workgroup partial sums that a one-block
// finish kernel adds in a fixed order, so losses are bit-reproducible run to run.  The kernels are HBM-streaming
// (Adam: 28 B per parameter; the losses: a few planes each); none of them is GEMM-shaped.
#include <cmath>
#include <cstring>

#include "gigs_internal.h"

namespace gigs {

constexpr int kSsimTile = 32;                      // outputs per workgroup side
constexpr int kSsimR = 5;                          // window radius: window_size 11 (loss_utils.py:56)
constexpr int kSsimHalo = kSsimTile + 2 * kSsimR;  // 42
struct SsimWindow { float w[2 * kSsimR + 1]; };

// valid in every thread
template <typename T>
__device__ __forceinline__ T block_sum(T v, T* s_red) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = v;
  __syncthreads();
  return s_red[0] + s_red[1] + s_red[2] + s_red[3];
}

// One block: out[c] = sum over rows of partials[row * ncols + c], rows added in a fixed order.
template <int kCols>
__device__ __forceinline__ void reduce_rows(const float* __restrict__ partials, int nrows, float* s_cols, float* tot) {
  float acc[kCols];
#pragma unroll
  for (int c = 0; c < kCols; c++) acc[c] = 0.0f;
  for (int r = threadIdx.x; r < nrows; r += 256)
#pragma unroll
    for (int c = 0; c < kCols; c++) acc[c] += partials[(size_t)r * kCols + c];
#pragma unroll
  for (int c = 0; c < kCols; c++) tot[c] = block_sum(acc[c], s_cols);
}

// ---- L1 + SSIM ------------------------------------------------------------------------------------------------
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

// ---- per-view evaluation metrics (render.py:115-395 NVS, :596-631 albedo, normal_eval.py) -------------------------------
// The record of one view goes to out + stride * (*slot) and *slot is incremented (slot == NULL: to out), so a replayed
// graph fills successive records with no host synchronisation.  All sums are doubles added in a fixed order.
__device__ __forceinline__ double* record_at(double* out, int* slot, int stride) {
  return slot ? out + (size_t)stride * (size_t)(*slot) : out;
}

// record {mse_0 .. mse_{C-1}, mean_c psnr_c, mean ssim, masked mse, masked element count}; rows = workgroups per channel
__global__ void __launch_bounds__(256)
image_metrics_finish_kernel(const double* __restrict__ part, int C, int rows, double npix, int* slot,
                            double* __restrict__ out) {
  __shared__ double s_red[4];
  double* rec = record_at(out, slot, C + 4);
  double psnr = 0.0, ss = 0.0, sem = 0.0, cnt = 0.0;
  for (int c = 0; c < C; c++) {
    double a = 0.0, b = 0.0, m = 0.0, n = 0.0;
    for (int r = threadIdx.x; r < rows; r += 256) {
      const double* q = part + 4 * ((size_t)c * rows + r);
      a += q[0]; b += q[1]; m += q[2]; n += q[3];
    }
    a = block_sum(a, s_red);
    b = block_sum(b, s_red);
    m = block_sum(m, s_red);
    n = block_sum(n, s_red);
    const double mse = b / npix;
    ss += a; sem += m; cnt += n;
    psnr += 20.0 * log10(1.0 / sqrt(mse));  // utils/image_utils.py:31-33
    if (threadIdx.x == 0) rec[c] = mse;
  }
  if (threadIdx.x == 0) {
    rec[C] = psnr / C;
    rec[C + 1] = ss / (npix * C);
    rec[C + 2] = sem / cnt;  // ((a - b) ** 2)[mask].mean(): NaN for an empty mask, as torch's mean of nothing
    rec[C + 3] = cnt;
    if (slot) *slot += 1;
  }
}

// normal_eval.py:11-18 (get_mae) on what render.py saves and normal_eval.py reads back, per pixel in double:
//   gt   = (rgba[:3] / 255 - 0.5) * 2 blended with a = rgba[-1] / 255 over (0, 0, 1), then normalised;
//   pred = the saved plane as torchvision's save_image rounds it (uint8(clamp(x * 255 + 0.5, 0, 255)) in fp32),
//          / 255, (x - 0.5) * 2, (128, 128, 255) -> (0, 0, 1), then normalised;
//   sum of arccos(clip(<gt, pred>, -1, 1)) * 180 / pi and the pixel count.  A zero vector normalises to NaN, as numpy.
__device__ __forceinline__ unsigned png8(float x) {
  float v = x * 255.0f + 0.5f;
  v = v < 0.0f ? 0.0f : (v > 255.0f ? 255.0f : v);
  return v == v ? (unsigned)v : 0u;
}

__global__ void __launch_bounds__(256)
normal_angular_error_kernel(int HW, const float* __restrict__ pred, const uint8_t* __restrict__ gt, int gt_channels,
                            double* __restrict__ part) {
  __shared__ double s_red[4];
  double acc = 0.0;
  for (int p = blockIdx.x * 256 + threadIdx.x; p < HW; p += gridDim.x * 256) {
    const uint8_t* g = gt + (size_t)p * gt_channels;
    const double a = g[gt_channels - 1] / 255.0;
    double n[3];
    for (int c = 0; c < 3; c++) {
      const double bg = c == 2 ? 1.0 : 0.0;
      n[c] = (g[c] / 255.0 - 0.5) * 2.0 * a + bg * (1.0 - a);
    }
    const double ng = sqrt(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
    unsigned u[3];
    for (int c = 0; c < 3; c++) u[c] = png8(pred[(size_t)c * HW + p]);
    double m[3];
    if (u[0] == 128u && u[1] == 128u && u[2] == 255u) {
      m[0] = 0.0; m[1] = 0.0; m[2] = 1.0;
    } else {
      for (int c = 0; c < 3; c++) m[c] = (u[c] / 255.0 - 0.5) * 2.0;
    }
    const double nm = sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
    double d = (n[0] / ng) * (m[0] / nm) + (n[1] / ng) * (m[1] / nm);
    d = d + (n[2] / ng) * (m[2] / nm);
    d = d < -1.0 ? -1.0 : (d > 1.0 ? 1.0 : d);  // keeps NaN, as np.clip
    acc += acos(d) * 180.0 / 3.141592653589793;
  }
  acc = block_sum(acc, s_red);
  if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

// record {sum of angles in degrees, pixel count}
__global__ void __launch_bounds__(256)
normal_angular_error_finish_kernel(const double* __restrict__ part, int rows, double npix, int* slot,
                                   double* __restrict__ out) {
  __shared__ double s_red[4];
  double* rec = record_at(out, slot, 2);
  double a = 0.0;
  for (int r = threadIdx.x; r < rows; r += 256) a += part[r];
  a = block_sum(a, s_red);
  if (threadIdx.x == 0) {
    rec[0] = a;
    rec[1] = npix;
    if (slot) *slot += 1;
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

// ---- Adam (torch.optim.Adam as configured at scene/gaussian_model.py:346: betas (0.9, 0.999), eps 1e-15,
// no weight decay, no amsgrad) --------------------------------------------------------------------------------
constexpr int kAdamMaxGroups = 16;
constexpr int kAdamChunk = 2048;  // elements per workgroup: 256 lanes x 2 x float4
struct AdamGroups {
  float* param[kAdamMaxGroups];
  float* grad[kAdamMaxGroups];
  float* exp_avg[kAdamMaxGroups];
  float* exp_avg_sq[kAdamMaxGroups];
  long long n[kAdamMaxGroups];
  unsigned first_chunk[kAdamMaxGroups + 1];
  float step_size[kAdamMaxGroups];      // lr / (1 - beta1^t)
  float bc2_sqrt[kAdamMaxGroups];       // sqrt(1 - beta2^t)
  int count;
  // hipGraph-capturable form: the two per-step scalars of group k are read from device memory, dyn[2 * (dyn_base + k)]
  // = {step_size, bc2_sqrt}, which the host refreshes before every replay (NULL: the by-value members above)
  const float* dyn;
  int dyn_base;
  // gigs_adam_step_watch: bit k set = group k of this launch is watched; *changed |= 1 when one of its parameters changes
  unsigned watch_mask;
  unsigned* changed;
  // gigs_adam_step_guarded: the launch is a no-op while *guard != 0 (a violated gradient declaration: gigs_ctx_set_materials_only)
  const unsigned* guard;
};

struct AdamConsts { float b2, omb1, omb2, eps; };  // beta2, 1 - beta1, 1 - beta2 (rounded from double as torch does), eps
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamConsts& k,
                                         float step_size, float bc2_sqrt) {
  const float eps = k.eps;
  m = m + k.omb1 * (g - m);                 // exp_avg.lerp_(grad, 1 - beta1)
  v = v * k.b2 + k.omb2 * (g * g);          // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  p = p - step_size * (m / denom);          // param.addcdiv_(exp_avg, denom, value=-step_size)
}

typedef float adam_f4 __attribute__((ext_vector_type(4)));
// kStream: the three arrays a step reads and rewrites are touched once per step and are far larger than any cache: loads
// and stores carry the non-temporal hint (they do not displace what the next kernels of the iteration will read)
template <bool kStream>
__device__ __forceinline__ float4 adam_ld4(const float* p) {
  if constexpr (kStream) {
    const adam_f4 v = __builtin_nontemporal_load(reinterpret_cast<const adam_f4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
  } else {
    return *reinterpret_cast<const float4*>(p);
  }
}
template <bool kStream>
__device__ __forceinline__ void adam_st4(float* p, float4 v) {
  if constexpr (kStream) {
    adam_f4 w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<adam_f4*>(p));
  } else {
    *reinterpret_cast<float4*>(p) = v;
  }
}

template <bool kStream>
__global__ void __launch_bounds__(256)
adam_kernel(AdamGroups G, AdamConsts K, int zero_grad) {
  if (G.guard && *G.guard != 0u) return;  // uniform: nothing of this update is computed from gradients that were declared wrongly
  int gi = 0;
  while (gi + 1 < G.count && blockIdx.x >= G.first_chunk[gi + 1]) gi++;
  const long long n = G.n[gi];
  const long long base = (long long)(blockIdx.x - G.first_chunk[gi]) * kAdamChunk;
  float* __restrict__ P = G.param[gi];
  float* __restrict__ Gr = G.grad[gi];
  float* __restrict__ M = G.exp_avg[gi];
  float* __restrict__ V = G.exp_avg_sq[gi];
  const float ss = G.dyn ? G.dyn[2 * (G.dyn_base + gi)] : G.step_size[gi];
  const float bs = G.dyn ? G.dyn[2 * (G.dyn_base + gi) + 1] : G.bc2_sqrt[gi];
  // Gr == NULL: the group's gradient is an exact zero the caller did not materialise -- the same arithmetic with g = 0
  const bool vec = ((((uintptr_t)P | (uintptr_t)Gr | (uintptr_t)M | (uintptr_t)V) & 15) == 0) && base + kAdamChunk <= n;
  const bool watched = (G.watch_mask >> gi) & 1u;
  bool moved = false;
  if (vec) {
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const long long i = base + (long long)(r * 256 + threadIdx.x) * 4;
      float4 p = adam_ld4<kStream>(P + i), m = adam_ld4<kStream>(M + i);
      float4 v = adam_ld4<kStream>(V + i);
      const float4 g = Gr ? *reinterpret_cast<const float4*>(Gr + i) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      const float4 p0 = p;
      adam_one(p.x, g.x, m.x, v.x, K, ss, bs);
      adam_one(p.y, g.y, m.y, v.y, K, ss, bs);
      adam_one(p.z, g.z, m.z, v.z, K, ss, bs);
      adam_one(p.w, g.w, m.w, v.w, K, ss, bs);
      moved |= (__float_as_uint(p.x) != __float_as_uint(p0.x)) | (__float_as_uint(p.y) != __float_as_uint(p0.y)) |
               (__float_as_uint(p.z) != __float_as_uint(p0.z)) | (__float_as_uint(p.w) != __float_as_uint(p0.w));
      adam_st4<kStream>(P + i, p);
      adam_st4<kStream>(M + i, m);
      adam_st4<kStream>(V + i, v);
      if (zero_grad && Gr) *reinterpret_cast<float4*>(Gr + i) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
  } else {
    for (int r = 0; r < kAdamChunk / 256; r++) {
      const long long i = base + r * 256 + threadIdx.x;
      if (i >= n) break;
      float p = P[i], m = M[i], v = V[i];
      const float p0 = p;
      adam_one(p, Gr ? Gr[i] : 0.0f, m, v, K, ss, bs);
      moved |= __float_as_uint(p) != __float_as_uint(p0);
      P[i] = p; M[i] = m; V[i] = v;
      if (zero_grad && Gr) Gr[i] = 0.0f;
    }
  }
  // frozen geometry: no wave of a watched group sees a change, no atomic is issued
  if (watched && G.changed && __any(moved) && (threadIdx.x & 63) == 0) atomicOr(G.changed, 1u);
}

// ---- parameter activations (scene/gaussian_model.py:48-58, 178-263) ------------------------------------------
// get_features = cat(f_dc, f_rest), get_opacity / albedo / roughness / metallic = sigmoid, get_scaling = exp,
// get_rotation / get_normal = F.normalize(dim=-1, eps=1e-12): eight getters, ~10 torch kernels forward and ~20 backward
// per iteration; here one launch each way (the SH concatenation in 64-Gaussian tiles, then the sixteen small attributes
// one Gaussian per lane).
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

// ---- densification bookkeeping ----------------------------------------------------------
// train.py:494-498 + GaussianModel.add_densification_stats (scene/gaussian_model.py:933-945) for the Gaussians with
// radii > 0, one pass instead of ~20 masked torch ops per iteration:
//   max_radii2D = max(max_radii2D, radii);  accum += |(gx, gy)|;  accum_abs += |gx| + |gy|;
//   accum_abs_max = max(accum_abs_max, |gx| + |gy|);  denom += 1
__global__ void __launch_bounds__(256)
densify_stats_kernel(int P, const float* __restrict__ grad2d, const int* __restrict__ radii, float* __restrict__ accum,
                     float* __restrict__ accum_abs, float* __restrict__ accum_abs_max, float* __restrict__ denom,
                     float* __restrict__ max_radii2D, const int* __restrict__ skip) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= P) return;
  if (skip && *skip != 0) return;  // guarded form: a captured forward whose binning overflowed adds nothing
  const int r = radii[i];
  if (r <= 0) return;
  const float gx = grad2d[3 * (size_t)i], gy = grad2d[3 * (size_t)i + 1];
  const float a = fabsf(gx) + fabsf(gy);
  max_radii2D[i] = fmaxf(max_radii2D[i], (float)r);
  accum[i] += sqrtf(gx * gx + gy * gy);
  accum_abs[i] += a;
  accum_abs_max[i] = fmaxf(accum_abs_max[i], a);
  denom[i] += 1.0f;
}

// Row gather over many tensors at once: dst_t[r, :] = zero_row[r] && t.zero_new ? 0 : src_t[src_index[r], :].
// One launch rebuilds every parameter and optimizer-state tensor after a densify / prune decision
// (the reference: ~30 boolean-mask index ops and cats, scene/gaussian_model.py:595-706).
constexpr int kGatherMaxTensors = 32;
constexpr int kGatherChunk = 1024;
struct GatherTable {
  const float* src[kGatherMaxTensors];
  float* dst[kGatherMaxTensors];
  int row_floats[kGatherMaxTensors];
  int zero_new[kGatherMaxTensors];
  unsigned first_chunk[kGatherMaxTensors + 1];
  int count;
};
__global__ void __launch_bounds__(256)
gather_rows_kernel(GatherTable T, long long n_rows, const int* __restrict__ src_index,
                   const uint8_t* __restrict__ zero_row) {
  int t = 0;
  while (t + 1 < T.count && blockIdx.x >= T.first_chunk[t + 1]) t++;
  const int rf = T.row_floats[t];
  const long long total = n_rows * rf;
  const long long base = (long long)(blockIdx.x - T.first_chunk[t]) * kGatherChunk;
  const float* __restrict__ src = T.src[t];
  float* __restrict__ dst = T.dst[t];
  const bool zn = T.zero_new[t] != 0 && zero_row != nullptr;
#pragma unroll
  for (int k = 0; k < kGatherChunk / 256; k++) {
    const long long e = base + k * 256 + threadIdx.x;
    if (e >= total) break;
    const long long r = e / rf;
    const int c = (int)(e - r * rf);
    float v = 0.0f;
    if (!(zn && zero_row[r])) v = src[(long long)src_index[r] * rf + c];
    dst[e] = v;
  }
}

static SsimWindow make_window() {
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

static inline unsigned ssim_blocks(int H, int W) {
  return (unsigned)(((H + kSsimTile - 1) / kSsimTile) * ((W + kSsimTile - 1) / kSsimTile));
}
static inline unsigned mae_blocks(size_t HW) {
  const size_t b = (HW + 255) / 256;
  return (unsigned)(b < 1024 ? b : 1024);
}
static inline unsigned stream_blocks(size_t HW) {
  const size_t b = (HW + 255) / 256;
  return (unsigned)(b < 2048 ? b : 2048);
}

}  // namespace gigs

extern "C" {

size_t gigs_loss_scratch_floats(int channels, int height, int width) {
  if (channels <= 0 || height <= 0 || width <= 0) return 0;
  const size_t ssim = 2 * (size_t)channels * gigs::ssim_blocks(height, width);
  const size_t tv = (size_t)((width + 63) / 64) * ((height + 3) / 4);
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
  const dim3 grid((width + gigs::kSsimTile - 1) / gigs::kSsimTile, (height + gigs::kSsimTile - 1) / gigs::kSsimTile,
                  channels);
  hipLaunchKernelGGL(gigs::l1_ssim_fwd_kernel<false>, grid, dim3(256), 0, s, height, width, image, gt,
                     gigs::make_window(), d_mu1, d_e11, d_e12, scratch, nullptr, nullptr);
  hipLaunchKernelGGL(gigs::l1_ssim_finish_kernel, dim3(1), dim3(256), 0, s, scratch, (int)(grid.x * grid.y * grid.z),
                     (float)channels * (float)height * (float)width, lambda_dssim, out3);
  return gigs_internal_check_launch("l1_ssim_fwd");
}

size_t gigs_image_metrics_scratch_bytes(int channels, int height, int width) {
  if (channels <= 0 || height <= 0 || width <= 0) return 0;
  const size_t ssim = 4 * (size_t)channels * gigs::ssim_blocks(height, width);
  const size_t mae = gigs::mae_blocks((size_t)height * width);
  return (ssim > mae ? ssim : mae) * sizeof(double);
}

int gigs_image_metrics(int channels, int height, int width, const float* pred, const float* gt, const uint8_t* mask,
                       void* scratch, int* slot, double* out, void* stream) {
  if (channels <= 0 || height <= 0 || width <= 0 || !pred || !gt || !scratch || !out)
    return gigs_internal_fail(GIGS_ERR_INVALID, "image_metrics: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid((width + gigs::kSsimTile - 1) / gigs::kSsimTile, (height + gigs::kSsimTile - 1) / gigs::kSsimTile,
                  channels);
  gigs::StageTimer timer(gigs::Stage::kL1SsimFwd, stream);
  hipLaunchKernelGGL(gigs::l1_ssim_fwd_kernel<true>, grid, dim3(256), 0, s, height, width, pred, gt, gigs::make_window(),
                     nullptr, nullptr, nullptr, nullptr, mask, (double*)scratch);
  hipLaunchKernelGGL(gigs::image_metrics_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)scratch, channels,
                     (int)(grid.x * grid.y), (double)height * (double)width, slot, out);
  return gigs_internal_check_launch("image_metrics");
}

int gigs_normal_angular_error(int height, int width, const float* pred, const uint8_t* gt, int gt_channels,
                              void* scratch, int* slot, double* out, void* stream) {
  if (height <= 0 || width <= 0 || !pred || !gt || (gt_channels != 3 && gt_channels != 4) || !scratch || !out)
    return gigs_internal_fail(GIGS_ERR_INVALID, "normal_angular_error: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const size_t HW = (size_t)height * width;
  if (HW > 0x7fffffff) return gigs_internal_fail(GIGS_ERR_INVALID, "normal_angular_error: image too large");
  const unsigned blocks = gigs::mae_blocks(HW);
  gigs::StageTimer timer(gigs::Stage::kL1SsimFwd, stream);
  hipLaunchKernelGGL(gigs::normal_angular_error_kernel, dim3(blocks), dim3(256), 0, s, (int)HW, pred, gt, gt_channels,
                     (double*)scratch);
  hipLaunchKernelGGL(gigs::normal_angular_error_finish_kernel, dim3(1), dim3(256), 0, s, (const double*)scratch,
                     (int)blocks, (double)HW, slot, out);
  return gigs_internal_check_launch("normal_angular_error");
}

int gigs_l1_ssim_bwd(int channels, int height, int width, const float* image, const float* gt, float lambda_dssim,
                     const float* d_mu1, const float* d_e11, const float* d_e12, const float* g_loss, float* g_image,
                     void* stream) {
  if (channels <= 0 || height <= 0 || width <= 0 || !image || !gt || !d_mu1 || !d_e11 || !d_e12 || !g_image)
    return gigs_internal_fail(GIGS_ERR_INVALID, "l1_ssim_bwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  gigs::StageTimer timer(gigs::Stage::kL1SsimBwd, stream);
  const dim3 grid((width + gigs::kSsimTile - 1) / gigs::kSsimTile, (height + gigs::kSsimTile - 1) / gigs::kSsimTile,
                  channels);
  const float count = (float)channels * (float)height * (float)width;
  hipLaunchKernelGGL(gigs::l1_ssim_bwd_kernel, grid, dim3(256), 0, s, height, width, image, gt, gigs::make_window(),
                     d_mu1, d_e11, d_e12, g_loss, (1.0f - lambda_dssim) / count, -lambda_dssim / count, g_image);
  return gigs_internal_check_launch("l1_ssim_bwd");
}

int gigs_tv_loss_fwd(int channels, int height, int width, int step, const float* gt, const float* prediction,
                     const float* mask_f, float* scratch, float* loss, void* stream) {
  if (channels <= 0 || height <= 0 || width <= 0 || step < 1 || step >= height || step >= width ||
      !prediction || !scratch || !loss)
    return gigs_internal_fail(GIGS_ERR_INVALID, "tv_loss_fwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  gigs::StageTimer timer(gigs::Stage::kTvFwd, stream);
  const dim3 grid((width + 63) / 64, (height + 3) / 4);
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
  hipLaunchKernelGGL(gigs::tv_bwd_kernel, dim3((width + 63) / 64, (height + 3) / 4), dim3(256), 0, s, channels,
                     height, width, step, gt, prediction, mask_f, g_loss, g_prediction);
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

int gigs_adam_step(int n_groups, const gigs_adam_group* groups, double beta1, double beta2, double eps, int zero_grad,
                   void* stream) {
  return gigs_adam_step_dyn(n_groups, groups, beta1, beta2, eps, zero_grad, nullptr, stream);
}

void gigs_adam_scalars(double lr, int step, double beta1, double beta2, float* out2) {
  // torch/optim/adam.py (_single_tensor_adam): python-float bias corrections, then fp32 tensor ops
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  out2[0] = (float)(lr / bc1);
  out2[1] = (float)sqrt(bc2);
}

int gigs_adam_step_dyn(int n_groups, const gigs_adam_group* groups, double beta1, double beta2, double eps, int zero_grad,
                       const float* dyn, void* stream) {
  return gigs_adam_step_watch(n_groups, groups, beta1, beta2, eps, zero_grad, dyn, nullptr, nullptr, stream);
}

int gigs_adam_step_watch(int n_groups, const gigs_adam_group* groups, double beta1, double beta2, double eps, int zero_grad,
                         const float* dyn, const unsigned char* watch, unsigned* changed, void* stream) {
  return gigs_adam_step_guarded(n_groups, groups, beta1, beta2, eps, zero_grad, dyn, watch, changed, nullptr, stream);
}

int gigs_adam_step_guarded(int n_groups, const gigs_adam_group* groups, double beta1, double beta2, double eps, int zero_grad,
                           const float* dyn, const unsigned char* watch, unsigned* changed, const unsigned* guard, void* stream) {
  if (n_groups < 0 || (n_groups > 0 && !groups)) return gigs_internal_fail(GIGS_ERR_INVALID, "adam_step: bad argument");
  hipStream_t s = (hipStream_t)stream;
  gigs::StageTimer timer(gigs::Stage::kAdam, stream);
  int done = 0;
  while (done < n_groups) {
    gigs::AdamGroups G;
    memset(&G, 0, sizeof(G));
    unsigned chunks = 0;
    int k = 0;
    for (; done < n_groups && k < gigs::kAdamMaxGroups; done++) {
      const gigs_adam_group& g = groups[done];
      if (g.n < 0 || (!dyn && g.step < 1) || (g.n > 0 && (!g.param || !g.exp_avg || !g.exp_avg_sq)))  // grad == NULL: an exact-zero gradient, not materialised
        return gigs_internal_fail(GIGS_ERR_INVALID, "adam_step: bad group");
      if (g.n == 0) {
        if (dyn && k > 0) break;  // keep the (dyn_base + k) <-> group index correspondence: close this launch
        if (dyn) { G.dyn_base = done + 1; }
        continue;
      }
      const unsigned long long c = (unsigned long long)((g.n + gigs::kAdamChunk - 1) / gigs::kAdamChunk);
      if (chunks + c > 0x7fffffffull) break;  // next launch
      if (k == 0) G.dyn_base = done;
      G.param[k] = g.param; G.grad[k] = g.grad; G.exp_avg[k] = g.exp_avg; G.exp_avg_sq[k] = g.exp_avg_sq;
      G.n[k] = g.n;
      if (watch && changed && watch[done]) G.watch_mask |= 1u << k;
      G.first_chunk[k] = chunks;
      chunks += (unsigned)c;
      // torch/optim/adam.py (_single_tensor_adam): python-float bias corrections, then fp32 tensor ops
      if (!dyn) {
        float sc[2];
        gigs_adam_scalars(g.lr, g.step, beta1, beta2, sc);
        G.step_size[k] = sc[0];
        G.bc2_sqrt[k] = sc[1];
      }
      k++;
    }
    G.count = k;
    G.dyn = dyn;
    G.changed = changed;
    G.guard = guard;
    G.first_chunk[k] = chunks;
    if (k == 0 || chunks == 0) {
      if (k == 0 && done < n_groups)  // a single group too large for one grid
        return gigs_internal_fail(GIGS_ERR_INVALID, "adam_step: group too large");
      continue;
    }
    const gigs::AdamConsts K = {(float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps};
    // bit 8 of zero_grad (diagnostic, tools/adam_bw.py): the plain loads / stores instead of the streaming ones
    if (zero_grad & 0x100) hipLaunchKernelGGL(gigs::adam_kernel<false>, dim3(chunks), dim3(256), 0, s, G, K, zero_grad & 0xff);
    else hipLaunchKernelGGL(gigs::adam_kernel<true>, dim3(chunks), dim3(256), 0, s, G, K, zero_grad & 0xff);
  }
  return gigs_internal_check_launch("adam_step");
}

int gigs_densify_stats_guarded(int P, const float* viewspace_grad, const int* radii, float* xyz_gradient_accum,
                               float* xyz_gradient_accum_abs, float* xyz_gradient_accum_abs_max, float* denom,
                               float* max_radii2D, const int* skip, void* stream) {
  if (P < 0 || (P > 0 && (!viewspace_grad || !radii || !xyz_gradient_accum || !xyz_gradient_accum_abs ||
                          !xyz_gradient_accum_abs_max || !denom || !max_radii2D)))
    return gigs_internal_fail(GIGS_ERR_INVALID, "densify_stats: bad argument");
  if (P == 0) return 0;
  gigs::StageTimer timer(gigs::Stage::kDensifyStats, stream);
  hipLaunchKernelGGL(gigs::densify_stats_kernel, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, P,
                     viewspace_grad, radii, xyz_gradient_accum, xyz_gradient_accum_abs, xyz_gradient_accum_abs_max,
                     denom, max_radii2D, skip);
  return gigs_internal_check_launch("densify_stats");
}

int gigs_densify_stats(int P, const float* viewspace_grad, const int* radii, float* xyz_gradient_accum,
                       float* xyz_gradient_accum_abs, float* xyz_gradient_accum_abs_max, float* denom,
                       float* max_radii2D, void* stream) {
  return gigs_densify_stats_guarded(P, viewspace_grad, radii, xyz_gradient_accum, xyz_gradient_accum_abs,
                                    xyz_gradient_accum_abs_max, denom, max_radii2D, nullptr, stream);
}

int gigs_gather_rows(int n_tensors, const gigs_gather_tensor* tensors, long long n_rows_out, long long n_rows_in,
                     const int* src_index, const uint8_t* zero_row, void* stream) {
  if (n_tensors < 0 || n_rows_out < 0 || n_rows_in < 0 || (n_tensors > 0 && !tensors) || (n_rows_out > 0 && !src_index))
    return gigs_internal_fail(GIGS_ERR_INVALID, "gather_rows: bad argument");
  if (n_rows_out == 0 || n_tensors == 0) return 0;
  gigs::StageTimer timer(gigs::Stage::kGatherRows, stream);
  int done = 0;
  while (done < n_tensors) {
    gigs::GatherTable T;
    memset(&T, 0, sizeof(T));
    unsigned chunks = 0;
    int k = 0;
    for (; done < n_tensors && k < gigs::kGatherMaxTensors; done++) {
      const gigs_gather_tensor& g = tensors[done];
      if (g.row_floats <= 0 || !g.dst || (n_rows_in > 0 && !g.src))
        return gigs_internal_fail(GIGS_ERR_INVALID, "gather_rows: bad tensor");
      const unsigned long long c =
          (unsigned long long)((n_rows_out * g.row_floats + gigs::kGatherChunk - 1) / gigs::kGatherChunk);
      if (chunks + c > 0x7fffffffull) {
        if (k == 0)
          return gigs_internal_fail(GIGS_ERR_INVALID, "gather_rows: tensor too large");
        break;
      }
      T.src[k] = g.src; T.dst[k] = g.dst; T.row_floats[k] = g.row_floats; T.zero_new[k] = g.zero_new;
      T.first_chunk[k] = chunks;
      chunks += (unsigned)c;
      k++;
    }
    T.count = k;
    T.first_chunk[k] = chunks;
    hipLaunchKernelGGL(gigs::gather_rows_kernel, dim3(chunks), dim3(256), 0, (hipStream_t)stream, T, n_rows_out,
                       src_index, zero_row);
  }
  return gigs_internal_check_launch("gather_rows");
}

static bool act_raw_ok(const gigs_activation_raw* r, int K) {
  return r && r->f_dc && (K == 1 || r->f_rest) && r->opacity && r->normal && r->albedo && r->roughness && r->metallic &&
         r->scaling && r->rotation;
}
static void act_fill_raw(gigs::ActPtrs& A, const gigs_activation_raw* r) {
  A.f_dc = r->f_dc; A.f_rest = r->f_rest; A.opacity = r->opacity; A.normal = r->normal; A.albedo = r->albedo;
  A.roughness = r->roughness; A.metallic = r->metallic; A.scaling = r->scaling; A.rotation = r->rotation;
}

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
