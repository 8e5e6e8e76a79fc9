// eval_metrics.hip -- per-view evaluation metrics (render.py:115-395 NVS, :596-631 albedo, normal_eval.py).
//
//   gigs_image_metrics          per-channel MSE, PSNR, SSIM and the masked MSE of one [C,H,W] pair: the evaluating form
//                               of the training loss's SSIM forward (ssim.h) and a one-block finish
//   gigs_normal_angular_error   normal_eval.py's mean angular error on what render.py saves as an 8-bit image
//
// The record of one view goes to out + stride * (*slot) and *slot is incremented (slot == NULL: to out), so a replayed
// graph fills successive records with no host synchronisation.  All sums are doubles added in a fixed order.
#include <cmath>

#include "block_reduce.h"
#include "gigs_internal.h"
#include "ssim.h"

namespace gigs {

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

static inline unsigned mae_blocks(size_t HW) {
  const size_t b = (HW + 255) / 256;
  return (unsigned)(b < 1024 ? b : 1024);
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

}  // namespace gigs

extern "C" {

size_t gigs_image_metrics_scratch_bytes(int channels, int height, int width) {
  if (channels <= 0 || height <= 0 || width <= 0) return 0;
  const size_t ssim = 4 * (size_t)channels * gigs::ssim_blocks(height, width);
  const size_t mae = gigs::mae_blocks((size_t)height * width);
  return (ssim > mae ? ssim : mae) * sizeof(double);
}

// Both entry points time themselves as l1_ssim_fwd on purpose: the stage table and the accounting recorded against it stay.
int gigs_image_metrics(int channels, int height, int width, const float* pred, const float* gt, const uint8_t* mask,
                       void* scratch, int* slot, double* out, void* stream) {
  if (channels <= 0 || height <= 0 || width <= 0 || !pred || !gt || !scratch || !out)
    return gigs_internal_fail(GIGS_ERR_INVALID, "image_metrics: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const dim3 grid = gigs::ssim_grid(height, width, channels);
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

}  // extern "C"
