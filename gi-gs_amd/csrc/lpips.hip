// lpips.hip -- LPIPS with the VGG16 backbone (lpips 0.1, net="vgg", lpips=True, spatial=False, eval mode), forward only.
//
// The network (torchvision vgg16().features, lpips/pretrained_networks.py's vgg16 slices, lpips/lpips.py's LPIPS):
//   ScalingLayer  x' = (x - shift) / scale on the input, before the zero padding of conv1_1
//   13 x (3x3 conv, padding 1, stride 1, + bias, ReLU), MaxPool2d(2, 2) before conv2_1, conv3_1, conv4_1, conv5_1
//   taps after the ReLU of conv1_2, conv2_2, conv3_3, conv4_3, conv5_3 (C = 64, 128, 256, 512, 512)
//   per tap and pixel: f / (sqrt(sum_c f^2) + 1e-10) for both images, d = sum_c w_c (f0 - f1)^2 (the `lin` 1x1 conv)
//   value = sum over the taps, in order, of the mean of d over that tap's pixels
//
// Both images of every pair run as one batch of 2n (in0 = images 0..n-1, in1 = n..2n-1), NHWC in two ping-pong
// activation buffers of the scratch.  Kernels:
//   conv1_kernel   conv1_1 (Cin = 3, K = 27): VALU, 4 threads per pixel, 16 outputs each; applies normalize / ScalingLayer
//   conv_kernel    every other conv: implicit GEMM on v_mfma_f32_32x32x2_f32 (f32 in, f32 accumulate), D[cout][pixel]
//                  = sum_k Wp[k][cout] * X[k][pixel], K = 9 * Cin in the order (ky, kx, ci); a 128-pixel x TC-cout
//                  tile per 256-thread workgroup, K staged through LDS 32 at a time (one (ky, kx) and 32 channels)
//   pool_kernel    2x2 max pool, NHWC, odd sizes floored
//   head_kernel    normalise + squared difference + lin dot, 16 lanes per pixel, a double partial per 64 pixels and image
//   finish_kernel  one workgroup: the partials of the five taps in a fixed order -> the record of each image
// Every output element is an fmaf chain in a fixed K order that depends on nothing but its own inputs (not on the tile,
// the batch position or the grid), and every sum of the value is a fixed-order double reduction, so a pair gives the
// same bits alone, inside a batch, in either argument order (the head is symmetric) and on every call.
#include <cmath>

#include "block_reduce.h"
#include "gigs_internal.h"

namespace gigs {
namespace lp {

constexpr int kLayers = 13;
constexpr int kTaps = 5;
constexpr int kCin[kLayers] = {3, 64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512};
constexpr int kCout[kLayers] = {64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512};
constexpr int kTapC[kTaps] = {64, 128, 256, 512, 512};
constexpr int kMinSide = 16;  // conv5 needs at least one pixel after four floor-halvings

constexpr int kTP = 128;  // conv tile: pixels
constexpr int kKC = 32;   // conv tile: K per LDS stage

// packed weights: per layer Wp[9 * Cin][Cout] (k = (ky * 3 + kx) * Cin + ci) then bias[Cout]; then the 5 lin vectors
constexpr size_t layer_floats(int l) { return (size_t)9 * kCin[l] * kCout[l] + kCout[l]; }
constexpr size_t layer_offset(int l) { return l == 0 ? 0 : layer_offset(l - 1) + layer_floats(l - 1); }
constexpr size_t lin_offset(int t) { return t == 0 ? layer_offset(kLayers) : lin_offset(t - 1) + kTapC[t - 1]; }
constexpr size_t kWeightFloats = lin_offset(kTaps);

typedef float floatx16 __attribute__((ext_vector_type(16)));

// torch [Cout][Cin][3][3] -> Wp[(ky * 3 + kx) * Cin + ci][Cout]
__global__ void __launch_bounds__(256)
pack_kernel(int Cin, int Cout, const float* __restrict__ w, float* __restrict__ wp) {
  const size_t total = (size_t)9 * Cin * Cout;
  for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) {
    const int co = (int)(o % Cout);
    const int k = (int)(o / Cout);
    const int tap = k / Cin, ci = k - tap * Cin;
    wp[o] = w[((size_t)co * Cin + ci) * 9 + tap];
  }
}

// conv1_1 on the planar inputs: image b < n is in0[b], else in1[b - n]; out NHWC [2n][H][W][64].  Four threads per
// pixel, 16 output channels each.
__global__ void __launch_bounds__(256)
conv1_kernel(int n, int H, int W, const float* __restrict__ in0, const float* __restrict__ in1, int normalize,
             const float* __restrict__ wp, float* __restrict__ out) {
  __shared__ float s_w[27 * 64 + 64];
  for (int i = threadIdx.x; i < 27 * 64 + 64; i += 256) s_w[i] = wp[i];
  __syncthreads();
  const int HW = H * W;
  const size_t g = (size_t)blockIdx.x * 256 + threadIdx.x;
  const size_t p = g >> 2;
  const int quarter = (int)(g & 3);
  if (p >= (size_t)2 * n * HW) return;
  const int b = (int)(p / HW), rem = (int)(p - (size_t)b * HW);
  const int y = rem / W, x = rem - y * W;
  const float* src = b < n ? in0 + (size_t)b * 3 * HW : in1 + (size_t)(b - n) * 3 * HW;
  const float shift[3] = {-0.030f, -0.088f, -0.188f};  // lpips/lpips.py ScalingLayer
  const float scale[3] = {0.458f, 0.448f, 0.450f};
  float xv[27];
#pragma unroll
  for (int tap = 0; tap < 9; tap++) {
    const int yy = y + tap / 3 - 1, xx = x + tap % 3 - 1;
    const bool ok = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      float v = 0.0f;
      if (ok) {
        v = src[(size_t)c * HW + (size_t)yy * W + xx];
        if (normalize) v = 2.0f * v - 1.0f;
        v = (v - shift[c]) / scale[c];
      }
      xv[tap * 3 + c] = v;
    }
  }
  float4* dst = (float4*)(out + p * 64);
  for (int c4 = quarter * 4; c4 < quarter * 4 + 4; c4++) {
    float r[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int co = c4 * 4 + j;
      float acc = 0.0f;
#pragma unroll
      for (int k = 0; k < 27; k++) acc = fmaf(s_w[k * 64 + co], xv[k], acc);
      r[j] = fmaxf(acc + s_w[27 * 64 + co], 0.0f);
    }
    dst[c4] = make_float4(r[0], r[1], r[2], r[3]);
  }
}

// 3x3 conv + bias + ReLU, NHWC in [P][Cin] -> out [P][Cout], P = images * H * W.  A 1-D grid of (pixel tile, cout tile)
// with the cout tile fastest, so the workgroups that share a pixel tile run together.  Four waves as 2 (cout) x 2
// (pixels): a wave owns a TC/2 x 64 block = (TC/64) x 2 MFMA tiles of 32 x 32.  The A operand (weights) and B operand
// (activations) are read k-major from LDS: lane l takes row k = 2 kk + (l >> 5), column l & 31.
template <int TC>
__global__ void __launch_bounds__(256)
conv_kernel(int P, int H, int W, int Cin, int Cout, const float* __restrict__ in, const float* __restrict__ wp,
            const float* __restrict__ bias, float* __restrict__ out) {
  constexpr int LDW = TC + 4;    // float4 rows, 16-B aligned
  constexpr int LDX = kTP + 1;   // transposed scalar writes: odd stride
  constexpr int NW = kKC * TC / 4 / 256;  // float4 weight loads per thread per stage
  constexpr int TI = TC / 64;             // MFMA tiles along cout per wave
  __shared__ float s_w[kKC * LDW];
  __shared__ float s_x[kKC * LDX];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int nct = Cout / TC;
  const int c0 = (int)(blockIdx.x % nct) * TC;
  const int p0 = (int)(blockIdx.x / nct) * kTP;
  const int HW = H * W;

  // activation staging: 4 float4 per thread, pixel m = (t >> 3) + 32 r, channels 4 k4 .. 4 k4 + 3 of the stage
  const int k4 = t & 7;
  int py[4], px[4];
  const float* src[4];
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int p = p0 + (t >> 3) + 32 * r;
    const int img = p / HW, rem = p - img * HW;
    const int y = rem / W;
    py[r] = p < P ? y : -4;  // an invalid row for every shift
    px[r] = rem - y * W;
    src[r] = in + (size_t)(p < P ? p : 0) * Cin + k4 * 4;
  }
  const int cpt = Cin / kKC;  // stages per (ky, kx)
  const int nstage = 9 * cpt;
  float4 xr[4], wr[NW];
  auto load = [&](int s) {
    const int tap = s / cpt, ci0 = (s - tap * cpt) * kKC;
    const int dy = tap / 3 - 1, dx = tap % 3 - 1;
    const long off = ((long)dy * W + dx) * Cin + ci0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const int y = py[r] + dy, x = px[r] + dx;
      xr[r] = ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? *(const float4*)(src[r] + off)
                                                                        : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
    const float* ws = wp + (size_t)s * kKC * Cout + c0;
#pragma unroll
    for (int r = 0; r < NW; r++) {
      const int f = t + 256 * r;
      const int k = f / (TC / 4), q = f - k * (TC / 4);
      wr[r] = *(const float4*)(ws + (size_t)k * Cout + q * 4);
    }
  };

  floatx16 acc[TI][2];
#pragma unroll
  for (int i = 0; i < TI; i++)
#pragma unroll
    for (int j = 0; j < 2; j++)
#pragma unroll
      for (int e = 0; e < 16; e++) acc[i][j][e] = 0.0f;

  const int wc = (wave & 1) * (TC / 2), wpx = (wave >> 1) * 64;
  const int col = lane & 31, kh = lane >> 5;
  load(0);
  for (int s = 0; s < nstage; s++) {
    __syncthreads();  // the previous stage's reads are done
#pragma unroll
    for (int r = 0; r < 4; r++) {
      float* d = s_x + (k4 * 4) * LDX + (t >> 3) + 32 * r;
      d[0] = xr[r].x;
      d[LDX] = xr[r].y;
      d[2 * LDX] = xr[r].z;
      d[3 * LDX] = xr[r].w;
    }
#pragma unroll
    for (int r = 0; r < NW; r++) {
      const int f = t + 256 * r;
      const int k = f / (TC / 4), q = f - k * (TC / 4);
      *(float4*)(s_w + k * LDW + q * 4) = wr[r];
    }
    __syncthreads();
    if (s + 1 < nstage) load(s + 1);  // in flight during this stage's MFMAs
#pragma unroll
    for (int kk = 0; kk < kKC / 2; kk++) {
      const int k = 2 * kk + kh;
      float a[TI], b[2];
#pragma unroll
      for (int i = 0; i < TI; i++) a[i] = s_w[k * LDW + wc + 32 * i + col];
#pragma unroll
      for (int j = 0; j < 2; j++) b[j] = s_x[k * LDX + wpx + 32 * j + col];
#pragma unroll
      for (int i = 0; i < TI; i++)
#pragma unroll
        for (int j = 0; j < 2; j++) acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[i], b[j], acc[i][j], 0, 0, 0);
    }
  }

  // D[row = cout][col = pixel]: register 4 q + e of lane l is cout 8 q + 4 (l >> 5) + e of the tile, pixel l & 31
#pragma unroll
  for (int j = 0; j < 2; j++) {
    const int p = p0 + wpx + 32 * j + col;
    if (p >= P) continue;
    float* dst = out + (size_t)p * Cout;
#pragma unroll
    for (int i = 0; i < TI; i++)
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const int c = c0 + wc + 32 * i + 8 * q + 4 * kh;
        const float4 bb = *(const float4*)(bias + c);
        *(float4*)(dst + c) = make_float4(fmaxf(acc[i][j][4 * q + 0] + bb.x, 0.0f), fmaxf(acc[i][j][4 * q + 1] + bb.y, 0.0f),
                                          fmaxf(acc[i][j][4 * q + 2] + bb.z, 0.0f), fmaxf(acc[i][j][4 * q + 3] + bb.w, 0.0f));
      }
  }
}

// MaxPool2d(2, 2) on NHWC [B][H][W][C] -> [B][H / 2][W / 2][C]
__global__ void __launch_bounds__(256)
pool_kernel(int B, int H, int W, int C, const float* __restrict__ in, float* __restrict__ out) {
  const int Ho = H / 2, Wo = W / 2, C4 = C / 4;
  const size_t total = (size_t)B * Ho * Wo * C4;
  for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) {
    const int c4 = (int)(o % C4);
    const size_t pix = o / C4;
    const int xo = (int)(pix % Wo);
    const size_t r = pix / Wo;
    const int yo = (int)(r % Ho), b = (int)(r / Ho);
    const float4* s = (const float4*)(in + (((size_t)b * H + 2 * yo) * W + 2 * xo) * C) + c4;
    const size_t row = (size_t)W * C4;
    const float4 a = s[0], bq = s[C4], c = s[row], d = s[row + C4];
    ((float4*)out)[o] = make_float4(fmaxf(fmaxf(a.x, bq.x), fmaxf(c.x, d.x)), fmaxf(fmaxf(a.y, bq.y), fmaxf(c.y, d.y)),
                                    fmaxf(fmaxf(a.z, bq.z), fmaxf(c.z, d.z)), fmaxf(fmaxf(a.w, bq.w), fmaxf(c.w, d.w)));
  }
}

// sum over the 16 lanes of a group by an xor butterfly: every lane gets the same bits (a + b == b + a)
__device__ __forceinline__ float group16_sum(float v) {
#pragma unroll
  for (int m = 1; m < 16; m <<= 1) v += __shfl_xor(v, m);
  return v;
}

// one tap: act NHWC [2n][HW][C].  16 lanes per pixel (lane j reads channels 4 j + 64 r .. +3: 256 contiguous bytes per
// pixel and step), a group takes 4 pixels in turn, 64 pixels per workgroup; part[i * gridDim.x + block] = the sum over
// the block's pixels of image i of d, in double.
constexpr int kHeadPix = 64;
__global__ void __launch_bounds__(256)
head_kernel(int n, int HW, int C, const float* __restrict__ act, const float* __restrict__ lin, double* __restrict__ part) {
  __shared__ double s_red[4];
  const int i = blockIdx.y;
  const int grp = threadIdx.x >> 4, j = threadIdx.x & 15;
  double d = 0.0;
  for (int q = 0; q < kHeadPix / 16; q++) {
    const int p = blockIdx.x * kHeadPix + q * 16 + grp;
    if (p >= HW) break;
    const float4* f0 = (const float4*)(act + ((size_t)i * HW + p) * C) + j;
    const float4* f1 = (const float4*)(act + ((size_t)(n + i) * HW + p) * C) + j;
    const float4* w = (const float4*)lin + j;
    float s0 = 0.0f, s1 = 0.0f;
    for (int c = 0; c < C / 4; c += 16) {
      const float4 a = f0[c], b = f1[c];
      s0 = fmaf(a.x, a.x, s0); s0 = fmaf(a.y, a.y, s0); s0 = fmaf(a.z, a.z, s0); s0 = fmaf(a.w, a.w, s0);
      s1 = fmaf(b.x, b.x, s1); s1 = fmaf(b.y, b.y, s1); s1 = fmaf(b.z, b.z, s1); s1 = fmaf(b.w, b.w, s1);
    }
    s0 = group16_sum(s0);
    s1 = group16_sum(s1);
    const float n0 = sqrtf(s0) + 1e-10f, n1 = sqrtf(s1) + 1e-10f;  // lpips/__init__.py normalize_tensor
    float acc = 0.0f;
    for (int c = 0; c < C / 4; c += 16) {
      const float4 a = f0[c], b = f1[c], ww = w[c];
      float e;
      e = a.x / n0 - b.x / n1; acc = fmaf(ww.x, e * e, acc);
      e = a.y / n0 - b.y / n1; acc = fmaf(ww.y, e * e, acc);
      e = a.z / n0 - b.z / n1; acc = fmaf(ww.z, e * e, acc);
      e = a.w / n0 - b.w / n1; acc = fmaf(ww.w, e * e, acc);
    }
    acc = group16_sum(acc);
    if (j == 0) d += (double)acc;
  }
  d = block_sum(d, s_red);
  if (threadIdx.x == 0) part[(size_t)i * gridDim.x + blockIdx.x] = d;
}

struct TapGrid {
  int blocks[kTaps];     // head workgroups per image
  size_t offset[kTaps];  // of the tap's partials, in doubles
  double npix[kTaps];
};

// record of image i (stride 6) = {sum over taps of mean d, mean d of tap 0 .. 4} at out + 6 (*slot + i); *slot += n
__global__ void __launch_bounds__(256)
finish_kernel(int n, const double* __restrict__ part, TapGrid g, int* slot, double* __restrict__ out) {
  __shared__ double s_red[4];
  double* rec = out + 6 * (size_t)(slot ? *slot : 0);
  for (int i = 0; i < n; i++) {
    double val = 0.0;
    for (int l = 0; l < kTaps; l++) {
      const double* q = part + g.offset[l] + (size_t)i * g.blocks[l];
      double s = 0.0;
      for (int r = threadIdx.x; r < g.blocks[l]; r += 256) s += q[r];
      s = block_sum(s, s_red) / g.npix[l];
      val += s;
      if (threadIdx.x == 0) rec[6 * (size_t)i + 1 + l] = s;
    }
    if (threadIdx.x == 0) rec[6 * (size_t)i] = val;
  }
  __syncthreads();  // every thread has read *slot
  if (slot && threadIdx.x == 0) *slot += n;
}

// raw tap NHWC [2n][HW][C] -> NCHW [n][C][HW] of each image set
__global__ void __launch_bounds__(256)
tap_out_kernel(int n, int HW, int C, const float* __restrict__ act, float* __restrict__ t0, float* __restrict__ t1) {
  const size_t total = (size_t)n * C * HW;
  for (size_t o = (size_t)blockIdx.x * 256 + threadIdx.x; o < total; o += (size_t)gridDim.x * 256) {
    const int p = (int)(o % HW);
    const size_t r = o / HW;
    const int c = (int)(r % C), i = (int)(r / C);
    t0[o] = act[((size_t)i * HW + p) * C + c];
    t1[o] = act[((size_t)(n + i) * HW + p) * C + c];
  }
}

inline unsigned grid_for(size_t work) {
  const size_t b = (work + 255) / 256;
  return (unsigned)(b < 65536 ? b : 65536);
}

struct Sizes {
  int h[kTaps], w[kTaps];
  size_t act_floats;  // one ping-pong buffer
  TapGrid g;
  size_t bytes;
};

inline Sizes sizes(int n, int H, int W) {
  Sizes z;
  for (int l = 0; l < kTaps; l++) {
    z.h[l] = l == 0 ? H : z.h[l - 1] / 2;
    z.w[l] = l == 0 ? W : z.w[l - 1] / 2;
  }
  z.act_floats = (size_t)2 * n * H * W * 64;  // the largest activation: conv1_x
  size_t off = 0;
  for (int l = 0; l < kTaps; l++) {
    const int hw = z.h[l] * z.w[l];
    z.g.blocks[l] = (hw + kHeadPix - 1) / kHeadPix;
    z.g.offset[l] = off;
    z.g.npix[l] = (double)hw;
    off += (size_t)n * z.g.blocks[l];
  }
  z.bytes = 2 * z.act_floats * sizeof(float) + off * sizeof(double);
  return z;
}

}  // namespace lp
}  // namespace gigs

extern "C" {

size_t gigs_lpips_vgg_weight_floats(void) { return gigs::lp::kWeightFloats; }

int gigs_lpips_vgg_pack(const float* const* conv_w, const float* const* conv_b, const float* const* lin_w, float* packed,
                        void* stream) {
  using namespace gigs::lp;
  if (!conv_w || !conv_b || !lin_w || !packed) return gigs_internal_fail(GIGS_ERR_INVALID, "lpips_vgg_pack: bad argument");
  for (int l = 0; l < kLayers; l++)
    if (!conv_w[l] || !conv_b[l]) return gigs_internal_fail(GIGS_ERR_INVALID, "lpips_vgg_pack: NULL conv weight");
  for (int t = 0; t < kTaps; t++)
    if (!lin_w[t]) return gigs_internal_fail(GIGS_ERR_INVALID, "lpips_vgg_pack: NULL lin weight");
  hipStream_t s = (hipStream_t)stream;
  for (int l = 0; l < kLayers; l++) {
    float* dst = packed + layer_offset(l);
    const size_t nw = (size_t)9 * kCin[l] * kCout[l];
    hipLaunchKernelGGL(pack_kernel, dim3(grid_for(nw)), dim3(256), 0, s, kCin[l], kCout[l], conv_w[l], dst);
    if (hipMemcpyAsync(dst + nw, conv_b[l], kCout[l] * sizeof(float), hipMemcpyDeviceToDevice, s) != hipSuccess)
      return gigs_internal_fail(GIGS_ERR_HIP, "lpips_vgg_pack: copy failed");
  }
  for (int t = 0; t < kTaps; t++)
    if (hipMemcpyAsync(packed + lin_offset(t), lin_w[t], kTapC[t] * sizeof(float), hipMemcpyDeviceToDevice, s) !=
        hipSuccess)
      return gigs_internal_fail(GIGS_ERR_HIP, "lpips_vgg_pack: copy failed");
  return gigs_internal_check_launch("lpips_vgg_pack");
}

size_t gigs_lpips_vgg_scratch_bytes(int n, int height, int width) {
  using namespace gigs::lp;
  if (n <= 0 || height < kMinSide || width < kMinSide) return 0;
  return sizes(n, height, width).bytes;
}

int gigs_lpips_vgg(int n, int height, int width, const float* in0, const float* in1, int normalize, const float* packed,
                   void* scratch, int* slot, double* out, float* const* taps, void* stream) {
  using namespace gigs::lp;
  if (n <= 0 || !in0 || !in1 || !packed || !scratch || !out)
    return gigs_internal_fail(GIGS_ERR_INVALID, "lpips_vgg: bad argument");
  if (height < kMinSide || width < kMinSide)
    return gigs_internal_fail(GIGS_ERR_INVALID, "lpips_vgg: height and width must be at least 16 (conv5 has no pixels)");
  if ((size_t)2 * n * height * width * 64 >= ((size_t)1 << 40))
    return gigs_internal_fail(GIGS_ERR_INVALID, "lpips_vgg: batch too large");
  if (taps)
    for (int i = 0; i < 2 * kTaps; i++)
      if (!taps[i]) return gigs_internal_fail(GIGS_ERR_INVALID, "lpips_vgg: taps needs 10 pointers");
  hipStream_t s = (hipStream_t)stream;
  const Sizes z = sizes(n, height, width);
  float* cur = (float*)scratch;
  float* nxt = cur + z.act_floats;
  double* part = (double*)(nxt + z.act_floats);
  const int B = 2 * n;

  hipLaunchKernelGGL(conv1_kernel, dim3((unsigned)(((size_t)4 * B * height * width + 255) / 256)), dim3(256), 0, s, n, height,
                     width, in0, in1, normalize, packed, cur);
  int l = 1;
  for (int tap = 0; tap < kTaps; tap++) {
    const int H = z.h[tap], W = z.w[tap], P = B * H * W;
    if (tap > 0) {  // MaxPool2d(2, 2) of the previous tap
      const int C = kTapC[tap - 1], Hp = z.h[tap - 1], Wp = z.w[tap - 1];
      hipLaunchKernelGGL(pool_kernel, dim3(grid_for((size_t)B * H * W * (C / 4))), dim3(256), 0, s, B, Hp, Wp, C, cur,
                         nxt);
      float* t = cur; cur = nxt; nxt = t;
    }
    const int nconv = tap == 0 ? 1 : (tap == 1 ? 2 : 3);  // conv1_1 ran above
    for (int c = 0; c < nconv; c++, l++) {
      const float* w = packed + layer_offset(l);
      const float* b = w + (size_t)9 * kCin[l] * kCout[l];
      const unsigned ptiles = (unsigned)((P + kTP - 1) / kTP);
      // 64-wide cout tiles for Cout = 64 and for grids that would not fill the 256 CUs twice over (the deep layers of
      // small images); an output element is the same fma chain either way
      if (kCout[l] == 64 || ptiles * (kCout[l] / 128) < 512)
        hipLaunchKernelGGL(conv_kernel<64>, dim3(ptiles * (kCout[l] / 64)), dim3(256), 0, s, P, H, W, kCin[l], kCout[l], cur,
                           w, b, nxt);
      else
        hipLaunchKernelGGL(conv_kernel<128>, dim3(ptiles * (kCout[l] / 128)), dim3(256), 0, s, P, H, W, kCin[l], kCout[l],
                           cur, w, b, nxt);
      float* t = cur; cur = nxt; nxt = t;
    }
    hipLaunchKernelGGL(head_kernel, dim3(z.g.blocks[tap], n), dim3(256), 0, s, n, H * W, kTapC[tap], cur,
                       packed + lin_offset(tap), part + z.g.offset[tap]);
    if (taps)
      hipLaunchKernelGGL(tap_out_kernel, dim3(grid_for((size_t)n * kTapC[tap] * H * W)), dim3(256), 0, s, n, H * W,
                         kTapC[tap], cur, taps[tap], taps[kTaps + tap]);
  }
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(256), 0, s, n, part, z.g, slot, out);
  return gigs_internal_check_launch("lpips_vgg");
}
}  // extern "C"
