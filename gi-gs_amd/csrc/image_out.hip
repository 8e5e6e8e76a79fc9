// image_out.hip -- float planes -> 8-bit sheets -> filtered PNG scanlines, all images of a view per launch.
//
// The device half of the image writer (image_writer.py): what is left for the host is a run-length deflate of bytes
// that are already filtered, the chunk CRCs and the write.  Kernels:
//   pack_kernel     grid (kPackBlocks, n): image blockIdx.y, grid-stride over groups of 4 pixels.  Fast path (width % 4
//                   == 0, planes 16-byte and destination 4-byte aligned): one float4 per channel in, three dwords out;
//                   otherwise a pixel per thread with byte stores.  v = trunc(clamp(x * 255 + bias, 0, 255)): the
//                   product and the sum are two roundings (__fmul_rn / __fadd_rn, never an FMA) because torch's
//                   mul(255).add_(bias) rounds twice and the result is compared byte for byte; NaN -> 0 (fmaxf(NaN, 0)
//                   = 0).  With lohi: x = (x - lo) / (hi - lo) first, the correctly rounded division.
//   minmax_kernel / minmax_finish_kernel   kMinMaxBlocks fixed partials, then one workgroup: no float atomics, and
//                   min / max do not depend on the order anyway.  NaNs are ignored (fminf / fmaxf).
//   filter_kernel   grid (kFilterBlocks, n), one wave64 per row.  Pass 1: the row and the row above as 16-byte chunks
//                   per lane (dwordx4; the three bytes left of a chunk come from the dword in front of it), the sums of
//                   |residual as int8| of the five filters, a wave reduction, the smallest sum wins and ties go to the
//                   lowest filter number.  Pass 2: the chosen filter again (the row is in L1 / L2 by now), shifted to the
//                   byte phase of the output row, which starts at an odd offset (1 + 3 W bytes per row), and stored as
//                   aligned dwords; only the dwords a row shares with its neighbours are stored byte by byte.
// Descriptor tables live in device memory: the launches read no host state but n, so a captured graph stays valid
// while the tables are rewritten between replays.  A descriptor that is not well-formed is skipped.
#include "gigs_internal.h"

namespace gigs {
namespace img {

constexpr int kPackBlocks = 128;
constexpr int kFilterBlocks = 128;
constexpr int kMinMaxBlocks = GIGS_MINMAX_SCRATCH_FLOATS / 2;

typedef float fvec4 __attribute__((ext_vector_type(4)));
typedef unsigned uvec4 __attribute__((ext_vector_type(4)));

// The descriptors' pointers come out of memory, where the compiler cannot see their address space: the kernels say it is
// global, so that the accesses are global_* and not flat_* instructions.
#define GIGS_GLOBAL __attribute__((address_space(1)))
typedef GIGS_GLOBAL const float gfloat;
typedef GIGS_GLOBAL const fvec4 gfloat4;
typedef GIGS_GLOBAL unsigned gword;
typedef GIGS_GLOBAL const uint8_t gcbyte;
typedef GIGS_GLOBAL uint8_t gbyte;

__device__ __forceinline__ unsigned quant(float x, float bias, bool norm, float lo, float range) {
  if (norm) x = __fdiv_rn(__fsub_rn(x, lo), range);
  float t = __fadd_rn(__fmul_rn(x, 255.0f), bias);
  t = fminf(fmaxf(t, 0.0f), 255.0f);  // NaN -> 0
  return (unsigned)(int)t;
}

__global__ __launch_bounds__(256) void pack_kernel(int n, const gigs_pack_desc* __restrict__ descs) {
  const gigs_pack_desc d = descs[blockIdx.y];
  const int C = d.channels, H = d.height, W = d.width;
  if ((C != 1 && C != 3) || H <= 0 || W <= 0 || !d.src || !d.dst) return;
  const bool norm = d.lohi != nullptr;
  float lo = 0.0f, range = 1.0f;
  if (norm) {
    gfloat* lohi = (gfloat*)d.lohi;
    lo = lohi[0];
    range = __fsub_rn(lohi[1], lo);
  }
  const size_t plane = (size_t)H * W;
  gfloat* p0 = (gfloat*)d.src;
  gfloat* p1 = C == 3 ? p0 + plane : p0;
  gfloat* p2 = C == 3 ? p0 + 2 * plane : p0;
  gbyte* dst = (gbyte*)d.dst + (size_t)d.dst_x * 3;
  const size_t stride = (size_t)d.dst_stride;
  const int tid = blockIdx.x * 256 + threadIdx.x, nthr = gridDim.x * 256;
  const bool fast = (W & 3) == 0 && ((uintptr_t)d.src & 15) == 0 && (((uintptr_t)d.dst + (size_t)d.dst_x * 3) & 3) == 0 && (stride & 3) == 0;
  if (fast) {
    const int gw = W >> 2;
    const int groups = H * gw;
    for (int g = tid; g < groups; g += nthr) {
      const int y = g / gw, x = (g - y * gw) << 2;
      const size_t o = (size_t)y * W + x;
      const fvec4 r = *(gfloat4*)(p0 + o);
      fvec4 gg = r, b = r;
      if (C == 3) {
        gg = *(gfloat4*)(p1 + o);
        b = *(gfloat4*)(p2 + o);
      }
      const unsigned r0 = quant(r.x, d.bias, norm, lo, range), r1 = quant(r.y, d.bias, norm, lo, range),
                     r2 = quant(r.z, d.bias, norm, lo, range), r3 = quant(r.w, d.bias, norm, lo, range);
      unsigned g0 = r0, g1 = r1, g2 = r2, g3 = r3, b0 = r0, b1 = r1, b2 = r2, b3 = r3;
      if (C == 3) {
        g0 = quant(gg.x, d.bias, norm, lo, range); g1 = quant(gg.y, d.bias, norm, lo, range);
        g2 = quant(gg.z, d.bias, norm, lo, range); g3 = quant(gg.w, d.bias, norm, lo, range);
        b0 = quant(b.x, d.bias, norm, lo, range); b1 = quant(b.y, d.bias, norm, lo, range);
        b2 = quant(b.z, d.bias, norm, lo, range); b3 = quant(b.w, d.bias, norm, lo, range);
      }
      gword* w = (gword*)(dst + (size_t)y * stride + (size_t)x * 3);  // dword-aligned only: three stores, merged to a dwordx3
      w[0] = r0 | (g0 << 8) | (b0 << 16) | (r1 << 24);
      w[1] = g1 | (b1 << 8) | (r2 << 16) | (g2 << 24);
      w[2] = b2 | (r3 << 8) | (g3 << 16) | (b3 << 24);
    }
  } else {
    const size_t pixels = plane;
    for (size_t i = tid; i < pixels; i += nthr) {
      const int y = (int)(i / W), x = (int)(i - (size_t)y * W);
      gbyte* o = dst + (size_t)y * stride + (size_t)x * 3;
      const unsigned r = quant(p0[i], d.bias, norm, lo, range);
      o[0] = (uint8_t)r;
      o[1] = (uint8_t)(C == 3 ? quant(p1[i], d.bias, norm, lo, range) : r);
      o[2] = (uint8_t)(C == 3 ? quant(p2[i], d.bias, norm, lo, range) : r);
    }
  }
}

__device__ __forceinline__ void block_minmax(float& lo, float& hi, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    lo = fminf(lo, __shfl_xor(lo, o));
    hi = fmaxf(hi, __shfl_xor(hi, o));
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) { sh[wave] = lo; sh[4 + wave] = hi; }
  __syncthreads();
  lo = fminf(fminf(sh[0], sh[1]), fminf(sh[2], sh[3]));
  hi = fmaxf(fmaxf(sh[4], sh[5]), fmaxf(sh[6], sh[7]));
}

__global__ __launch_bounds__(256) void minmax_kernel(long long count, const float* __restrict__ src,
                                                     float* __restrict__ scratch) {
  __shared__ float sh[8];
  float lo = INFINITY, hi = -INFINITY;
  const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, nthr = (long long)gridDim.x * 256;
  if (((uintptr_t)src & 15) == 0) {
    const long long n4 = count >> 2;
    for (long long i = tid; i < n4; i += nthr) {
      const float4 v = reinterpret_cast<const float4*>(src)[i];
      lo = fminf(fminf(lo, v.x), fminf(fminf(v.y, v.z), v.w));
      hi = fmaxf(fmaxf(hi, v.x), fmaxf(fmaxf(v.y, v.z), v.w));
    }
    for (long long i = (n4 << 2) + tid; i < count; i += nthr) { lo = fminf(lo, src[i]); hi = fmaxf(hi, src[i]); }
  } else {
    for (long long i = tid; i < count; i += nthr) { lo = fminf(lo, src[i]); hi = fmaxf(hi, src[i]); }
  }
  block_minmax(lo, hi, sh);
  if (threadIdx.x == 0) { scratch[blockIdx.x] = lo; scratch[kMinMaxBlocks + blockIdx.x] = hi; }
}

__global__ __launch_bounds__(256) void minmax_finish_kernel(const float* __restrict__ scratch, float* __restrict__ out2) {
  __shared__ float sh[8];
  float lo = INFINITY, hi = -INFINITY;
  for (int i = threadIdx.x; i < kMinMaxBlocks; i += 256) {
    lo = fminf(lo, scratch[i]);
    hi = fmaxf(hi, scratch[kMinMaxBlocks + i]);
  }
  block_minmax(lo, hi, sh);
  if (threadIdx.x == 0) { out2[0] = lo; out2[1] = hi; }
}

// ---- PNG filters ---------------------------------------------------------------------------------------------------
// The dword at byte offset j of a row of N bytes (j a multiple of 4, j = -4 allowed): bytes outside [0, N) read as 0.
__device__ __forceinline__ unsigned row_word(gcbyte* row, int j, int N, bool aligned) {
  if (row == nullptr || j < 0 || j >= N) return 0u;
  if (aligned && j + 4 <= N) return *(GIGS_GLOBAL const unsigned*)(row + j);
  unsigned w = 0;
#pragma unroll
  for (int b = 0; b < 4; b++)
    if (j + b < N) w |= (unsigned)row[j + b] << (8 * b);
  return w;
}

// bytes [j - 4, j + 16) of a row as five dwords
__device__ __forceinline__ void row_chunk(gcbyte* row, int j, int N, bool aligned, unsigned (&w)[5]) {
  w[0] = row_word(row, j - 4, N, aligned);
  if (row != nullptr && aligned && j + 16 <= N) {
    const uvec4 v = *(GIGS_GLOBAL const uvec4*)(row + j);
    w[1] = v.x; w[2] = v.y; w[3] = v.z; w[4] = v.w;
  } else {
#pragma unroll
    for (int i = 0; i < 4; i++) w[1 + i] = row_word(row, j + 4 * i, N, aligned);
  }
}

__device__ __forceinline__ int byte_of(const unsigned (&w)[5], int i) { return (int)((w[i >> 2] >> (8 * (i & 3))) & 0xffu); }

// residual of filter F for current byte x, left a, up b, up-left c (PNG specification, section 9)
template <int F>
__device__ __forceinline__ int residual(int x, int a, int b, int c) {
  int pred = 0;
  if (F == 1) pred = a;
  if (F == 2) pred = b;
  if (F == 3) pred = (a + b) >> 1;
  if (F == 4) {
    const int pa = abs(b - c), pb = abs(a - c), pc = abs(a + b - 2 * c);
    pred = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
  }
  return (x - pred) & 0xff;
}

template <int F>
__device__ __forceinline__ void filter_chunk(const unsigned (&cur)[5], const unsigned (&up)[5], unsigned (&out)[4]) {
#pragma unroll
  for (int i = 0; i < 4; i++) {
    unsigned w = 0;
#pragma unroll
    for (int b = 0; b < 4; b++) {
      const int j = 4 * i + b;  // byte of the chunk; index j + 4 in the five-dword window, its left neighbour j + 1
      w |= (unsigned)residual<F>(byte_of(cur, j + 4), byte_of(cur, j + 1), byte_of(up, j + 4), byte_of(up, j + 1)) << (8 * b);
    }
    out[i] = w;
  }
}

__global__ __launch_bounds__(256) void filter_kernel(int n, const gigs_filter_desc* __restrict__ descs) {
  const gigs_filter_desc d = descs[blockIdx.y];
  const int H = d.height, W = d.width;
  if (H <= 0 || W <= 0 || !d.sheet || !d.out) return;
  const int N = 3 * W;
  const size_t stride = (size_t)d.stride;
  const bool aligned = ((uintptr_t)d.sheet & 15) == 0 && (stride & 15) == 0;
  const int lane = threadIdx.x & 63;
  const int wave = blockIdx.x * 4 + (threadIdx.x >> 6);
  for (int y = wave; y < H; y += gridDim.x * 4) {
    gcbyte* row = (gcbyte*)d.sheet + (size_t)y * stride;
    gcbyte* above = y > 0 ? row - stride : nullptr;
    // pass 1: the five sums of |residual as int8|
    unsigned sums[5] = {0u, 0u, 0u, 0u, 0u};
    for (int j0 = lane * 16; j0 < N; j0 += 64 * 16) {
      unsigned cur[5], up[5];
      row_chunk(row, j0, N, aligned, cur);
      row_chunk(above, j0, N, aligned, up);
#pragma unroll
      for (int j = 0; j < 16; j++) {
        if (j0 + j < N) {
          const int x = byte_of(cur, j + 4), a = byte_of(cur, j + 1), b = byte_of(up, j + 4), c = byte_of(up, j + 1);
          const int r0 = residual<0>(x, a, b, c), r1 = residual<1>(x, a, b, c), r2 = residual<2>(x, a, b, c),
                    r3 = residual<3>(x, a, b, c), r4 = residual<4>(x, a, b, c);
          sums[0] += r0 < 128 ? r0 : 256 - r0;
          sums[1] += r1 < 128 ? r1 : 256 - r1;
          sums[2] += r2 < 128 ? r2 : 256 - r2;
          sums[3] += r3 < 128 ? r3 : 256 - r3;
          sums[4] += r4 < 128 ? r4 : 256 - r4;
        }
      }
    }
#pragma unroll
    for (int f = 0; f < 5; f++)
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) sums[f] += __shfl_xor(sums[f], o);
    int best = 0;
#pragma unroll
    for (int f = 1; f < 5; f++)
      if (sums[f] < sums[best]) best = f;
    // pass 2: the chosen filter, stored at the byte phase of the output row.  Output dword m of this row covers the
    // filtered bytes [4 m - off, 4 m - off + 4); byte -1 is the filter type.
    gbyte* orow = (gbyte*)d.out + (size_t)y * (size_t)(N + 1) + 1;  // filtered byte 0
    const int off = (int)((uintptr_t)orow & 3);
    gbyte* obase = orow - off;  // 4-byte aligned
    if (lane == 0 && off == 0) orow[-1] = (uint8_t)best;
    unsigned carry = (unsigned)best << 24;  // the dword in front of chunk 0 ends with the filter type
    for (int base = 0; base < N + off; base += 64 * 16) {  // wave-uniform trip count: the shuffles below need every lane
      const int j0 = base + lane * 16;
      unsigned cur[5], up[5], fw[4];
      row_chunk(row, j0, N, aligned, cur);
      row_chunk(above, j0, N, aligned, up);
      switch (best) {
        case 0: filter_chunk<0>(cur, up, fw); break;
        case 1: filter_chunk<1>(cur, up, fw); break;
        case 2: filter_chunk<2>(cur, up, fw); break;
        case 3: filter_chunk<3>(cur, up, fw); break;
        default: filter_chunk<4>(cur, up, fw); break;
      }
      unsigned prev = __shfl_up(fw[3], 1);
      if (lane == 0) prev = carry;
      carry = __shfl(fw[3], 63);
      const unsigned seq[5] = {prev, fw[0], fw[1], fw[2], fw[3]};
      unsigned o[4];
#pragma unroll
      for (int i = 0; i < 4; i++)
        o[i] = off == 0 ? seq[i + 1] : ((seq[i] >> (8 * (4 - off))) | (seq[i + 1] << (8 * off)));
      const int jf = j0 - off;  // first filtered byte of o[0]
      if (jf >= -1 && jf + 16 <= N) {
        gword* w = (gword*)(obase + j0);  // dword-aligned only: four stores, merged to a dwordx4
        w[0] = o[0]; w[1] = o[1]; w[2] = o[2]; w[3] = o[3];
      } else {
#pragma unroll
        for (int i = 0; i < 4; i++) {
          const int jw = jf + 4 * i;
          if (jw >= -1 && jw + 4 <= N) {
            *(gword*)(obase + j0 + 4 * i) = o[i];
          } else {
#pragma unroll
            for (int b = 0; b < 4; b++)
              if (jw + b >= -1 && jw + b < N) orow[jw + b] = (uint8_t)(o[i] >> (8 * b));
          }
        }
      }
    }
  }
}

}  // namespace img
}  // namespace gigs

extern "C" {

int gigs_pack_images(int n, const gigs_pack_desc* desc, void* stream) {
  if (n == 0) return 0;
  if (n < 0 || n > GIGS_MAX_IMAGES || !desc) return gigs_internal_fail(GIGS_ERR_INVALID, "pack_images: bad argument");
  hipLaunchKernelGGL(gigs::img::pack_kernel, dim3(gigs::img::kPackBlocks, n), dim3(256), 0, (hipStream_t)stream, n, desc);
  return gigs_internal_check_launch("pack_images");
}

int gigs_plane_minmax(long long count, const float* src, float* scratch, float* out2, void* stream) {
  if (count <= 0 || !src || !scratch || !out2) return gigs_internal_fail(GIGS_ERR_INVALID, "plane_minmax: bad argument");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(gigs::img::minmax_kernel, dim3(gigs::img::kMinMaxBlocks), dim3(256), 0, s, count, src, scratch);
  hipLaunchKernelGGL(gigs::img::minmax_finish_kernel, dim3(1), dim3(256), 0, s, scratch, out2);
  return gigs_internal_check_launch("plane_minmax");
}

int gigs_png_filter(int n, const gigs_filter_desc* desc, void* stream) {
  if (n == 0) return 0;
  if (n < 0 || n > GIGS_MAX_IMAGES || !desc) return gigs_internal_fail(GIGS_ERR_INVALID, "png_filter: bad argument");
  hipLaunchKernelGGL(gigs::img::filter_kernel, dim3(gigs::img::kFilterBlocks, n), dim3(256), 0, (hipStream_t)stream, n, desc);
  return gigs_internal_check_launch("png_filter");
}
}  // extern "C"
