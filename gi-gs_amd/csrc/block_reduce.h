// block_reduce.h -- the one block sum of the library's 256-thread reduction kernels (device only).
//
// Assumes a one-dimensional workgroup of 256 threads = four waves of 64, every thread of which makes the call, and an
// LDS array `s_red` of four T.  The wave sums are added in the fixed order ((s0 + s1) + s2) + s3, so a result does not
// depend on the run, and it is valid in every thread.  The barrier in front of the LDS store makes back-to-back calls
// on one `s_red` safe.
#pragma once
#include "gigs_common.h"

namespace gigs {

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

}  // namespace gigs
