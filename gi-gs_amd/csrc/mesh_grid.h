// mesh_grid.h -- what the mesh units share.  gigs::mesh_common, for mesh_clean, mesh_simplify, mesh_distance, mesh_raycast,
// mesh_light and mesh_atlas: this thread's item, the index range check, the float64 vector helpers, the counter hash and the block
// count of a launch.  gigs::mesh_distance, for mesh_distance and mesh_ray.h: the triangle grid's cell arithmetic
// (include/gigs_hip.h, "Comparing meshes", 4) and the host-side argument check of a grid; Grid is named by their kernels'
// signatures, so it keeps its namespace.  Header-only; nothing here is a symbol of the library.
#pragma once
#include <cfloat>
#include <cmath>

#include "gigs_internal.h"

namespace gigs {
namespace mesh_common {

// this thread's item of n, or -1: the index is formed and compared unsigned, so n close to 2^31 cannot wrap it
template <unsigned kBlock>
__device__ __forceinline__ int item(int n) {
  const unsigned i = blockIdx.x * kBlock + threadIdx.x;
  return i < (unsigned)n ? (int)i : -1;
}

__device__ __forceinline__ bool in_range(int a, int b, int c, int n) {
  return a >= 0 && a < n && b >= 0 && b < n && c >= 0 && c < n;
}

__device__ __forceinline__ bool finite3(const double* p) {
  return fabs(p[0]) <= DBL_MAX && fabs(p[1]) <= DBL_MAX && fabs(p[2]) <= DBL_MAX;
}

__device__ __forceinline__ double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

__device__ __forceinline__ void cross3(const double* a, const double* b, double* n) {
  n[0] = a[1] * b[2] - a[2] * b[1];
  n[1] = a[2] * b[0] - a[0] * b[2];
  n[2] = a[0] * b[1] - a[1] * b[0];
}

__device__ __forceinline__ void load3(const float* v, int i, double* p) {
  p[0] = (double)v[3 * (size_t)i];
  p[1] = (double)v[3 * (size_t)i + 1];
  p[2] = (double)v[3 * (size_t)i + 2];
}

__device__ __forceinline__ unsigned long long mix64(unsigned long long z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
  return z ^ (z >> 31);
}

inline unsigned blocks_for(int n, unsigned block = 256u) { return ((unsigned)n + block - 1u) / block; }

}  // namespace mesh_common

namespace mesh_distance {

using namespace gigs::mesh_common;

constexpr int kGridAxis = 256;

struct Grid {
  double lo[3], cell;
  int G[3];
};

// the clamped cell coordinate of x on axis a; a NaN goes to 0
__device__ __forceinline__ int cell_of(const Grid& g, int a, double x) {
  const double t = floor((x - g.lo[a]) / g.cell);
  const double top = (double)(g.G[a] - 1);
  return !(t >= 0.0) ? 0 : (t > top ? g.G[a] - 1 : (int)t);
}

__device__ __forceinline__ double plane_of(const Grid& g, int a, int k) { return g.lo[a] + (double)k * g.cell; }

// cell_of and plane_of for a caller that holds the axis' lo and G in registers of its own: the same operations
__device__ __forceinline__ int cell_at(double lo, double cell, int G, double x) {
  const double t = floor((x - lo) / cell);
  const double top = (double)(G - 1);
  return !(t >= 0.0) ? 0 : (t > top ? G - 1 : (int)t);
}

__device__ __forceinline__ double plane_at(double lo, double cell, int k) { return lo + (double)k * cell; }

// the grid of a call, or false
inline bool make_grid(const float* lo, double cell, const int* dims, Grid* g) {
  if (!lo || !dims || !(cell > 0.0 && cell <= DBL_MAX)) return false;
  for (int a = 0; a < 3; a++) {
    if (!(std::fabs(lo[a]) <= FLT_MAX) || dims[a] < 1 || dims[a] > kGridAxis) return false;
    g->lo[a] = (double)lo[a];
    g->G[a] = dims[a];
  }
  g->cell = cell;
  return true;
}

}  // namespace mesh_distance
}  // namespace gigs
