// mesh_atlas.hip -- texturing a light mesh from a heavy one: the surface point of every texel of an atlas of equal per-face
// charts, and the closest point of a query on a given triangle as barycentric weights, with the per-vertex channels of that
// triangle interpolated there.  include/gigs_hip.h, "Texturing meshes", states every quantity and tests/mesh_atlas_ref.py
// restates them in numpy.  The search between the two kernels is gigs_mesh_closest (mesh.bake_atlas).
//
//   determinism   One independent thread per texel or query; no thread waits on another and there is no float atomic.  A
//                 texel of the atlas belongs to one face, so no two threads store to one address.  The two counters are
//                 integer atomics.  float64 on the float32 inputs, + - * / only, no sqrt, no transcendental; the library
//                 is built with -ffp-contract=off (build.py): no product below is fused into a sum, in any run.
//   addresses     A face or vertex index, a destination texel and a texel's place in the image are compared with their
//                 ranges before they are used; a violation that mesh.py cannot produce sets *overflow and the thread
//                 stores nothing (gigs_mesh_compact's convention).
//   closest       triangle_closest<true> (mesh_triangle.h) is the routine the search calls as triangle_closest<false>, with
//                 the weights kept: one definition of the candidates, expressions and order, so the d^2 that decides
//                 between the candidates has the bits the search compared.
//   registers     The weights and corners live in named scalars and fixed-size arrays with compile-time indices; the
//                 channel loop reads and writes memory only.  No scratch.
#include "mesh_triangle.h"  // triangle_closest; through it mesh_grid.h: the per-thread and vector helpers

namespace gigs {
namespace mesh_atlas {

using namespace gigs::mesh_common;  // item, in_range, finite3, load3, blocks_for, triangle_closest

// ---- texel -> surface point --------------------------------------------------------------------------------------------------
struct PointsArgs {
  int V, F, B, W, H, per_row, n_texels;  // n_texels = n_blocks B (B + 1)
  const float* vertices;
  const int* faces;
  float *points, *bary;
  int* texel_face;
  long long* dest;
  int* overflow;
};

__global__ __launch_bounds__(256) void points_kernel(PointsArgs a) {
  const int q = item<256>(a.n_texels);
  if (q < 0) return;
  const int B = a.B, per_block = B * (B + 1);
  const int blk = q / per_block, r = q - blk * per_block;
  const int j = r / (B + 1), i = r - j * (B + 1);
  const int x = (blk % a.per_row) * (B + 1) + i, y = (blk / a.per_row) * B + j;
  if (x >= a.W || y >= a.H) {  // only with a layout that is not atlas_layout's
    *a.overflow = 1;
    return;
  }
  const int half = i + j <= B - 1 ? 0 : 1;
  const int f = 2 * blk + half;
  const int li = half ? B - i : i, lj = half ? B - 1 - j : j;  // the upper half is the point reflection of the lower
  const double w1 = (double)li / (double)(B - 2), w2 = (double)lj / (double)(B - 2);
  const double w0 = (1.0 - w1) - w2;
  a.bary[2 * (size_t)q] = (float)w1;
  a.bary[2 * (size_t)q + 1] = (float)w2;
  float out[3] = {NAN, NAN, NAN};
  long long d = -1;
  int tf = -1;
  if (f < a.F) {
    tf = f;
    const int ia = a.faces[3 * (size_t)f], ib = a.faces[3 * (size_t)f + 1], ic = a.faces[3 * (size_t)f + 2];
    if (in_range(ia, ib, ic, a.V)) {  // else never dereferenced
      double p0[3], p1[3], p2[3];
      load3(a.vertices, ia, p0);
      load3(a.vertices, ib, p1);
      load3(a.vertices, ic, p2);
      if (finite3(p0) && finite3(p1) && finite3(p2)) {
#pragma unroll
        for (int c = 0; c < 3; c++) out[c] = (float)((w0 * p0[c] + w1 * p1[c]) + w2 * p2[c]);
        d = (long long)y * a.W + x;
      }
    }
  }
  a.points[3 * (size_t)q] = out[0];
  a.points[3 * (size_t)q + 1] = out[1];
  a.points[3 * (size_t)q + 2] = out[2];
  a.texel_face[q] = tf;
  a.dest[q] = d;
}

// ---- channels at the closest point of a given triangle ----------------------------------------------------------------------
struct TransferArgs {
  int V, F, C, N;
  const float* vertices;
  const int* faces;
  const float *values, *points;
  const int* face;
  const long long* dest;
  long long plane;
  float* out;
  unsigned char* coverage;
  float* bary;
  unsigned long long* counts;
  int* overflow;
};

__global__ __launch_bounds__(256) void transfer_kernel(TransferArgs a) {
  const int q = item<256>(a.N);
  if (q < 0) return;
  const int f = a.face[q];
  const long long d = a.dest ? a.dest[q] : (long long)q;
  if (f >= a.F || f < -1 || d < -1 || (a.dest && d >= a.plane)) {
    *a.overflow = 1;
    return;
  }
  if (f < 0 || d < 0) {
    atomicAdd(a.counts + 1, 1ULL);
    return;
  }
  const int i0 = a.faces[3 * (size_t)f], i1 = a.faces[3 * (size_t)f + 1], i2 = a.faces[3 * (size_t)f + 2];
  if (!in_range(i0, i1, i2, a.V)) {
    *a.overflow = 1;
    return;
  }
  double p[3], p0[3], p1[3], p2[3];
  load3(a.points, q, p);
  load3(a.vertices, i0, p0);
  load3(a.vertices, i1, p1);
  load3(a.vertices, i2, p2);
  if (!(finite3(p) && finite3(p0) && finite3(p1) && finite3(p2))) {
    atomicAdd(a.counts + 1, 1ULL);
    return;
  }
  double w0, w1, w2;
  triangle_closest<true>(p, i0, i1, i2, p0, p1, p2, &w0, &w1, &w2);
  a.bary[2 * (size_t)q] = (float)w1;
  a.bary[2 * (size_t)q + 1] = (float)w2;
  const float *v0 = a.values + (size_t)i0 * a.C, *v1 = a.values + (size_t)i1 * a.C, *v2 = a.values + (size_t)i2 * a.C;
  if (a.dest) {
    for (int c = 0; c < a.C; c++)
      a.out[(size_t)c * (size_t)a.plane + (size_t)d] = (float)((w0 * (double)v0[c] + w1 * (double)v1[c]) + w2 * (double)v2[c]);
    a.coverage[d] = 1;
  } else {
    for (int c = 0; c < a.C; c++)
      a.out[(size_t)q * a.C + c] = (float)((w0 * (double)v0[c] + w1 * (double)v1[c]) + w2 * (double)v2[c]);
  }
  atomicAdd(a.counts, 1ULL);
}

}  // namespace mesh_atlas
}  // namespace gigs

extern "C" {

int gigs_mesh_atlas_points(int n_vertices, int n_faces, const float* vertices, const int* faces, int block, int width, int height,
                           int n_blocks, float* points, float* bary, int* texel_face, long long* dest, int* overflow,
                           void* stream) {
  using namespace gigs::mesh_atlas;
  if (n_vertices < 0 || n_faces < 0 || n_blocks < 0 || block < 3 || block > 1024 || width < block + 1 || height < 0 || !overflow ||
      (n_faces > 0 && !faces) || (n_vertices > 0 && !vertices))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_atlas_points: bad argument");
  const long long texels = (long long)n_blocks * block * (block + 1);
  if (texels > 0x7fffffffLL || (long long)width * height > (1LL << 40))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_atlas_points: the atlas is too large");
  if (texels == 0) return 0;
  if (!points || !bary || !texel_face || !dest) return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_atlas_points: NULL array");
  PointsArgs a;
  a.V = n_vertices, a.F = n_faces, a.B = block, a.W = width, a.H = height, a.per_row = width / (block + 1);
  a.n_texels = (int)texels;
  a.vertices = vertices, a.faces = faces, a.points = points, a.bary = bary, a.texel_face = texel_face, a.dest = dest;
  a.overflow = overflow;
  hipLaunchKernelGGL(points_kernel, dim3(blocks_for(a.n_texels)), dim3(256), 0, (hipStream_t)stream, a);
  return gigs_internal_check_launch("mesh_atlas_points");
}

int gigs_mesh_transfer(int n_vertices, int n_faces, const float* vertices, const int* faces, int n_channels, const float* values,
                       int n_points, const float* points, const int* face, const long long* dest, long long plane, float* out,
                       unsigned char* coverage, float* bary, unsigned long long* counts, int* overflow, void* stream) {
  using namespace gigs::mesh_atlas;
  if (n_vertices < 0 || n_faces < 0 || n_points < 0 || n_channels < 1 || n_channels > 16 || !counts || !overflow ||
      (dest && (plane < 0 || !coverage)))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_transfer: bad argument");
  hipStream_t s = (hipStream_t)stream;
  if (hipMemsetAsync(counts, 0, 2 * sizeof(unsigned long long), s) != hipSuccess)
    return gigs_internal_fail(GIGS_ERR_HIP, "mesh_transfer: clear failed");
  if (n_points == 0) return 0;
  if (!points || !face || !out || !bary || (n_faces > 0 && (!faces || !vertices || !values)))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_transfer: NULL array");
  TransferArgs a;
  a.V = n_vertices, a.F = n_faces, a.C = n_channels, a.N = n_points;
  a.vertices = vertices, a.faces = faces, a.values = values, a.points = points, a.face = face, a.dest = dest;
  a.plane = plane, a.out = out, a.coverage = coverage, a.bary = bary, a.counts = counts, a.overflow = overflow;
  hipLaunchKernelGGL(transfer_kernel, dim3(blocks_for(n_points)), dim3(256), 0, s, a);
  return gigs_internal_check_launch("mesh_transfer");
}
}  // extern "C"
