// mesh.hip -- a trained scene as a mesh: TSDF fusion of rendered planes, then naive surface nets.
//
// The volume is a regular grid of samples s(i,j,k) = lo + (i,j,k) h, x fastest, all fp32 and addressed with size_t:
// tsdf [G] (initially 1) and weight [G] (0), the pair every view touches, apart from the cold block attr_weight [G] and
// attr [8][G] (planar: world normal xyz, albedo rgb, roughness, metallic) that only samples within the truncation band
// of a surface touch.  Kernels:
//   integrate_kernel     one thread owns one sample (linear index, lanes along x: loads and stores coalesce), no atomics,
//                        so the result is deterministic.  A launch applies 1..8 views in order with the sample's state
//                        in registers; the views (matrix, focal lengths, size, six plane pointers) are a by-value
//                        kernel argument, read with scalar loads because the view index is wave-uniform.  The cold
//                        block is loaded on a sample's first attribute update and stored only if it was loaded; tsdf /
//                        weight are stored only if a view touched them.  Every product and sum is rounded on its own
//                        (-ffp-contract=off), division is IEEE: the arithmetic is the header's, operation by operation,
//                        and n views in one launch equal n launches of one view bit for bit (fp32 state round-trips).
//   count_cells_kernel   flag of every cell (samples (i..i+1, j..j+1, k..k+1)): 1 = active (all eight weights >=
//                        min_weight and the signs of tsdf differ; tsdf < 0 is inside)
//   count_quads_kernel   per sample, the number (0..3) of its +x / +y / +z edges that get a quad (ends differ in sign,
//                        the four cells around the edge exist and are valid)
//   write_vertices_kernel / write_faces_kernel   the same predicates again, behind exclusive scans of the two count
//                        arrays (the caller's): one vertex per active cell in ascending cell index, two triangles per
//                        quad ordered by (sample index, axis).  Both take the capacities of their outputs: an index
//                        beyond a capacity sets *overflow and stores nothing.
#include "gigs_internal.h"

namespace gigs {
namespace mesh {

#define GIGS_GLOBAL __attribute__((address_space(1)))
typedef GIGS_GLOBAL const float gfloat;

constexpr float kNear = 0.2f;  // the rasterizer's near cull (preprocess: p_view.z <= 0.2)

struct ViewK {
  float m[16];
  float fx, fy, cx, cy;
  int W, H;
  const float *opacity, *depth, *normal, *albedo, *roughness, *metallic;
};
struct ViewsK {
  ViewK v[GIGS_TSDF_MAX_VIEWS];
};

struct GridK {
  float lox, loy, loz, h;
  int Gx, Gy, Gz;
  float trunc, opacity_min;
  int carve;
};

__global__ __launch_bounds__(256) void integrate_kernel(GridK g, int n_views, ViewsK views, float* __restrict__ tsdf,
                                                        float* __restrict__ weight, float* __restrict__ attr_weight,
                                                        float* __restrict__ attr) {
  const size_t total = (size_t)g.Gx * g.Gy * g.Gz;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const unsigned row = (unsigned)(idx / (unsigned)g.Gx);
  const int i = (int)(idx - (size_t)row * g.Gx);
  const int k = (int)(row / (unsigned)g.Gy), j = (int)(row - (unsigned)k * g.Gy);
  const v3 s = {g.lox + (float)i * g.h, g.loy + (float)j * g.h, g.loz + (float)k * g.h};

  float t = tsdf[idx], w = weight[idx];
  float aw = 0.0f, a[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  bool touched = false, cold = false;

  for (int n = 0; n < n_views; n++) {
    const ViewK& V = views.v[n];
    const v3 p = xform_point_4x3(s, V.m);
    if (!(p.z > kNear)) continue;
    const float u = p.x / p.z * V.fx + V.cx;
    const float v = p.y / p.z * V.fy + V.cy;
    const float fu = floorf(u + 0.5f), fv = floorf(v + 0.5f);
    if (!(fu >= 0.0f && fu < (float)V.W && fv >= 0.0f && fv < (float)V.H)) continue;  // NaN skips too
    const size_t plane = (size_t)V.W * V.H;
    const size_t pix = (size_t)(int)fv * V.W + (int)fu;  // 0 <= pix < plane by the test above
    const float O = ((gfloat*)V.opacity)[pix];
    const bool bg = O < g.opacity_min;
    float d = 1.0f, sdf = 0.0f;
    if (bg) {
      if (!g.carve) continue;
    } else {
      sdf = ((gfloat*)V.depth)[pix] - p.z;
      if (!(sdf >= -g.trunc)) continue;  // behind the surface by more than the band (and a NaN depth)
      d = fminf(1.0f, sdf / g.trunc);
    }
    t = (t * w + d) / (w + 1.0f);
    w = w + 1.0f;
    touched = true;
    if (!bg && sdf <= g.trunc) {
      if (!cold) {
        cold = true;
        aw = attr_weight[idx];
#pragma unroll
        for (int c = 0; c < 8; c++) a[c] = attr[(size_t)c * total + idx];
      }
      gfloat* nrm = (gfloat*)V.normal + pix;
      gfloat* alb = (gfloat*)V.albedo + pix;
      const float x[8] = {nrm[0], nrm[plane], nrm[2 * plane], alb[0], alb[plane], alb[2 * plane],
                          ((gfloat*)V.roughness)[pix], ((gfloat*)V.metallic)[pix]};
#pragma unroll
      for (int c = 0; c < 8; c++) a[c] = (a[c] * aw + x[c]) / (aw + 1.0f);
      aw = aw + 1.0f;
    }
  }
  if (touched) {
    tsdf[idx] = t;
    weight[idx] = w;
  }
  if (cold) {
    attr_weight[idx] = aw;
#pragma unroll
    for (int c = 0; c < 8; c++) attr[(size_t)c * total + idx] = a[c];
  }
}

// ---- surface nets --------------------------------------------------------------------------------------------------
// The 12 edges of a cell in their fixed order: the four along x, the four along y, the four along z; within an axis the
// other two coordinates of the edge's first corner run (0,0), (1,0), (0,1), (1,1) with the lower axis first.
// kEdge[e] = {dx, dy, dz of the first corner, axis}.
__constant__ const int kEdge[12][4] = {{0, 0, 0, 0}, {0, 1, 0, 0}, {0, 0, 1, 0}, {0, 1, 1, 0},
                                       {0, 0, 0, 1}, {1, 0, 0, 1}, {0, 0, 1, 1}, {1, 0, 1, 1},
                                       {0, 0, 0, 2}, {1, 0, 0, 2}, {0, 1, 0, 2}, {1, 1, 0, 2}};

struct Dims {
  int Gx, Gy, Gz;
  __device__ __forceinline__ size_t sample(int i, int j, int k) const { return ((size_t)k * Gy + j) * Gx + i; }
  __device__ __forceinline__ size_t cell(int i, int j, int k) const { return ((size_t)k * (Gy - 1) + j) * (Gx - 1) + i; }
};

// all eight samples of cell (i,j,k) have weight >= min_weight; the cell must exist
__device__ __forceinline__ bool cell_valid(const Dims& D, const float* __restrict__ weight, float min_weight, int i, int j, int k) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 8; c++) ok = ok && weight[D.sample(i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2))] >= min_weight;
  return ok;
}

__device__ __forceinline__ bool cell_active(const Dims& D, const float* __restrict__ tsdf, const float* __restrict__ weight,
                                            float min_weight, int i, int j, int k) {
  if (!cell_valid(D, weight, min_weight, i, j, k)) return false;
  int inside = 0;
#pragma unroll
  for (int c = 0; c < 8; c++) inside += tsdf[D.sample(i + (c & 1), j + ((c >> 1) & 1), k + (c >> 2))] < 0.0f ? 1 : 0;
  return inside != 0 && inside != 8;
}

__global__ __launch_bounds__(256) void count_cells_kernel(Dims D, float min_weight, const float* __restrict__ tsdf,
                                                          const float* __restrict__ weight, int* __restrict__ flags) {
  const size_t cells = (size_t)(D.Gx - 1) * (D.Gy - 1) * (D.Gz - 1);
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= cells) return;
  const unsigned row = (unsigned)(idx / (unsigned)(D.Gx - 1));
  const int i = (int)(idx - (size_t)row * (D.Gx - 1));
  const int k = (int)(row / (unsigned)(D.Gy - 1)), j = (int)(row - (unsigned)k * (D.Gy - 1));
  flags[idx] = cell_active(D, tsdf, weight, min_weight, i, j, k) ? 1 : 0;
}

// the quad of the edge from sample (i,j,k) along `axis`: its four cells, counter-clockwise as seen from the + end of
// the axis (the two other axes u, v with axis = u x v: cells (-1,-1), (0,-1), (0,0), (-1,0) in (u,v)).  False if the
// ends do not differ in sign or one of the cells does not exist or is not valid.
__device__ __forceinline__ bool edge_quad(const Dims& D, const float* __restrict__ tsdf, const float* __restrict__ weight,
                                          float min_weight, int i, int j, int k, int axis, size_t (&cells)[4], bool& flip) {
  const int G[3] = {D.Gx, D.Gy, D.Gz};
  const int p[3] = {i, j, k};
  const int u = (axis + 1) % 3, v = (axis + 2) % 3;
  if (p[axis] + 1 >= G[axis] || p[u] < 1 || p[u] + 1 >= G[u] || p[v] < 1 || p[v] + 1 >= G[v]) return false;
  int q[3] = {i, j, k};
  q[axis] += 1;
  const bool in0 = tsdf[D.sample(i, j, k)] < 0.0f, in1 = tsdf[D.sample(q[0], q[1], q[2])] < 0.0f;
  if (in0 == in1) return false;
  const int du[4] = {-1, 0, 0, -1}, dv[4] = {-1, -1, 0, 0};
#pragma unroll
  for (int c = 0; c < 4; c++) {
    int r[3] = {i, j, k};
    r[u] += du[c];
    r[v] += dv[c];
    if (!cell_valid(D, weight, min_weight, r[0], r[1], r[2])) return false;
    cells[c] = D.cell(r[0], r[1], r[2]);
  }
  flip = !in0;  // the outside (positive) end is the sample itself: seen from there the order above is clockwise
  return true;
}

__global__ __launch_bounds__(256) void count_quads_kernel(Dims D, float min_weight, const float* __restrict__ tsdf,
                                                          const float* __restrict__ weight, int* __restrict__ counts) {
  const size_t total = (size_t)D.Gx * D.Gy * D.Gz;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const unsigned row = (unsigned)(idx / (unsigned)D.Gx);
  const int i = (int)(idx - (size_t)row * D.Gx);
  const int k = (int)(row / (unsigned)D.Gy), j = (int)(row - (unsigned)k * D.Gy);
  int n = 0;
  size_t cells[4];
  bool flip;
  for (int axis = 0; axis < 3; axis++) n += edge_quad(D, tsdf, weight, min_weight, i, j, k, axis, cells, flip) ? 1 : 0;
  counts[idx] = n;
}

__global__ __launch_bounds__(256) void write_vertices_kernel(Dims D, float lox, float loy, float loz, float h, float min_weight,
                                                             const float* __restrict__ tsdf, const float* __restrict__ weight,
                                                             const float* __restrict__ attr_weight, const float* __restrict__ attr,
                                                             const int* __restrict__ cell_offsets, int capacity,
                                                             float* __restrict__ vertices, float* __restrict__ normals,
                                                             float* __restrict__ albedo, float* __restrict__ roughness,
                                                             float* __restrict__ metallic, int* __restrict__ overflow) {
  const size_t cells = (size_t)(D.Gx - 1) * (D.Gy - 1) * (D.Gz - 1);
  const size_t total = (size_t)D.Gx * D.Gy * D.Gz;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= cells) return;
  const unsigned row = (unsigned)(idx / (unsigned)(D.Gx - 1));
  const int i = (int)(idx - (size_t)row * (D.Gx - 1));
  const int k = (int)(row / (unsigned)(D.Gy - 1)), j = (int)(row - (unsigned)k * (D.Gy - 1));
  if (!cell_active(D, tsdf, weight, min_weight, i, j, k)) return;
  const int out = cell_offsets[idx];
  if (out < 0 || out >= capacity) {
    *overflow = 1;
    return;
  }
  float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f, sa[8] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  int n = 0;
  for (int e = 0; e < 12; e++) {
    const int dx = kEdge[e][0], dy = kEdge[e][1], dz = kEdge[e][2], axis = kEdge[e][3];
    const size_t s0 = D.sample(i + dx, j + dy, k + dz);
    const size_t s1 = D.sample(i + dx + (axis == 0), j + dy + (axis == 1), k + dz + (axis == 2));
    const float f0 = tsdf[s0], f1 = tsdf[s1];
    if ((f0 < 0.0f) == (f1 < 0.0f)) continue;
    const float t = f0 / (f0 - f1);
    sx = sx + ((float)dx + (axis == 0 ? t : 0.0f));
    sy = sy + ((float)dy + (axis == 1 ? t : 0.0f));
    sz = sz + ((float)dz + (axis == 2 ? t : 0.0f));
    n++;
    const float w0 = attr_weight[s0] == 0.0f ? 0.0f : 1.0f - t;
    const float w1 = attr_weight[s1] == 0.0f ? 0.0f : t;
    sw = sw + w0;
    sw = sw + w1;
#pragma unroll
    for (int c = 0; c < 8; c++) {
      sa[c] = sa[c] + w0 * attr[(size_t)c * total + s0];
      sa[c] = sa[c] + w1 * attr[(size_t)c * total + s1];
    }
  }
  const float fn = (float)n;  // n >= 1: an active cell has an edge whose ends differ in sign
  vertices[3 * (size_t)out + 0] = lox + ((float)i + sx / fn) * h;
  vertices[3 * (size_t)out + 1] = loy + ((float)j + sy / fn) * h;
  vertices[3 * (size_t)out + 2] = loz + ((float)k + sz / fn) * h;
  float r[8];
#pragma unroll
  for (int c = 0; c < 8; c++) r[c] = sw > 0.0f ? sa[c] / sw : 0.0f;
  const float len = sqrtf(r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
#pragma unroll
  for (int c = 0; c < 3; c++) normals[3 * (size_t)out + c] = len > 0.0f ? r[c] / len : 0.0f;
#pragma unroll
  for (int c = 0; c < 3; c++) albedo[3 * (size_t)out + c] = r[3 + c];
  roughness[out] = r[6];
  metallic[out] = r[7];
}

__global__ __launch_bounds__(256) void write_faces_kernel(Dims D, float min_weight, const float* __restrict__ tsdf,
                                                          const float* __restrict__ weight, const int* __restrict__ cell_offsets,
                                                          const int* __restrict__ quad_offsets, int vertex_capacity,
                                                          int face_capacity, int* __restrict__ faces, int* __restrict__ overflow) {
  const size_t total = (size_t)D.Gx * D.Gy * D.Gz;
  const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const unsigned row = (unsigned)(idx / (unsigned)D.Gx);
  const int i = (int)(idx - (size_t)row * D.Gx);
  const int k = (int)(row / (unsigned)D.Gy), j = (int)(row - (unsigned)k * D.Gy);
  long long quad = quad_offsets[idx];
  for (int axis = 0; axis < 3; axis++) {
    size_t cells[4];
    bool flip;
    if (!edge_quad(D, tsdf, weight, min_weight, i, j, k, axis, cells, flip)) continue;
    const long long f = 2 * quad;
    quad++;
    int a = cell_offsets[cells[0]], b = cell_offsets[cells[1]], c = cell_offsets[cells[2]], d = cell_offsets[cells[3]];
    if (f < 0 || f + 2 > (long long)face_capacity || a < 0 || a >= vertex_capacity || b < 0 || b >= vertex_capacity || c < 0 ||
        c >= vertex_capacity || d < 0 || d >= vertex_capacity) {
      *overflow = 1;
      continue;
    }
    if (flip) {
      const int tmp = b;
      b = d;
      d = tmp;
    }
    int* o = faces + 3 * (size_t)f;  // the diagonal is a-c
    o[0] = a; o[1] = b; o[2] = c;
    o[3] = a; o[4] = c; o[5] = d;
  }
}

inline bool grid_ok(const gigs_tsdf_grid* g) {
  if (!g) return false;
  for (int c = 0; c < 3; c++)
    if (g->dims[c] < 1 || g->dims[c] > GIGS_TSDF_MAX_AXIS) return false;
  return (long long)g->dims[0] * g->dims[1] * g->dims[2] < (1ll << 31) && g->voxel > 0.0f && g->tsdf && g->weight &&
         g->attr_weight && g->attr;
}

inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace mesh
}  // namespace gigs

extern "C" {

int gigs_tsdf_integrate(const gigs_tsdf_grid* grid, int n_views, const gigs_tsdf_view* views, void* stream) {
  using namespace gigs::mesh;
  if (n_views == 0) return 0;
  if (!grid_ok(grid) || n_views < 0 || n_views > GIGS_TSDF_MAX_VIEWS || !views || !(grid->trunc > 0.0f))
    return gigs_internal_fail(GIGS_ERR_INVALID, "tsdf_integrate: bad argument");
  ViewsK vk = {};
  for (int n = 0; n < n_views; n++) {
    const gigs_tsdf_view& s = views[n];
    if (s.width < 1 || s.height < 1 || !(s.tanfovx > 0.0f) || !(s.tanfovy > 0.0f) || !s.opacity || !s.depth || !s.normal ||
        !s.albedo || !s.roughness || !s.metallic)
      return gigs_internal_fail(GIGS_ERR_INVALID, "tsdf_integrate: bad view");
    ViewK& d = vk.v[n];
    for (int c = 0; c < 16; c++) d.m[c] = s.viewmatrix[c];
    d.fx = (float)s.width / (2.0f * s.tanfovx);
    d.fy = (float)s.height / (2.0f * s.tanfovy);
    d.cx = (float)(s.width - 1) / 2.0f;
    d.cy = (float)(s.height - 1) / 2.0f;
    d.W = s.width;
    d.H = s.height;
    d.opacity = s.opacity; d.depth = s.depth; d.normal = s.normal;
    d.albedo = s.albedo; d.roughness = s.roughness; d.metallic = s.metallic;
  }
  const GridK g = {grid->lo[0], grid->lo[1], grid->lo[2], grid->voxel, grid->dims[0], grid->dims[1], grid->dims[2],
                   grid->trunc, grid->opacity_min, grid->carve};
  const size_t total = (size_t)g.Gx * g.Gy * g.Gz;
  hipLaunchKernelGGL(integrate_kernel, dim3(blocks_for(total)), dim3(256), 0, (hipStream_t)stream, g, n_views, vk, grid->tsdf,
                     grid->weight, grid->attr_weight, grid->attr);
  return gigs_internal_check_launch("tsdf_integrate");
}

int gigs_mesh_count(const gigs_tsdf_grid* grid, float min_weight, int* cell_flags, int* sample_quads, void* stream) {
  using namespace gigs::mesh;
  if (!grid_ok(grid) || !cell_flags || !sample_quads) return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_count: bad argument");
  const Dims D = {grid->dims[0], grid->dims[1], grid->dims[2]};
  const size_t cells = (size_t)(D.Gx - 1) * (D.Gy - 1) * (D.Gz - 1);
  if (cells == 0) return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_count: a grid without cells");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(count_cells_kernel, dim3(blocks_for(cells)), dim3(256), 0, s, D, min_weight, grid->tsdf, grid->weight,
                     cell_flags);
  hipLaunchKernelGGL(count_quads_kernel, dim3(blocks_for((size_t)D.Gx * D.Gy * D.Gz)), dim3(256), 0, s, D, min_weight,
                     grid->tsdf, grid->weight, sample_quads);
  return gigs_internal_check_launch("mesh_count");
}

int gigs_mesh_write(const gigs_tsdf_grid* grid, float min_weight, const int* cell_offsets, const int* quad_offsets,
                    int vertex_capacity, int face_capacity, float* vertices, float* normals, float* albedo, float* roughness,
                    float* metallic, int* faces, int* overflow, void* stream) {
  using namespace gigs::mesh;
  if (!grid_ok(grid) || !cell_offsets || !quad_offsets || vertex_capacity < 0 || face_capacity < 0 || !overflow)
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_write: bad argument");
  const Dims D = {grid->dims[0], grid->dims[1], grid->dims[2]};
  const size_t cells = (size_t)(D.Gx - 1) * (D.Gy - 1) * (D.Gz - 1);
  if (cells == 0) return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_write: a grid without cells");
  if (vertex_capacity > 0 && (!vertices || !normals || !albedo || !roughness || !metallic))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_write: NULL vertex output");
  if (face_capacity > 0 && !faces) return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_write: NULL face output");
  hipStream_t s = (hipStream_t)stream;
  hipLaunchKernelGGL(write_vertices_kernel, dim3(blocks_for(cells)), dim3(256), 0, s, D, grid->lo[0], grid->lo[1], grid->lo[2],
                     grid->voxel, min_weight, grid->tsdf, grid->weight, grid->attr_weight, grid->attr, cell_offsets,
                     vertex_capacity, vertices, normals, albedo, roughness, metallic, overflow);
  hipLaunchKernelGGL(write_faces_kernel, dim3(blocks_for((size_t)D.Gx * D.Gy * D.Gz)), dim3(256), 0, s, D, min_weight,
                     grid->tsdf, grid->weight, cell_offsets, quad_offsets, vertex_capacity, face_capacity, faces, overflow);
  return gigs_internal_check_launch("mesh_write");
}
}  // extern "C"
