// mesh_raster.hip -- a triangle mesh as the G-buffer planes the deferred chain reads: a visibility-buffer rasterizer.
//
// Three stages, each a C-ABI call (include/gigs_hip.h states the arithmetic).  Nothing sorts or bins, and no result
// depends on the order threads run in: coverage is an integer decision on 24.8 fixed-point screen coordinates, and
// visibility is the minimum of a 64-bit key over the covering triangles.
//   project_kernel       one thread per vertex: view-space position, fixed-point screen position, cull flag
//   raster_small_kernel  one thread per triangle.  A triangle whose clamped box holds <= small_max pixel centres is walked by
//                        its thread; a larger one is appended to a device list (atomic counter)
//   raster_large_kernel  a fixed grid of waves strides over that list (the count is read on the device): one wave per
//                        triangle, lanes over the box
//   resolve_kernel       one thread per pixel: the winner's attributes, perspective-correct, or the blend kernel's background
//   resolve_textured_kernel  the same pixel, the same key: materials (and the normal) looked up bilinearly in the planes of a
//                        texture atlas at the perspective-correct UV of the face's corners, 36 independent gathers
// Both raster kernels and the resolve go through tri_setup / tri_sample, so the depth in a key and the depth plane have the
// same bits, and both paths and any small_max give the same visibility buffer.  No clipping: a triangle with a vertex
// behind the near cull (or outside the guard band) is dropped whole.
#include "gigs_internal.h"

namespace gigs {
namespace mesh_raster {

constexpr float kNear = 0.2f;          // the rasterizer's near cull (preprocess: p_view.z <= 0.2)
constexpr float kGuard = 16384.0f;     // pixels: |X| <= 2^22, edge functions below 2^48
constexpr int kSub = 256;              // sub-pixel steps per pixel
constexpr unsigned long long kEmpty = ~0ull;
constexpr int kLargeBlocks = 512;      // the second launch's fixed grid: 2048 waves

struct ProjK {
  float fx, fy, cx, cy;
};

__global__ __launch_bounds__(256) void project_kernel(int V, ProjK k, const float* __restrict__ vertices,
                                                      const float* __restrict__ viewmatrix, float* __restrict__ view_pos,
                                                      int* __restrict__ screen, uint8_t* __restrict__ flags) {
  const int idx = blockIdx.x * 256 + threadIdx.x;
  if (idx >= V) return;
  const v3 s = {vertices[3 * (size_t)idx], vertices[3 * (size_t)idx + 1], vertices[3 * (size_t)idx + 2]};
  const v3 p = xform_point_4x3(s, viewmatrix);
  const float u = p.x / p.z * k.fx + k.cx;
  const float v = p.y / p.z * k.fy + k.cy;
  // NaN fails every comparison; an infinite p.z gives a finite u and is caught by its own test
  const bool ok = p.z > kNear && isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && fabsf(u) <= kGuard && fabsf(v) <= kGuard;
  view_pos[3 * (size_t)idx] = p.x;
  view_pos[3 * (size_t)idx + 1] = p.y;
  view_pos[3 * (size_t)idx + 2] = p.z;
  screen[2 * (size_t)idx] = ok ? (int)rintf(u * (float)kSub) : 0;
  screen[2 * (size_t)idx + 1] = ok ? (int)rintf(v * (float)kSub) : 0;
  flags[idx] = ok ? 0 : 1;
}

struct MeshK {
  int V, F, W, H;
  const int* faces;
  const float* view_pos;
  const int* screen;
  const uint8_t* flags;
};

// A triangle ready to be sampled: vertices in counter-clockwise order of the screen integers (A > 0), 1 / z per vertex.
struct Tri {
  int v[3];
  int X[3], Y[3];
  float iz[3];
  float fA;
  bool flip;  // vertices 1 and 2 swapped roles: what is stored per face CORNER (the UVs) swaps with them
};

// False for a triangle that is dropped: an index outside [0, V), a flagged vertex, zero area.  Nothing is read through a
// bad index.
__device__ __forceinline__ bool tri_setup(const MeshK& m, unsigned t, Tri& T) {
  int i0 = m.faces[3 * (size_t)t], i1 = m.faces[3 * (size_t)t + 1], i2 = m.faces[3 * (size_t)t + 2];
  if ((unsigned)i0 >= (unsigned)m.V || (unsigned)i1 >= (unsigned)m.V || (unsigned)i2 >= (unsigned)m.V) return false;
  if ((m.flags[i0] | m.flags[i1] | m.flags[i2]) != 0) return false;
  const int X0 = m.screen[2 * (size_t)i0], Y0 = m.screen[2 * (size_t)i0 + 1];
  int X1 = m.screen[2 * (size_t)i1], Y1 = m.screen[2 * (size_t)i1 + 1];
  int X2 = m.screen[2 * (size_t)i2], Y2 = m.screen[2 * (size_t)i2 + 1];
  long long A = (long long)(X1 - X0) * (long long)(Y2 - Y0) - (long long)(Y1 - Y0) * (long long)(X2 - X0);
  if (A == 0) return false;
  const bool flip = A < 0;
  if (flip) {  // vertices 1 and 2 swap roles
    int tmp = i1; i1 = i2; i2 = tmp;
    tmp = X1; X1 = X2; X2 = tmp;
    tmp = Y1; Y1 = Y2; Y2 = tmp;
    A = -A;
  }
  T.v[0] = i0; T.v[1] = i1; T.v[2] = i2;
  T.X[0] = X0; T.X[1] = X1; T.X[2] = X2;
  T.Y[0] = Y0; T.Y[1] = Y1; T.Y[2] = Y2;
  T.iz[0] = 1.0f / m.view_pos[3 * (size_t)i0 + 2];
  T.iz[1] = 1.0f / m.view_pos[3 * (size_t)i1 + 2];
  T.iz[2] = 1.0f / m.view_pos[3 * (size_t)i2 + 2];
  T.fA = (float)A;
  T.flip = flip;
  return true;
}

// the edge function of the directed edge a -> b at q, and whether q belongs to the triangle on that edge's side
__device__ __forceinline__ bool edge_in(int Xa, int Ya, int Xb, int Yb, int qx, int qy, long long& E) {
  const int dx = Xb - Xa, dy = Yb - Ya;
  E = (long long)dx * (long long)(qy - Ya) - (long long)dy * (long long)(qx - Xa);
  return E > 0 || (E == 0 && (dy < 0 || (dy == 0 && dx > 0)));
}

struct Sample {
  float w0, w1, w2, s, z;
};

// Pixel (i, j): false if its centre is not covered or its depth is unusable.
__device__ __forceinline__ bool tri_sample(const Tri& T, int i, int j, Sample& S) {
  const int qx = i * kSub, qy = j * kSub;
  long long E0, E1, E2;
  const bool in0 = edge_in(T.X[1], T.Y[1], T.X[2], T.Y[2], qx, qy, E0);
  const bool in1 = edge_in(T.X[2], T.Y[2], T.X[0], T.Y[0], qx, qy, E1);
  const bool in2 = edge_in(T.X[0], T.Y[0], T.X[1], T.Y[1], qx, qy, E2);
  if (!(in0 && in1 && in2)) return false;
  const float b0 = (float)E0 / T.fA, b1 = (float)E1 / T.fA, b2 = (float)E2 / T.fA;
  S.w0 = b0 * T.iz[0];
  S.w1 = b1 * T.iz[1];
  S.w2 = b2 * T.iz[2];
  S.s = (S.w0 + S.w1) + S.w2;
  S.z = 1.0f / S.s;
  return S.z > 0.0f && isfinite(S.z);
}

// the pixels whose centres lie in the triangle's box, clamped to the image; false if there are none
__device__ __forceinline__ bool tri_box(const Tri& T, int W, int H, int& i0, int& j0, int& i1, int& j1) {
  const int minX = min(T.X[0], min(T.X[1], T.X[2])), maxX = max(T.X[0], max(T.X[1], T.X[2]));
  const int minY = min(T.Y[0], min(T.Y[1], T.Y[2])), maxY = max(T.Y[0], max(T.Y[1], T.Y[2]));
  i0 = max(0, (minX + kSub - 1) >> 8);  // ceil and floor of X / 256 (arithmetic shifts)
  j0 = max(0, (minY + kSub - 1) >> 8);
  i1 = min(W - 1, maxX >> 8);
  j1 = min(H - 1, maxY >> 8);
  return i0 <= i1 && j0 <= j1;
}

__device__ __forceinline__ void vis_min(unsigned long long* __restrict__ vis, size_t pix, float z, unsigned t) {
  const unsigned long long key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned long long)t;
  // keys only fall: a stale read is too large and costs one atomic that loses
  if (__hip_atomic_load(vis + pix, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= key) return;
  atomicMin(vis + pix, key);
}

__global__ __launch_bounds__(256) void raster_small_kernel(MeshK m, long long small_max, unsigned long long* __restrict__ vis,
                                                           unsigned* __restrict__ counter, unsigned* __restrict__ list) {
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  if (t >= (unsigned)m.F) return;
  Tri T;
  if (!tri_setup(m, t, T)) return;
  int i0, j0, i1, j1;
  if (!tri_box(T, m.W, m.H, i0, j0, i1, j1)) return;
  if ((long long)(i1 - i0 + 1) * (long long)(j1 - j0 + 1) > small_max) {
    const unsigned slot = atomicAdd(counter, 1u);
    if (slot < (unsigned)m.F) list[slot] = t;  // every triangle is appended at most once: F slots suffice
    return;
  }
  for (int j = j0; j <= j1; j++)
    for (int i = i0; i <= i1; i++) {
      Sample S;
      if (tri_sample(T, i, j, S)) vis_min(vis, (size_t)j * m.W + i, S.z, t);
    }
}

__global__ __launch_bounds__(256) void raster_large_kernel(MeshK m, unsigned long long* __restrict__ vis,
                                                           const unsigned* __restrict__ counter,
                                                           const unsigned* __restrict__ list) {
  const unsigned lane = threadIdx.x & 63u;
  const unsigned wave = blockIdx.x * 4u + (threadIdx.x >> 6);
  const unsigned n = min(*counter, (unsigned)m.F);
  for (unsigned e = wave; e < n; e += gridDim.x * 4u) {
    const unsigned t = list[e];
    if (t >= (unsigned)m.F) continue;
    Tri T;
    if (!tri_setup(m, t, T)) continue;
    int i0, j0, i1, j1;
    if (!tri_box(T, m.W, m.H, i0, j0, i1, j1)) continue;
    const unsigned bw = (unsigned)(i1 - i0 + 1);
    const unsigned long long count = (unsigned long long)bw * (unsigned)(j1 - j0 + 1);
    for (unsigned long long c = lane; c < count; c += 64) {
      const unsigned row = (unsigned)(c / bw);
      const int i = i0 + (int)(c - (unsigned long long)row * bw), j = j0 + (int)row;
      Sample S;
      if (tri_sample(T, i, j, S)) vis_min(vis, (size_t)j * m.W + i, S.z, t);
    }
  }
}

struct AttrK {
  const float *normals, *albedo, *roughness, *metallic, *viewmatrix;
};
struct PlanesK {
  float *opacity, *depth, *pos, *normal, *normal_view, *albedo, *roughness, *metallic;
  int* tri_id;
};

__device__ __forceinline__ float interp(const Sample& S, float a0, float a1, float a2) {
  return ((S.w0 * a0 + S.w1 * a1) + S.w2 * a2) / S.s;
}

__global__ __launch_bounds__(256) void resolve_kernel(MeshK m, AttrK a, const unsigned long long* __restrict__ vis, PlanesK o) {
  const size_t HW = (size_t)m.H * m.W;
  const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const int j = (int)(pix / (unsigned)m.W), i = (int)(pix - (size_t)j * m.W);
  const unsigned long long key = vis[pix];
  const unsigned t = (unsigned)(key & 0xffffffffull);
  Tri T;
  Sample S;
  const bool hit = key != kEmpty && t < (unsigned)m.F && tri_setup(m, t, T) && tri_sample(T, i, j, S);
  // What the blend kernel leaves where no Gaussian contributes (black background, inference): T = 1, every sum 0, so
  // colour-like planes 0, roughness = 0 + T, depth and pos 0 (opacity <= 1e-6), normal_view = normalize3 of a zero vector.
  v3 N = {0.0f, 0.0f, 0.0f}, Al = {0.0f, 0.0f, 0.0f}, P = {0.0f, 0.0f, 0.0f};
  float O = 0.0f, D = 0.0f, Rr = 1.0f, Mm = 0.0f;
  int id = -1;
  if (hit) {
    const size_t v0 = T.v[0], v1 = T.v[1], v2 = T.v[2];
    O = 1.0f;
    D = S.z;
    id = (int)t;
    P = {interp(S, m.view_pos[3 * v0], m.view_pos[3 * v1], m.view_pos[3 * v2]),
         interp(S, m.view_pos[3 * v0 + 1], m.view_pos[3 * v1 + 1], m.view_pos[3 * v2 + 1]),
         interp(S, m.view_pos[3 * v0 + 2], m.view_pos[3 * v1 + 2], m.view_pos[3 * v2 + 2])};
    N = {interp(S, a.normals[3 * v0], a.normals[3 * v1], a.normals[3 * v2]),
         interp(S, a.normals[3 * v0 + 1], a.normals[3 * v1 + 1], a.normals[3 * v2 + 1]),
         interp(S, a.normals[3 * v0 + 2], a.normals[3 * v1 + 2], a.normals[3 * v2 + 2])};
    Al = {interp(S, a.albedo[3 * v0], a.albedo[3 * v1], a.albedo[3 * v2]),
          interp(S, a.albedo[3 * v0 + 1], a.albedo[3 * v1 + 1], a.albedo[3 * v2 + 1]),
          interp(S, a.albedo[3 * v0 + 2], a.albedo[3 * v1 + 2], a.albedo[3 * v2 + 2])};
    Rr = interp(S, a.roughness[v0], a.roughness[v1], a.roughness[v2]);
    Mm = interp(S, a.metallic[v0], a.metallic[v1], a.metallic[v2]);
  }
  const v3 nv = normalize3(xform_vec_4x3(N, a.viewmatrix));  // NaN when N == 0, as in blend.hip
  o.opacity[pix] = O;
  o.depth[pix] = D;
  o.pos[pix] = P.x; o.pos[HW + pix] = P.y; o.pos[2 * HW + pix] = P.z;
  o.normal[pix] = N.x; o.normal[HW + pix] = N.y; o.normal[2 * HW + pix] = N.z;
  o.normal_view[pix] = nv.x; o.normal_view[HW + pix] = nv.y; o.normal_view[2 * HW + pix] = nv.z;
  o.albedo[pix] = Al.x; o.albedo[HW + pix] = Al.y; o.albedo[2 * HW + pix] = Al.z;
  o.roughness[pix] = Rr;
  o.metallic[pix] = Mm;
  o.tri_id[pix] = id;
}

struct TexK {
  const float* uvs;                     // [F,3,2]: one UV per face corner
  const float *albedo, *orm, *normal;   // [3,Ht,Wt] planes; normal may be NULL (the vertex normals are interpolated)
  int Wt, Ht;
};

// One texel coordinate: the two taps (clamped to [0, n - 1]) and the weight of the second.  c is brought into [-1, n]
// first (fmaxf returns its non-NaN argument: a NaN becomes -1), so the conversion to int is always in range.
__device__ __forceinline__ void tex_axis(float c, int n, int& a, int& b, float& f) {
  c = fminf(fmaxf(c, -1.0f), (float)n);
  const float c0 = floorf(c);
  f = c - c0;
  const int i = (int)c0;
  a = min(max(i, 0), n - 1);
  b = min(max(i + 1, 0), n - 1);
}

__device__ __forceinline__ float bilerp(float t00, float t01, float t10, float t11, float fx, float gx, float fy, float gy) {
  return gy * (gx * t00 + fx * t01) + fy * (gx * t10 + fx * t11);
}

__global__ __launch_bounds__(256) void resolve_textured_kernel(MeshK m, AttrK a, TexK x,
                                                               const unsigned long long* __restrict__ vis, PlanesK o,
                                                               float* __restrict__ occlusion) {
  const size_t HW = (size_t)m.H * m.W;
  const size_t pix = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (pix >= HW) return;
  const int j = (int)(pix / (unsigned)m.W), i = (int)(pix - (size_t)j * m.W);
  const unsigned long long key = vis[pix];
  const unsigned t = (unsigned)(key & 0xffffffffull);
  Tri T;
  Sample S;
  const bool hit = key != kEmpty && t < (unsigned)m.F && tri_setup(m, t, T) && tri_sample(T, i, j, S);
  // the background of resolve_kernel, and occlusion 1: open
  v3 N = {0.0f, 0.0f, 0.0f}, Al = {0.0f, 0.0f, 0.0f}, P = {0.0f, 0.0f, 0.0f};
  float O = 0.0f, D = 0.0f, Rr = 1.0f, Mm = 0.0f, Oc = 1.0f;
  int id = -1;
  if (hit) {
    const size_t v0 = T.v[0], v1 = T.v[1], v2 = T.v[2];
    const float* uv = x.uvs + 6 * (size_t)t;
    const int k1 = T.flip ? 2 : 1, k2 = T.flip ? 1 : 2;  // the corner that became T.v[1], T.v[2]
    const float u = interp(S, uv[0], uv[2 * k1], uv[2 * k2]);
    const float v = interp(S, uv[1], uv[2 * k1 + 1], uv[2 * k2 + 1]);
    int xa, xb, ya, yb;
    float fx, fy;
    tex_axis(u * (float)x.Wt - 0.5f, x.Wt, xa, xb, fx);
    tex_axis((1.0f - v) * (float)x.Ht - 0.5f, x.Ht, ya, yb, fy);  // v = 0 is the bottom row
    const float gx = 1.0f - fx, gy = 1.0f - fy;
    const size_t plane = (size_t)x.Wt * x.Ht;
    const size_t q00 = (size_t)ya * x.Wt + xa, q01 = (size_t)ya * x.Wt + xb;
    const size_t q10 = (size_t)yb * x.Wt + xa, q11 = (size_t)yb * x.Wt + xb;
    // every gather is issued before the first is used: the taps are independent
    float ta[3][4], tm[3][4], tn[3][4];
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const float* pa = x.albedo + c * plane;
      const float* pm = x.orm + c * plane;
      ta[c][0] = pa[q00]; ta[c][1] = pa[q01]; ta[c][2] = pa[q10]; ta[c][3] = pa[q11];
      tm[c][0] = pm[q00]; tm[c][1] = pm[q01]; tm[c][2] = pm[q10]; tm[c][3] = pm[q11];
    }
    if (x.normal != nullptr) {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const float* pn = x.normal + c * plane;
        tn[c][0] = pn[q00]; tn[c][1] = pn[q01]; tn[c][2] = pn[q10]; tn[c][3] = pn[q11];
      }
    } else {
#pragma unroll
      for (int c = 0; c < 3; c++) {
        tn[c][0] = a.normals[3 * v0 + c]; tn[c][1] = a.normals[3 * v1 + c]; tn[c][2] = a.normals[3 * v2 + c];
        tn[c][3] = 0.0f;
      }
    }
    O = 1.0f;
    D = S.z;
    id = (int)t;
    P = {interp(S, m.view_pos[3 * v0], m.view_pos[3 * v1], m.view_pos[3 * v2]),
         interp(S, m.view_pos[3 * v0 + 1], m.view_pos[3 * v1 + 1], m.view_pos[3 * v2 + 1]),
         interp(S, m.view_pos[3 * v0 + 2], m.view_pos[3 * v1 + 2], m.view_pos[3 * v2 + 2])};
    Al = {bilerp(ta[0][0], ta[0][1], ta[0][2], ta[0][3], fx, gx, fy, gy),
          bilerp(ta[1][0], ta[1][1], ta[1][2], ta[1][3], fx, gx, fy, gy),
          bilerp(ta[2][0], ta[2][1], ta[2][2], ta[2][3], fx, gx, fy, gy)};
    Oc = bilerp(tm[0][0], tm[0][1], tm[0][2], tm[0][3], fx, gx, fy, gy);
    Rr = bilerp(tm[1][0], tm[1][1], tm[1][2], tm[1][3], fx, gx, fy, gy);
    Mm = bilerp(tm[2][0], tm[2][1], tm[2][2], tm[2][3], fx, gx, fy, gy);
    if (x.normal != nullptr)
      N = {bilerp(tn[0][0], tn[0][1], tn[0][2], tn[0][3], fx, gx, fy, gy),
           bilerp(tn[1][0], tn[1][1], tn[1][2], tn[1][3], fx, gx, fy, gy),
           bilerp(tn[2][0], tn[2][1], tn[2][2], tn[2][3], fx, gx, fy, gy)};
    else
      N = {interp(S, tn[0][0], tn[0][1], tn[0][2]), interp(S, tn[1][0], tn[1][1], tn[1][2]),
           interp(S, tn[2][0], tn[2][1], tn[2][2])};
  }
  const v3 nv = normalize3(xform_vec_4x3(N, a.viewmatrix));  // NaN when N == 0, as in resolve_kernel
  o.opacity[pix] = O;
  o.depth[pix] = D;
  o.pos[pix] = P.x; o.pos[HW + pix] = P.y; o.pos[2 * HW + pix] = P.z;
  o.normal[pix] = N.x; o.normal[HW + pix] = N.y; o.normal[2 * HW + pix] = N.z;
  o.normal_view[pix] = nv.x; o.normal_view[HW + pix] = nv.y; o.normal_view[2 * HW + pix] = nv.z;
  o.albedo[pix] = Al.x; o.albedo[HW + pix] = Al.y; o.albedo[2 * HW + pix] = Al.z;
  o.roughness[pix] = Rr;
  o.metallic[pix] = Mm;
  occlusion[pix] = Oc;
  o.tri_id[pix] = id;
}

inline bool image_ok(int W, int H) { return W >= 1 && H >= 1 && W <= (int)kGuard && H <= (int)kGuard; }
inline unsigned blocks_for(size_t n) { return (unsigned)((n + 255) / 256); }

}  // namespace mesh_raster
}  // namespace gigs

extern "C" {

int gigs_mesh_project(int n_vertices, const float* vertices, const float* viewmatrix, float tanfovx, float tanfovy, int width,
                      int height, float* view_pos, int* screen, uint8_t* flags, void* stream) {
  using namespace gigs::mesh_raster;
  if (n_vertices == 0) return 0;
  if (n_vertices < 0 || !vertices || !viewmatrix || !image_ok(width, height) || !(tanfovx > 0.0f) || !(tanfovy > 0.0f) ||
      !view_pos || !screen || !flags)
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_project: bad argument");
  const ProjK k = {(float)width / (2.0f * tanfovx), (float)height / (2.0f * tanfovy), (float)(width - 1) / 2.0f,
                   (float)(height - 1) / 2.0f};
  hipLaunchKernelGGL(project_kernel, dim3(blocks_for((size_t)n_vertices)), dim3(256), 0, (hipStream_t)stream, n_vertices, k,
                     vertices, viewmatrix, view_pos, screen, flags);
  return gigs_internal_check_launch("mesh_project");
}

size_t gigs_mesh_raster_scratch_bytes(int n_faces) { return sizeof(unsigned) * ((size_t)(n_faces > 0 ? n_faces : 0) + 4); }

int gigs_mesh_raster(int n_vertices, int n_faces, const int* faces, const float* view_pos, const int* screen,
                     const uint8_t* flags, int width, int height, int small_max, unsigned long long* vis, void* scratch,
                     void* stream) {
  using namespace gigs::mesh_raster;
  if (n_vertices < 0 || n_faces < 0 || !image_ok(width, height) || !vis || !scratch)
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_raster: bad argument");
  if (n_faces > 0 && (!faces || (n_vertices > 0 && (!view_pos || !screen || !flags))))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_raster: NULL mesh array");
  hipStream_t s = (hipStream_t)stream;
  unsigned* counter = (unsigned*)scratch;  // [0] the list's length, [4..4 + F) the list
  unsigned* list = counter + 4;
  if (hipMemsetAsync(counter, 0, 4 * sizeof(unsigned), s) != hipSuccess)
    return gigs_internal_fail(GIGS_ERR_HIP, "mesh_raster: clearing the counter failed");
  if (n_faces == 0) return 0;
  const MeshK m = {n_vertices, n_faces, width, height, faces, view_pos, screen, flags};
  hipLaunchKernelGGL(raster_small_kernel, dim3(blocks_for((size_t)n_faces)), dim3(256), 0, s, m,
                     (long long)(small_max < 0 ? GIGS_MESH_SMALL_MAX : small_max), vis, counter, list);
  hipLaunchKernelGGL(raster_large_kernel, dim3(kLargeBlocks), dim3(256), 0, s, m, vis, counter, list);
  return gigs_internal_check_launch("mesh_raster");
}

int gigs_mesh_resolve(int n_vertices, int n_faces, const int* faces, const float* view_pos, const int* screen,
                      const uint8_t* flags, const float* normals, const float* albedo, const float* roughness,
                      const float* metallic, const float* viewmatrix, int width, int height, const unsigned long long* vis,
                      float* opacity, float* depth, float* pos, float* normal, float* normal_view, float* albedo_out,
                      float* roughness_out, float* metallic_out, int* tri_id, void* stream) {
  using namespace gigs::mesh_raster;
  if (n_vertices < 0 || n_faces < 0 || !image_ok(width, height) || !vis || !viewmatrix || !opacity || !depth || !pos ||
      !normal || !normal_view || !albedo_out || !roughness_out || !metallic_out || !tri_id)
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_resolve: bad argument");
  if (n_faces > 0 && (!faces || (n_vertices > 0 && (!view_pos || !screen || !flags || !normals || !albedo || !roughness ||
                                                    !metallic))))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_resolve: NULL mesh array");
  const MeshK m = {n_vertices, n_faces, width, height, faces, view_pos, screen, flags};
  const AttrK a = {normals, albedo, roughness, metallic, viewmatrix};
  const PlanesK o = {opacity, depth, pos, normal, normal_view, albedo_out, roughness_out, metallic_out, tri_id};
  hipLaunchKernelGGL(resolve_kernel, dim3(blocks_for((size_t)width * height)), dim3(256), 0, (hipStream_t)stream, m, a, vis, o);
  return gigs_internal_check_launch("mesh_resolve");
}

int gigs_mesh_resolve_textured(int n_vertices, int n_faces, const int* faces, const float* view_pos, const int* screen,
                               const uint8_t* flags, const float* uvs, const float* normals, int tex_width, int tex_height,
                               const float* tex_albedo, const float* tex_orm, const float* tex_normal, const float* viewmatrix,
                               int width, int height, const unsigned long long* vis, float* opacity, float* depth, float* pos,
                               float* normal, float* normal_view, float* albedo_out, float* roughness_out, float* metallic_out,
                               float* occlusion_out, int* tri_id, void* stream) {
  using namespace gigs::mesh_raster;
  if (n_vertices < 0 || n_faces < 0 || !image_ok(width, height) || !image_ok(tex_width, tex_height) || !vis || !viewmatrix ||
      !opacity || !depth || !pos || !normal || !normal_view || !albedo_out || !roughness_out || !metallic_out ||
      !occlusion_out || !tri_id)
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_resolve_textured: bad argument");
  if (n_faces > 0 && (!faces || !uvs || !tex_albedo || !tex_orm ||
                      (n_vertices > 0 && (!view_pos || !screen || !flags || (!tex_normal && !normals)))))
    return gigs_internal_fail(GIGS_ERR_INVALID, "mesh_resolve_textured: NULL mesh or texture array");
  const MeshK m = {n_vertices, n_faces, width, height, faces, view_pos, screen, flags};
  const AttrK a = {normals, nullptr, nullptr, nullptr, viewmatrix};
  const TexK x = {uvs, tex_albedo, tex_orm, tex_normal, tex_width, tex_height};
  const PlanesK o = {opacity, depth, pos, normal, normal_view, albedo_out, roughness_out, metallic_out, tri_id};
  hipLaunchKernelGGL(resolve_textured_kernel, dim3(blocks_for((size_t)width * height)), dim3(256), 0, (hipStream_t)stream, m, a,
                     x, vis, o, occlusion_out);
  return gigs_internal_check_launch("mesh_resolve_textured");
}
}  // extern "C"
