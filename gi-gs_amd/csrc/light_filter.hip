// light_filter.hip -- the cubemap light filters: diffuse (cosine) filter, GGX bounds and GGX pre-filter, forward
// and backward, table-free and through cached pair-weight tables.
//
// Reference behaviour restated ("RU/" is pbr/renderutils/c_src/):
//   DiffuseCubemapFwd/BwdKernel          RU/cubemap.cu:110-169
//   SpecularBoundsKernel                 RU/cubemap.cu:181-244
//   SpecularCubemapFwd/BwdKernel         RU/cubemap.cu:246-350
//
// MI355X design
//   * the cubemap-filter backward passes are GATHERS, not the reference's atomic scatters, wherever the
//     set of outputs that touch a texel is that texel's own window: same terms, no atomics,
//     reproducible sums.  The cone test dot(L, V) >= cutoff is symmetric in (L, V); the ACCEPTED set is
//     not everywhere: a pair also needs the input inside the output's per-face AABB, and the bounds'
//     corner-only tile cull (restated from the reference on purpose) drops in-cone texels at small
//     resolutions, e.g. (16, 0.22), (9, 0.3), (7, 0.4).  Whether a (resolution, cutoff) is symmetric is
//     decided once and cached (window_symmetric); an asymmetric level's backward is the transpose in
//     scatter form, float atomics over each output's window (the *_scatter kernels below);
//   * pixel-invariant tables (solid angle per texel) are built once on the host with libm and
//     cached per device.  That cache is this file's only mutable state.
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "cube.h"

namespace gigs {

__device__ __forceinline__ float ndf_ggx(float alphaSqr, float cosTheta) {  // RU/cubemap.cu:174-179
  const float c = fminf(fmaxf(cosTheta, 0.0f), 1.0f);
  const float d = (c * alphaSqr - c) * c + 1.0f;
  return (float)((double)alphaSqr / ((double)(d * d) * 3.14159265358979323846));
}

// ---- per-resolution texel table: float4 (unit direction of the texel centre, solid angle) ----
// direction = cube_to_dir (RU/cubemap.cu:33-47, computed on the device once per resolution with
// the same IEEE sequence as the oracle); solid angle = pixel_area (RU/cubemap.cu:17-31) from a
// 1-D table built on the HOST with libm atanf: area[i] = atan((i+1)/H) - atan(i/H), i = |x - H|.
// Both are pixel- and iteration-invariant, so the filters read one 16-byte entry per texel
// instead of redoing 5 divisions, a sqrt and 4 atanf per (output, input) pair.
__global__ void __launch_bounds__(256)
texel_table_kernel(int N, const float* __restrict__ area, float4* __restrict__ table) {
  const int o = blockIdx.x * 256 + threadIdx.x;
  if (o >= 6 * N * N) return;
  const int pz = o / (N * N), py = (o / N) % N, px = o % N;
  const v3 d = cube_to_dir(px, py, pz, N);
  float a = 1.0f;
  if (N > 1) {
    const int Hh = N / 2;
    a = area[abs(px - Hh)] * area[abs(py - Hh)];
  }
  table[o] = make_float4(d.x, d.y, d.z, a);
}

struct TexelTable { float4* dev = nullptr; };
static std::mutex g_table_mu;
static std::map<long long, TexelTable> g_table;

static const float4* texel_table(int N, hipStream_t s) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return nullptr;
  std::lock_guard<std::mutex> lk(g_table_mu);
  const long long key = ((long long)dev << 32) | (unsigned)N;
  auto it = g_table.find(key);
  if (it != g_table.end()) return it->second.dev;
  const int Hh = N / 2;
  std::vector<float> h(Hh + 2, 1.0f);
  if (N > 1)
    for (int i = 0; i <= Hh; i++) h[i] = atanf((float)(i + 1) / (float)Hh) - atanf((float)i / (float)Hh);
  float* area = nullptr;
  TexelTable t;
  // one-time per (device, resolution); kept for the lifetime of the process
  if (hipMalloc(&area, h.size() * sizeof(float)) != hipSuccess) return nullptr;
  if (hipMalloc(&t.dev, (size_t)6 * N * N * sizeof(float4)) != hipSuccess) return nullptr;
  if (hipMemcpyAsync(area, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice, s) != hipSuccess) return nullptr;
  hipLaunchKernelGGL(texel_table_kernel, dim3((6 * N * N + 255) / 256), dim3(256), 0, s, N, area, t.dev);
  if (hipStreamSynchronize(s) != hipSuccess) return nullptr;
  hipFree(area);
  g_table[key] = t;
  return t.dev;
}

// ------------------------------------------------------------------------------------------
// cubemap filters: ONE WAVE PER OUTPUT TEXEL (4 per 256-lane workgroup).  The 64 lanes sweep
// the texel's window as an 8x8 patch, so neighbouring lanes read neighbouring 16-byte table /
// texture entries, and the four partial sums are combined with DPP.  Even the 16x16 level
// (1536 outputs) then fills the chip with 1536 waves instead of 24.
// ------------------------------------------------------------------------------------------
// forward: out[o] = sum_in tex[in] * w(o, in);  backward (gather): g_in[i] = sum_o g[o] * w(o, i)
template <bool kBackward>
__global__ void __launch_bounds__(256)
diffuse_cubemap_kernel(int N, const float4* __restrict__ table, const float* __restrict__ src,
                       float* __restrict__ dst) {
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (o >= 6 * N * N) return;  // wave-uniform
  const float4 me = table[o];
  float c0 = 0, c1 = 0, c2 = 0;
  for (int i = lane; i < 6 * N * N; i += 64) {
    const float4 ot = table[i];
    // forward: N = me, L = other, area of L; backward: N = other, L = me, area of me
    const float d = kBackward ? (ot.x * me.x + ot.y * me.y + ot.z * me.z) : (me.x * ot.x + me.y * ot.y + me.z * ot.z);
    const float costheta = fminf(fmaxf(d, 0.0f), 0.999f);
    const float w = costheta * (kBackward ? me.w : ot.w) / 3.141592f;
    const float* t = src + 3 * (size_t)i;
    c0 += t[0] * w; c1 += t[1] * w; c2 += t[2] * w;
  }
  c0 = wave_sum63(c0); c1 = wave_sum63(c1); c2 = wave_sum63(c2);
  if (lane == 63) { dst[3 * (size_t)o] = c0; dst[3 * (size_t)o + 1] = c1; dst[3 * (size_t)o + 2] = c2; }
}


__global__ void __launch_bounds__(64)
specular_bounds_kernel(int N, float cutoff, float* __restrict__ bounds) {
  const int o = blockIdx.x * 64 + threadIdx.x;
  if (o >= 6 * N * N) return;
  const int pz = o / (N * N), py = (o / N) % N, px = o % N;
  const v3 VNR = cube_to_dir(px, py, pz, N);
  const int TILE = 16;
  for (int s = 0; s < 6; ++s) {
    int minx = N - 1, maxx = 0, miny = N - 1, maxy = 0;
    for (int tx = 0; tx < (N + TILE - 1) / TILE; tx++)
      for (int ty = 0; ty < (N + TILE - 1) / TILE; ty++) {
        const int tsx = tx * TILE, tsy = ty * TILE;
        const int tex = min((tx + 1) * TILE, N), tey = min((ty + 1) * TILE, N);
        const v3 L0 = cube_to_dir(tsx, tsy, s, N), L1 = cube_to_dir(tex, tsy, s, N);
        const v3 L2 = cube_to_dir(tsx, tey, s, N), L3 = cube_to_dir(tex, tey, s, N);
        const float mnx = fminf(fminf(L0.x, L1.x), fminf(L2.x, L3.x)), mxx = fmaxf(fmaxf(L0.x, L1.x), fmaxf(L2.x, L3.x));
        const float mny = fminf(fminf(L0.y, L1.y), fminf(L2.y, L3.y)), mxy = fmaxf(fmaxf(L0.y, L1.y), fmaxf(L2.y, L3.y));
        const float mnz = fminf(fminf(L0.z, L1.z), fminf(L2.z, L3.z)), mxz = fmaxf(fmaxf(L0.z, L1.z), fmaxf(L2.z, L3.z));
        const float maxdp = fmaxf(mnx * VNR.x, mxx * VNR.x) + fmaxf(mny * VNR.y, mxy * VNR.y) + fmaxf(mnz * VNR.z, mxz * VNR.z);
        if (maxdp >= cutoff) {
          for (int y = tsy; y < tey; ++y)
            for (int x = tsx; x < tex; ++x) {
              const v3 L = cube_to_dir(x, y, s, N);
              if (dot3(L, VNR) >= cutoff) {
                minx = min(minx, x); maxx = max(maxx, x);
                miny = min(miny, y); maxy = max(maxy, y);
              }
            }
        }
      }
    float* b = bounds + 24 * (size_t)o + s * 4;
    b[0] = (float)minx; b[1] = (float)maxx; b[2] = (float)miny; b[3] = (float)maxy;
  }
}

// safeNormalize (RU/vec3f.h:90-94) for |v| in (2^-60, 2^60): the three IEEE quotients v / l share one
// reciprocal refinement (same FMA chain as the compiler's division expansion, bit-identical results).
__device__ __forceinline__ v3 normalize_exact(v3 v) {
  const float l = sqrtf(v.x * v.x + v.y * v.y + v.z * v.z);
  if (!(l > 0x1p-60f && l < 0x1p60f)) return safe_normalize(v);
  const float r0 = __builtin_amdgcn_rcpf(l);
  const float e0 = __builtin_fmaf(-l, r0, 1.0f);
  const float r1 = __builtin_fmaf(e0, r0, r0);
  v3 q;
  {
    const float q0 = v.x * r1, e1 = __builtin_fmaf(-l, q0, v.x), q1 = __builtin_fmaf(e1, r1, q0);
    q.x = __builtin_fmaf(__builtin_fmaf(-l, q1, v.x), r1, q1);
  }
  {
    const float q0 = v.y * r1, e1 = __builtin_fmaf(-l, q0, v.y), q1 = __builtin_fmaf(e1, r1, q0);
    q.y = __builtin_fmaf(__builtin_fmaf(-l, q1, v.y), r1, q1);
  }
  {
    const float q0 = v.z * r1, e1 = __builtin_fmaf(-l, q0, v.z), q1 = __builtin_fmaf(e1, r1, q0);
    q.z = __builtin_fmaf(__builtin_fmaf(-l, q1, v.z), r1, q1);
  }
  return q;
}

// forward: out[o] = (sum_in tex[in] w, sum w) over in in window(o)
// backward: g_in[i] = sum_o g[o].rgb * w(o, i) over the outputs o whose window accepts i.
//   kBackward (gather): texel i sums over its OWN window with the roles exchanged -- the same set only where the
//     accepted set is symmetric (see the header; the host launches it for such levels only);
//   kScatter: the wave of output o walks o's window as the forward does and adds g[o].rgb * w(o, i) into dst[i]
//     (zeroed by the host) with float atomics: the transpose whatever the bounds are.
// Per accepted pair H = safeNormalize(L + V), c = V.H and d = (c a^2 - c) c + 1 are the reference's
// own IEEE sequence (RU/cubemap.cu:174-179, 270-277) on the cached unit directions.  This matters: d = 1 - c^2 (1 - alpha^2) cancels to ~alpha^2 at the lobe centre, so a 1-ulp change of
// c = V.H (e.g. the algebraic shortcut sqrt((1 + L.V) / 2)) moves a weight by ~1e-7 / alpha^2 --
// 2e-3 at the roughness-0.08 level.
template <bool kBackward, bool kScatter = false>
__global__ void __launch_bounds__(256)
specular_cubemap_kernel(int N, const float4* __restrict__ table, const float* __restrict__ src,
                        const float* __restrict__ bounds, float roughness, float cutoff,
                        float* __restrict__ dst) {
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (o >= 6 * N * N) return;  // wave-uniform
  const int lx = lane & 7, ly = lane >> 3;
  const float4 me = table[o];
  const float alpha = roughness * roughness, alphaSqr = alpha * alpha;
  float wsum = 0.0f, c0 = 0, c1 = 0, c2 = 0;
  const int stride = kBackward ? 4 : 3;
  float g0 = 0, g1 = 0, g2 = 0;
  if (kScatter) { const float* g = src + 4 * (size_t)o; g0 = g[0]; g1 = g[1]; g2 = g[2]; }
  const float4* b4 = reinterpret_cast<const float4*>(bounds + 24 * (size_t)o);
  for (int s = 0; s < 6; ++s) {
    const float4 b = b4[s];
    const int xmin = (int)b.x, xmax = (int)b.y, ymin = (int)b.z, ymax = (int)b.w;
    if (xmin > xmax) continue;
    for (int y = ymin + ly; y <= ymax; y += 8)
      for (int x = xmin + lx; x <= xmax; x += 8) {
        const int i = (s * N + y) * N + x;
        const float4 ot = table[i];
        const float d = kBackward ? (me.x * ot.x + me.y * ot.y + me.z * ot.z) : (ot.x * me.x + ot.y * me.y + ot.z * me.z);
        if (d >= cutoff) {
          const float wiDotN = fmaxf(d, 0.0f);
          // forward: VNR = me, L = other; backward: VNR = other, L = me
          const v3 Hh = kBackward ? normalize_exact(v3{me.x + ot.x, me.y + ot.y, me.z + ot.z})
                                  : normalize_exact(v3{ot.x + me.x, ot.y + me.y, ot.z + me.z});
          const float VNRDotH = fmaxf(kBackward ? (ot.x * Hh.x + ot.y * Hh.y + ot.z * Hh.z)
                                                : (me.x * Hh.x + me.y * Hh.y + me.z * Hh.z), 0.0f);
          // c and dd exactly as the reference; only the last, well-conditioned division
          // alphaSqr / (dd^2 * pi) is done in fp32 instead of fp64 (<= 2e-7 relative)
          const float c = fminf(fmaxf(VNRDotH, 0.0f), 1.0f);
          const float dd = (c * alphaSqr - c) * c + 1.0f;
          const float ndf = alphaSqr / ((dd * dd) * 3.14159265358979323846f);
          const float w = wiDotN * ndf * (kBackward ? me.w : ot.w) / 4.0f;
          if (kScatter) {
            float* q = dst + 3 * (size_t)i;
            const float v0 = g0 * w, v1 = g1 * w, v2 = g2 * w;
            if (v0 != 0.0f) atomicAdd(q, v0);  // true for NaN: it reaches dst
            if (v1 != 0.0f) atomicAdd(q + 1, v1);
            if (v2 != 0.0f) atomicAdd(q + 2, v2);
            continue;
          }
          const float* t = src + (size_t)stride * i;
          c0 += t[0] * w; c1 += t[1] * w; c2 += t[2] * w;
          wsum += w;
        }
      }
  }
  if (kScatter) return;
  c0 = wave_sum63(c0); c1 = wave_sum63(c1); c2 = wave_sum63(c2);
  if (!kBackward) wsum = wave_sum63(wsum);
  if (lane == 63) {
    if (kBackward) {
      float* q = dst + 3 * (size_t)o;
      q[0] = c0; q[1] = c1; q[2] = c2;
    } else {
      float* q = dst + 4 * (size_t)o;
      q[0] = c0; q[1] = c1; q[2] = c2; q[3] = wsum;
    }
  }
}

// 1 -> *asymmetric if some pair (o, i) is accepted by o and not by i (i in AABB_o, o outside AABB_i; the dot product
// is the same float both ways: the products commute and the additions keep their order).
__global__ void __launch_bounds__(256)
specular_symmetry_kernel(int N, const float4* __restrict__ table, const float* __restrict__ bounds, float cutoff,
                         int* __restrict__ asymmetric) {
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (o >= 6 * N * N) return;  // wave-uniform
  const int lx = lane & 7, ly = lane >> 3;
  const int so = o / (N * N), yo = (o / N) % N, xo = o % N;
  const float4 me = table[o];
  const float4* b4 = reinterpret_cast<const float4*>(bounds + 24 * (size_t)o);
  bool bad = false;
  for (int s = 0; s < 6; ++s) {
    const float4 b = b4[s];
    const int xmin = (int)b.x, xmax = (int)b.y, ymin = (int)b.z, ymax = (int)b.w;
    if (xmin > xmax) continue;
    for (int y = ymin + ly; y <= ymax; y += 8)
      for (int x = xmin + lx; x <= xmax; x += 8) {
        const int i = (s * N + y) * N + x;
        const float4 ot = table[i];
        if (ot.x * me.x + ot.y * me.y + ot.z * me.z >= cutoff) {
          const float4 r = reinterpret_cast<const float4*>(bounds + 24 * (size_t)i)[so];
          bad |= !(xo >= (int)r.x && xo <= (int)r.y && yo >= (int)r.z && yo <= (int)r.w);
        }
      }
  }
  if (bad) *asymmetric = 1;  // every writer stores the same value
}

// Whether the accepted set of (resolution, cutoff) is symmetric: 1 yes, 0 no, -1 on a HIP error.  Decided once per
// (device, resolution, cutoff) from the library's own bounds and cached for the lifetime of the process; the first
// query synchronises the stream (like the texel table's), so it belongs where bounds and tables are built, or to a
// first, eager, call -- not into a graph capture.
static std::map<std::pair<long long, uint32_t>, int> g_symmetric;

static int window_symmetric(int N, float cutoff, hipStream_t s) {
  const float4* table = texel_table(N, s);
  int dev = 0;
  if (!table || hipGetDevice(&dev) != hipSuccess) return -1;
  uint32_t bits;
  memcpy(&bits, &cutoff, sizeof bits);
  const std::pair<long long, uint32_t> key(((long long)dev << 32) | (unsigned)N, bits);
  std::lock_guard<std::mutex> lk(g_table_mu);
  auto it = g_symmetric.find(key);
  if (it != g_symmetric.end()) return it->second;
  const int total = 6 * N * N;
  float* bounds = nullptr;
  int* flag = nullptr;
  int host = 0;
  bool ok = hipMalloc(&bounds, (size_t)24 * total * sizeof(float)) == hipSuccess && hipMalloc(&flag, sizeof(int)) == hipSuccess &&
            hipMemsetAsync(flag, 0, sizeof(int), s) == hipSuccess;
  if (ok) {
    hipLaunchKernelGGL(specular_bounds_kernel, dim3((total + 63) / 64), dim3(64), 0, s, N, cutoff, bounds);
    hipLaunchKernelGGL(specular_symmetry_kernel, dim3((total + 3) / 4), dim3(256), 0, s, N, table, bounds, cutoff, flag);
    ok = hipMemcpyAsync(&host, flag, sizeof(int), hipMemcpyDeviceToHost, s) == hipSuccess && hipStreamSynchronize(s) == hipSuccess;
  }
  if (bounds) hipFree(bounds);
  if (flag) hipFree(flag);
  if (!ok) return -1;
  return g_symmetric[key] = host ? 0 : 1;
}

// The transpose from the FORWARD table, for the levels whose accepted set is not symmetric: the wave of output o walks
// o's runs as specular_weights_kernel laid them out and adds (w / wsum[o]) * g[o] -- w * g[o] without wsum -- into
// dst[i] (zeroed by the host) with float atomics.  The quotient is the float the sparse scatter forms.  Such levels are
// small (the tile cull drops texels at coarse resolutions); no tuning.
__global__ void __launch_bounds__(256)
specular_table_scatter_kernel(int N, const float* __restrict__ grad, int gstride, const float* __restrict__ bounds,
                              const uint32_t* __restrict__ offsets, const float* __restrict__ W,
                              const float* __restrict__ wsum, float* __restrict__ dst) {
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (o >= 6 * N * N) return;  // wave-uniform
  const float* g = grad + (size_t)gstride * o;
  const float g0 = g[0], g1 = g[1], g2 = g[2];
  const float4* b4 = reinterpret_cast<const float4*>(bounds + 24 * (size_t)o);
  for (int s = 0; s < 6; ++s) {
    const float4 b = b4[s];
    const int xmin = (int)b.x, xmax = (int)b.y, ymin = (int)b.z, ymax = (int)b.w;
    if (xmin > xmax || ymin > ymax) continue;
    const int wd = xmax - xmin + 1, n = wd * (ymax - ymin + 1);
    const float inv = 1.0f / (float)wd;
    const uint32_t base = offsets[6 * (size_t)o + s];
    for (int i = lane; i < n; i += 64) {
      const float w = W[(size_t)base + i];
      if (!(w >= 0.0f)) continue;  // -1 marks a candidate outside the cone
      const int yy = (int)(((float)i + 0.5f) * inv), xx = i - yy * wd;
      const float q = wsum ? w / wsum[o] : w;
      float* d = dst + 3 * ((size_t)(s * N + ymin + yy) * N + xmin + xx);
      const float v0 = q * g0, v1 = q * g1, v2 = q * g2;
      if (v0 != 0.0f) atomicAdd(d, v0);  // true for NaN: it reaches dst
      if (v1 != 0.0f) atomicAdd(d + 1, v1);
      if (v2 != 0.0f) atomicAdd(d + 2, v2);
    }
  }
}

// ------------------------------------------------------------------------------------------
// GGX pre-filter through a cached weight table.
// The weight of a (texel, texel) pair, f = max(L.V, 0) * D_ggx(V.H), depends only on the resolution,
// the roughness and the cutoff -- not on the cubemap values that change every training step.  With
// 288 GB of HBM it is cheaper to keep f for every candidate of every window (186 M floats = 0.74 GB
// for the 256..16 chain, twice that with the role-swapped table the backward needs) than to redo the
// normalisation, the NDF and its divisions each step: the filter becomes one streaming pass
// (4 B of weight + an L2-resident texel per candidate) instead of a VALU-bound one.
// Table layout: for (texel o, face s) the entries [offsets[6o+s], +w*h) hold f row-major over the
// face's AABB, or -1 for candidates outside the cone.  kSwap = false: roles (VNR = o, L = in) as the
// forward uses them; kSwap = true: (VNR = other, L = o) as the gather-form backward needs them, so
// that every product is bit-identical to the table-free kernels above.
// ------------------------------------------------------------------------------------------
template <bool kSwap>
__global__ void __launch_bounds__(256)
specular_weights_kernel(int N, const float4* __restrict__ table, const float* __restrict__ bounds,
                        const uint32_t* __restrict__ offsets, float roughness, float cutoff,
                        float* __restrict__ W) {
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (o >= 6 * N * N) return;
  const float4 me = table[o];
  const float alpha = roughness * roughness, alphaSqr = alpha * alpha;
  const float4* b4 = reinterpret_cast<const float4*>(bounds + 24 * (size_t)o);
  for (int s = 0; s < 6; ++s) {
    const float4 b = b4[s];
    const int xmin = (int)b.x, xmax = (int)b.y, ymin = (int)b.z, ymax = (int)b.w;
    if (xmin > xmax || ymin > ymax) continue;
    const int wd = xmax - xmin + 1, n = wd * (ymax - ymin + 1);
    const float inv = 1.0f / (float)wd;
    const uint32_t base = offsets[6 * (size_t)o + s];
    for (int i = lane; i < n; i += 64) {
      const int yy = (int)(((float)i + 0.5f) * inv), xx = i - yy * wd;
      const float4 ot = table[(s * N + ymin + yy) * N + xmin + xx];
      const float d = kSwap ? (me.x * ot.x + me.y * ot.y + me.z * ot.z) : (ot.x * me.x + ot.y * me.y + ot.z * me.z);
      float f = -1.0f;
      if (d >= cutoff) {
        const float wiDotN = fmaxf(d, 0.0f);
        const v3 Hh = kSwap ? normalize_exact(v3{me.x + ot.x, me.y + ot.y, me.z + ot.z})
                            : normalize_exact(v3{ot.x + me.x, ot.y + me.y, ot.z + me.z});
        const float VNRDotH = fmaxf(kSwap ? (ot.x * Hh.x + ot.y * Hh.y + ot.z * Hh.z)
                                          : (me.x * Hh.x + me.y * Hh.y + me.z * Hh.z), 0.0f);
        const float c = fminf(fmaxf(VNRDotH, 0.0f), 1.0f);
        const float dd = (c * alphaSqr - c) * c + 1.0f;
        // the full pair weight, ((wiDotN * ndf) * area) / 4 as in RU/cubemap.cu:276: area of the input
        // texel in the forward table, of the gathering texel in the role-swapped (backward) table
        f = wiDotN * (alphaSqr / ((dd * dd) * 3.14159265358979323846f)) * (kSwap ? me.w : ot.w) / 4.0f;
      }
      W[(size_t)base + i] = f;
    }
  }
}

// W2[o][i] = W[o][i] / divisor[texel i of o's window] (markers < 0 kept).  With divisor = the forward's weight sums this
// folds the d(rgb / wsum) division of the normalised filter's backward into its (cached) table: the backward then gathers
// the incoming gradient directly, one launch instead of a division pass + a gather.
__global__ void __launch_bounds__(256)
specular_divide_weights_kernel(int N, const float* __restrict__ bounds, const uint32_t* __restrict__ offsets,
                               const float* __restrict__ W, const float* __restrict__ divisor, float* __restrict__ W2) {
  const int o = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (o >= 6 * N * N) return;
  const float4* b4 = reinterpret_cast<const float4*>(bounds + 24 * (size_t)o);
  for (int s = 0; s < 6; ++s) {
    const float4 b = b4[s];
    const int xmin = (int)b.x, xmax = (int)b.y, ymin = (int)b.z, ymax = (int)b.w;
    if (xmin > xmax || ymin > ymax) continue;
    const int wd = xmax - xmin + 1, n = wd * (ymax - ymin + 1);
    const float inv = 1.0f / (float)wd;
    const uint32_t base = offsets[6 * (size_t)o + s];
    for (int i = lane; i < n; i += 64) {
      const int yy = (int)(((float)i + 0.5f) * inv), xx = i - yy * wd;
      const float w = W[(size_t)base + i];
      W2[(size_t)base + i] = w >= 0.0f ? w / divisor[(s * N + ymin + yy) * N + xmin + xx] : w;
    }
  }
}

// forward: out[o] = (sum tex[in] * f * area(in) / 4, sum of weights); backward: g_in[o] = sum g[other].rgb * f * area(o) / 4
// kNorm: the forward writes rgb / wsum to dst [.,3] and wsum to `wsum_out` (the division
// ops.py:458 does in torch); the backward then reads a 3-channel gradient that the caller has
// already divided by wsum.
// Sum over groups of kLanes consecutive lanes (8 = half a DPP row, 16 = a row, 64 = the wave); the total is
// valid in the last lane of every group.
typedef float pbr_f2 __attribute__((ext_vector_type(2)));

template <int kLanes>
__device__ __forceinline__ float group_sum_last(float v) {
  v += row_f<0xb1>(v);
  v += row_f<0x4e>(v);
  if (kLanes == 8) return v + row_f<0x141>(v);  // row_half_mirror: the other quad of the 8-lane group
  v += row_f<0x124>(v);
  v += row_f<0x128>(v);
  if (kLanes == 64) {
    v += row_f<0x142, 0xa>(v);
    v += row_f<0x143, 0xc>(v);
  }
  return v;
}

// Applies the cached GGX weights: out[o] = sum_i W[o][i] * src[window_o[i]].  A texel's window is up to six
// face rectangles (`bounds`), and its weights are ONE contiguous run of the table (the rectangles in face
// order, `offsets[6 o]` onward), so the kernel treats the window as a flat candidate list:
//   * all six rectangles are loaded up front (six independent 16-byte loads: one memory round trip instead
//     of one per face) and kept in LDS, one 20-word record per texel; a lane keeps the face it is in;
//   * an iteration issues the texel gathers of kU candidates per lane unconditionally (a rejected candidate,
//     weight -1, still lies inside its face) and, before it consumes anything, the weight loads of the NEXT
//     iteration: it waits for one memory round trip, and the weight stream stays in flight across iterations;
//   * kLanes = 8 / 16 pack eight / four texels into a wave for the levels whose windows hold ~10^2..10^3
//     candidates (the fixed per-texel work is shared by the wave), kLanes = 64 gives a whole wave to a texel.
// The lane-to-candidate assignment, the order of a lane's additions and the reduction are fixed: results are
// bit-identical from one version of the loop to the next.
// The pass streams the table once (0.74 GB per direction for the reference's 256..16 chain).  Plain loads, not
// nontemporal ones: the kU loads of an 8- or 16-lane group fall into one cache line, and a nontemporal load drops
// the line behind it (measured: +20 % time).
// kListed (the sparse forward, specular_apply_multi_fwd_sparse_kernel): group number j takes its output texel from
// list[j], j < n_listed, not from its own number.  The lanes of a group, their candidates, the order of a lane's additions
// and the reduction do not depend on which texels share the wave, so a listed texel gets the bits it has from the dense
// launch; texels that are not listed are not written.
template <bool kBackward, bool kNorm, int kLanes, bool kListed = false>
__device__ __forceinline__ void specular_apply_body(int block, int N, const float* __restrict__ src,
                                                    const float* __restrict__ bounds, const uint32_t* __restrict__ offsets,
                                                    const float* __restrict__ W, float* __restrict__ dst,
                                                    float* __restrict__ wsum_out, const int* __restrict__ list = nullptr,
                                                    int n_listed = 0) {
  constexpr int kPerWave = 64 / kLanes;
  constexpr int kU = 4;
  const int lane = threadIdx.x & 63;
  const int total = 6 * N * N;
  const int o_raw = (block * 4 + (threadIdx.x >> 6)) * kPerWave + lane / kLanes;
  if (kListed && (block * 4 + (int)(threadIdx.x >> 6)) * kPerWave >= n_listed) return;  // wave-uniform: no slot of the wave is listed
  const bool valid = kListed ? o_raw < n_listed : o_raw < total;
  // surplus groups stay in the wave for the DPP sums
  const int o = kListed ? (valid ? list[o_raw] : 0) : (valid ? o_raw : total - 1);
  const int g = lane % kLanes;
  const int stride = (kBackward && !kNorm) ? 4 : 3;

  // The six face rectangles of a texel -- prefix counts, widths, first texels -- are the same for all kLanes lanes of
  // its group and are needed again only where a lane crosses into the next face.  They live in LDS, 20 words per
  // texel, not in 25 registers per lane: the registers go to the loads in flight below.
  __shared__ int face_tab[4 * kPerWave * 20];
  int* tab = face_tab + ((threadIdx.x >> 6) * kPerWave + lane / kLanes) * 20;  // [0..6] pre, [8..13] wd, [14..19] base
  const float4* b4 = reinterpret_cast<const float4*>(bounds + 24 * (size_t)o);
  const uint32_t first = offsets[6 * (size_t)o];
  int n_all;
  {
    int wd[6], pre[7], base[6];
    pre[0] = 0;
#pragma unroll
    for (int s = 0; s < 6; ++s) {
      const float4 b = b4[s];
      const int xmin = (int)b.x, xmax = (int)b.y, ymin = (int)b.z, ymax = (int)b.w;
      const bool empty = xmin > xmax || ymin > ymax;
      wd[s] = empty ? 1 : xmax - xmin + 1;
      pre[s + 1] = pre[s] + (empty ? 0 : wd[s] * (ymax - ymin + 1));
      base[s] = empty ? 0 : (s * N + ymin) * N + xmin;
    }
    n_all = pre[6];
    if (g == 0) {
#pragma unroll
      for (int s = 0; s < 7; ++s) tab[s] = pre[s];
#pragma unroll
      for (int s = 0; s < 6; ++s) { tab[8 + s] = wd[s]; tab[14 + s] = base[s]; }
    }
    // written and read by lanes of the same wave only: LDS operations of a wave complete in order
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  }
  const int n = valid ? n_all : 0;
  // Both streams are addressed as a wave-uniform base plus a 32-bit byte offset (a 64-bit address per load in flight
  // would cost the registers the pipeline below needs).  The texels of a wave are consecutive and so are their runs
  // of the table, so the weights are addressed from the first lane's run.
  // (listed texels come in no order: there the base is the smallest run of the wave's listed texels, and the host admits
  // a level to the list only if its whole table lies within the 32-bit byte offset)
  uint32_t first_min = first;
  if (kListed) {
    first_min = valid ? first : 0xffffffffu;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) first_min = min(first_min, (uint32_t)__shfl_xor((int)first_min, d));
  }
  const uint32_t first0 = __builtin_amdgcn_readfirstlane(first_min);
  const char* wbase = reinterpret_cast<const char*>(W + first0);
  const char* tbase = reinterpret_cast<const char*>(src);
  const int wrel = (int)(first - first0);
  auto load_w = [&](int i) { return *reinterpret_cast<const float*>(wbase + (uint32_t)(4 * (wrel + i))); };

  pbr_f2 acc01 = {0.0f, 0.0f}, accw2 = {0.0f, 0.0f};  // (c0, c1) and (weight sum, c2)
  // Face of candidate i: the last face with pre[k] <= i (empty faces are overridden by the next one).  Candidate i of
  // a face with first candidate `pre`, width wd and first texel `base` is the texel base + loc + row (N - wd), with
  // loc = i - pre and row = floor(loc / wd); kept per face are the byte offset of (base - pre) and the byte stride
  // of a row, so that a candidate's offset is two shift-adds and one 24-bit multiply-add (row < N, the row stride
  // < 16 N: both far below 2^24), none of them a full 32-bit multiply.
  int f_pre, f_end;
  uint32_t f_off, f_row;
  float f_inv;
  auto find_face = [&](int i) {
    int k = 0;
#pragma unroll
    for (int j = 1; j < 6; j++) k += i >= tab[j] ? 1 : 0;  // the prefix counts do not decrease
    f_pre = tab[k]; f_end = tab[k + 1];
    const int f_wd = tab[8 + k];
    f_off = (uint32_t)(4 * stride * (tab[14 + k] - f_pre)); f_row = (uint32_t)(4 * stride * (N - f_wd));
    // row = floor((loc + 0.5) / wd): the half-texel slack dwarfs the 1-ulp error of the hardware reciprocal
    f_inv = __builtin_amdgcn_rcpf((float)f_wd);
  };
  auto texel_offset = [&](int i) {
    const uint32_t row = (uint32_t)(int)(((float)(i - f_pre) + 0.5f) * f_inv), ui = (uint32_t)i;
    uint32_t lin = (ui << (stride == 3 ? 2 : 4)) + f_off;
    // 12 i = 8 i + 4 i; in assembly because the compiler folds the two shift-adds back into a 32-bit multiply
    if (stride == 3) asm("v_lshl_add_u32 %0, %1, 3, %2" : "=v"(lin) : "v"(ui), "v"(lin));
    return __umul24(row, f_row) + lin;
  };
  // The weight stream is software-pipelined: batch k+1's weights are requested before batch k is consumed (their
  // addresses depend on no data), so an iteration waits for one memory round trip -- its gathers -- instead of two.
  // ic: the batch's candidate indices, clamped into the list (a candidate past its end reads the last one's weight
  // and texel; its weight is replaced by -1)
  float wn[kU];
  int ic[kU];
#pragma unroll
  for (int u = 0; u < kU; u++) { wn[u] = -1.0f; ic[u] = min(g + kLanes * u, n - 1); }
  if (n > 0) {
#pragma unroll
    for (int u = 0; u < kU; u++) wn[u] = load_w(ic[u]);
  }
  find_face(g);
  for (int i0 = g; i0 < n; i0 += kLanes * kU) {
    float w[kU];
    uint32_t off[kU];
    // Lanes walk their candidates in increasing order, so the face changes at most five times per texel: the table
    // is read only in iterations where some lane of the wave crosses a face end (past the END OF THE LIST the
    // clamped candidates stay in the last face).
    const bool cross = i0 + kLanes * (kU - 1) >= f_end && f_end < n;
    if (__any(cross)) {
#pragma unroll
      for (int u = 0; u < kU; u++) {
        find_face(ic[u]);
        off[u] = texel_offset(ic[u]);
      }
      find_face(min(i0 + kLanes * kU, n - 1));
    } else {
#pragma unroll
      for (int u = 0; u < kU; u++) off[u] = texel_offset(ic[u]);
    }
    // all kU gathers, unconditionally (a rejected candidate, weight -1, still lies inside its face) ...
    float t0[kU], t1[kU], t2[kU];
#pragma unroll
    for (int u = 0; u < kU; u++) {
      const float* t = reinterpret_cast<const float*>(tbase + off[u]);
      t0[u] = t[0]; t1[u] = t[1]; t2[u] = t[2];
    }
    // ... then this batch's weights and the request for the next batch's
#pragma unroll
    for (int u = 1; u < kU; u++) w[u] = i0 + kLanes * u < n ? wn[u] : -1.0f;
    // candidate 0 is always inside the list; the explicit move frees wn[0] for the load below (left to the compiler,
    // the copy lands at the end of the loop, behind a wait for that load)
    asm volatile("v_mov_b32 %0, %1" : "=v"(w[0]) : "v"(wn[0]));
#pragma unroll
    for (int u = 0; u < kU; u++) {
      ic[u] = min(i0 + kLanes * (kU + u), n - 1);
      wn[u] = load_w(ic[u]);
    }
    // every gathered value is used here whatever its weight: the compiler must not sink a gather below the sign
    // test of its weight (it did: a second, dependent round trip per batch)
#pragma unroll
    for (int u = 0; u < kU; u++) asm volatile("" : "+v"(t0[u]), "+v"(t1[u]), "+v"(t2[u]));
    // -1 marks candidates outside the cone: they never touch an accumulator (0 * Inf).  The products are formed for
    // every candidate and ADDED under an execution mask of the lanes with w >= 0 (false for a NaN weight, like the
    // comparison in C++): five vector instructions per candidate where the compiler's select per accumulator takes nine.
#pragma unroll
    for (int u = 0; u < kU; u++) {
      const pbr_f2 wp = {w[u], t2[u] * w[u]};
      const pbr_f2 p01 = {t0[u] * w[u], t1[u] * w[u]};
      unsigned long long saved;
      asm volatile("s_mov_b64 %[sv], exec\n\t"
                   "v_cmpx_le_f32_e32 vcc, 0, %[w]\n\t"
                   "v_pk_add_f32 %[a01], %[a01], %[p01]\n\t"
                   "v_pk_add_f32 %[aw2], %[aw2], %[wp]\n\t"
                   "s_mov_b64 exec, %[sv]"
                   : [a01] "+v"(acc01), [aw2] "+v"(accw2), [sv] "=&s"(saved)
                   : [w] "v"(w[u]), [p01] "v"(p01), [wp] "v"(wp)
                   : "vcc");
    }
  }
  float c0 = acc01.x, c1 = acc01.y, c2 = accw2.y, wsum = accw2.x;
  c0 = group_sum_last<kLanes>(c0); c1 = group_sum_last<kLanes>(c1); c2 = group_sum_last<kLanes>(c2);
  if (!kBackward) wsum = group_sum_last<kLanes>(wsum);
  if (g == kLanes - 1 && valid) {
    if (kBackward) {
      float* q = dst + 3 * (size_t)o;
      q[0] = c0; q[1] = c1; q[2] = c2;
    } else if (kNorm) {
      float* q = dst + 3 * (size_t)o;
      q[0] = c0 / wsum; q[1] = c1 / wsum; q[2] = c2 / wsum;
      wsum_out[o] = wsum;
    } else {
      float* q = dst + 4 * (size_t)o;
      q[0] = c0; q[1] = c1; q[2] = c2; q[3] = wsum;
    }
  }
}

template <bool kBackward, bool kNorm, int kLanes>
__global__ void __launch_bounds__(256)
specular_apply_kernel(int N, const float* __restrict__ src, const float* __restrict__ bounds,
                      const uint32_t* __restrict__ offsets, const float* __restrict__ W,
                      float* __restrict__ dst, float* __restrict__ wsum_out) {
  specular_apply_body<kBackward, kNorm, kLanes>(blockIdx.x, N, src, bounds, offsets, W, dst, wsum_out);
}

// All levels of the chain in ONE launch (gigs_specular_cubemap_multi_*): the levels are independent, so their
// workgroups share one grid -- the largest level first -- instead of five dependent launches (five kernel nodes with
// 10-17 us of dispatch latency between them on the light's side stream, each with its own under-filled tail).
struct SpecLevel {
  int N, lanes, block_begin;
  const float* src;
  const float* bounds;
  const uint32_t* offsets;
  const float* W;
  float* dst;
  float* wsum_out;
};
struct SpecLevels { int n; SpecLevel lv[8]; };

template <bool kBackward>
__global__ void __launch_bounds__(256) specular_apply_multi_kernel(SpecLevels L) {
  int k = 0;
#pragma unroll
  for (int i = 1; i < 8; i++)
    if (i < L.n && (int)blockIdx.x >= L.lv[i].block_begin) k = i;
  const SpecLevel& v = L.lv[k];
  const int block = (int)blockIdx.x - v.block_begin;
  if (v.lanes == 8) specular_apply_body<kBackward, true, 8>(block, v.N, v.src, v.bounds, v.offsets, v.W, v.dst, v.wsum_out);
  else if (v.lanes == 16) specular_apply_body<kBackward, true, 16>(block, v.N, v.src, v.bounds, v.offsets, v.W, v.dst, v.wsum_out);
  else specular_apply_body<kBackward, true, 64>(block, v.N, v.src, v.bounds, v.offsets, v.W, v.dst, v.wsum_out);
}

// tuning knobs (gigs_options.spec_max8 / spec_max16): largest mean window served by 8- and by 16-lane groups
static int spec_lanes_for(const Options& o, int avg_window) {
  return (avg_window > 0 && avg_window <= o.spec_max8) ? 8 : (avg_window > 0 && avg_window <= o.spec_max16) ? 16 : 64;
}

template <bool kBackward, bool kNorm>
static void launch_specular_apply(const Options& o, int res, int avg_window, const float* src, const float* bounds,
                                  const uint32_t* offsets, const float* W, float* dst, float* wsum_out, hipStream_t s) {
  const int total = 6 * res * res;
  const int max8 = o.spec_max8, max16 = o.spec_max16;
  if (avg_window > 0 && avg_window <= max8) {
    const int waves = (total + 7) / 8;
    hipLaunchKernelGGL((specular_apply_kernel<kBackward, kNorm, 8>), dim3((waves + 3) / 4), dim3(256), 0, s, res, src,
                       bounds, offsets, W, dst, wsum_out);
  } else if (avg_window > 0 && avg_window <= max16) {
    const int waves = (total + 3) / 4;
    hipLaunchKernelGGL((specular_apply_kernel<kBackward, kNorm, 16>), dim3((waves + 3) / 4), dim3(256), 0, s, res, src,
                       bounds, offsets, W, dst, wsum_out);
  } else {
    hipLaunchKernelGGL((specular_apply_kernel<kBackward, kNorm, 64>), dim3((total + 3) / 4), dim3(256), 0, s, res, src,
                       bounds, offsets, W, dst, wsum_out);
  }
}

// ------------------------------------------------------------------------------------------
// Backward of the filter for gradients that are mostly exact zeros (gigs_specular_cubemap_multi_bwd_sparse).
// The shade backward zero-fills the level gradients and adds into the sampled texels only, so a fine level receives a
// few thousand nonzero texels (or none: every pixel rougher than the level's range).  The gather above still streams
// the level's whole table.  Instead: a census lists the nonzero texels of every level, and a level whose list fits its
// capacity is summed from them with their runs of the forward table (the tile gather below) -- W_fwd[o][i] is the same
// float as W_swapped[i][o] (specular_weights_kernel evaluates one expression for both), so (w / wsum[o]) * g[o] is the
// very product the gather forms from its pre-divided table; only the order of the additions differs.
// state: [0..7] working counters, [8..15] path taken (1 sparse, 0 gather), [16..23] nonzero texels counted.
// ------------------------------------------------------------------------------------------
struct SparseLevel {
  int total, cap, block_begin, unit_begin, N;
  int vec;    // src and dst are 16-byte aligned: the census may use 16-byte accesses
  int narrow; // scattered, one wave per slot, instead of the tile gather
  int nt;     // tiles along a face edge
  int parts;  // slices of the list, i.e. workgroups per tile
  const float* src;
  float* dst;
  const float* bounds;
  const uint32_t* offsets;
  const float* Wfwd;
  const float* wsum;
  int* list;
};
struct SparseLevels { int n; SparseLevel lv[8]; };

constexpr int kCensusPerThread = 4;  // texels per thread: 48 contiguous bytes of gradient, three 16-byte loads

// One pass over the incoming gradients of all levels: dst = 0, and the indices of the texels with a channel != 0
// (true for NaN, false for -0) go to the level's list.  A workgroup claims its slots with ONE returning atomic on the
// level's counter; the counter keeps counting past the capacity (the count decides the path), the list does not grow past it.
__global__ void __launch_bounds__(256) specular_census_kernel(SparseLevels L, int* __restrict__ state) {
  int k = 0;
#pragma unroll
  for (int i = 1; i < 8; i++)
    if (i < L.n && (int)blockIdx.x >= L.lv[i].block_begin) k = i;
  const SparseLevel& v = L.lv[k];
  const int lane = threadIdx.x & 63;
  const int t0 = (((int)blockIdx.x - v.block_begin) * 256 + (int)threadIdx.x) * kCensusPerThread;
  bool nz[kCensusPerThread];
  if (v.vec && t0 + kCensusPerThread <= v.total) {
    // texel index a multiple of 4: byte offset a multiple of 48 from an aligned base
    const float4* s4 = reinterpret_cast<const float4*>(v.src + 3 * (size_t)t0);
    float4* d4 = reinterpret_cast<float4*>(v.dst + 3 * (size_t)t0);
    const float4 a = s4[0], b = s4[1], c = s4[2];
    nz[0] = a.x != 0.0f || a.y != 0.0f || a.z != 0.0f;
    nz[1] = a.w != 0.0f || b.x != 0.0f || b.y != 0.0f;
    nz[2] = b.z != 0.0f || b.w != 0.0f || c.x != 0.0f;
    nz[3] = c.y != 0.0f || c.z != 0.0f || c.w != 0.0f;
    const float4 z = {0.0f, 0.0f, 0.0f, 0.0f};
    d4[0] = z; d4[1] = z; d4[2] = z;
  } else {
#pragma unroll
    for (int j = 0; j < kCensusPerThread; j++) {
      nz[j] = false;
      if (t0 + j < v.total) {
        const float* s = v.src + 3 * (size_t)(t0 + j);
        float* d = v.dst + 3 * (size_t)(t0 + j);
        nz[j] = s[0] != 0.0f || s[1] != 0.0f || s[2] != 0.0f;
        d[0] = 0.0f; d[1] = 0.0f; d[2] = 0.0f;
      }
    }
  }
  unsigned long long m[kCensusPerThread];
  int wave_total = 0;
#pragma unroll
  for (int j = 0; j < kCensusPerThread; j++) { m[j] = __ballot(nz[j]); wave_total += __popcll(m[j]); }
  // one returning atomic per workgroup: 1536 waves of a 256^2 level adding to one address took 15 us
  __shared__ int wave_base[5];
  const int wave = threadIdx.x >> 6;
  if (lane == 0) wave_base[wave] = wave_total;
  __syncthreads();
  if (threadIdx.x == 0) {
    const int t01 = wave_base[0] + wave_base[1], t012 = t01 + wave_base[2], all = t012 + wave_base[3];
    const int first = all ? atomicAdd(state + k, all) : 0;
    wave_base[3] = first + t012; wave_base[2] = first + t01; wave_base[1] = first + wave_base[0]; wave_base[0] = first;
  }
  __syncthreads();
  if (wave_total == 0) return;  // wave-uniform
  int base = wave_base[wave];
  const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
  for (int j = 0; j < kCensusPerThread; j++) {
    const int slot = base + __popcll(m[j] & below);
    if (nz[j] && slot < v.cap) v.list[slot] = t0 + j;
    base += __popcll(m[j]);
  }
}

// Sparse levels are summed ON CHIP by the owners of the destination texels.  A workgroup owns one kSpTile x kSpTile tile
// of one face and one slice of kSpSlice slots of the level's list: a tile next to a highlight sees thousands of listed
// texels, so a tile's sources are split over `parts` workgroups, one slice each.
//   * test: a thread takes a slot o of the slice and o's OWN rectangle on the tile's face (the pinned meaning of a sparse
//     level is the forward table's runs; the bounds are not symmetric everywhere); the slots whose rectangle meets the
//     tile are packed into LDS records in slot order (ballots and a prefix over the waves: no LDS atomics);
//   * sum: a wave owns an 8 x 8 quadrant, a lane one texel.  The wave lists the records that meet its quadrant (in record
//     order) and walks that list: a record is wave-uniform, so the lanes inside its rectangle read 8 contiguous pieces
//     of o's run; kSpU records are in flight per lane, each with an accumulator of its own, and the accumulators are
//     folded in a fixed tree.  The product is the gather's: (w / wsum[o]) * g[o], markers (w < 0, and a NaN weight)
//     skipped, a NaN quotient kept;
//   * the tile is written once: stored where the level has one slice, else added to dst (zeroed by the census) with one
//     atomic per texel, channel and slice -- never one per pair.
// No workgroup waits for another.  A workgroup whose slice lies past the count returns at entry.
constexpr int kSpTile = 16;
constexpr int kSpSlice = 256;  // one slot per thread
constexpr int kSpU = 8;

__device__ __forceinline__ void specular_tile_gather_body(const SparseLevel& v, int unit, int count) {
  const int N = v.N, nt = v.nt, tiles = 6 * nt * nt;
  const int part = unit / tiles, tile = unit - part * tiles;
  const int slot = part * kSpSlice + (int)threadIdx.x, end = min(count, v.cap);
  if (part * kSpSlice >= end) return;  // uniform over the workgroup
  const int face = tile / (nt * nt), tt = tile - face * nt * nt;
  const int tx0 = (tt % nt) * kSpTile, ty0 = (tt / nt) * kSpTile;
  const int tx1 = min(tx0 + kSpTile, N) - 1, ty1 = min(ty0 + kSpTile, N) - 1;
  const int lane = threadIdx.x & 63, wave = (int)threadIdx.x >> 6;

  __shared__ uint32_t r_base[kSpSlice];  // index into Wfwd of the rectangle's (virtual) texel (0, 0), modulo 2^32
  __shared__ int r_wd[kSpSlice], r_x[kSpSlice], r_y[kSpSlice];  // row length; xmin | xmax << 16; ymin | ymax << 16
  __shared__ float r_ws[kSpSlice], r_g0[kSpSlice], r_g1[kSpSlice], r_g2[kSpSlice];
  __shared__ unsigned short q_rec[4][kSpSlice];  // per wave: the records that meet its quadrant
  __shared__ int wave_cnt[4];

  bool hit = false;
  int wd = 0, px = 0, py = 0;
  uint32_t t_base = 0;
  float t_ws = 0.0f, t_g0 = 0.0f, t_g1 = 0.0f, t_g2 = 0.0f;
  if (slot < end) {
    const int o = v.list[slot];
    const float4 b = reinterpret_cast<const float4*>(v.bounds + 24 * (size_t)o)[face];
    const int xmin = (int)b.x, xmax = (int)b.y, ymin = (int)b.z, ymax = (int)b.w;
    hit = xmin <= xmax && ymin <= ymax && xmin <= tx1 && xmax >= tx0 && ymin <= ty1 && ymax >= ty0;
    if (hit) {
      wd = xmax - xmin + 1; px = xmin | (xmax << 16); py = ymin | (ymax << 16);
      t_base = v.offsets[6 * (size_t)o + face] - (uint32_t)(ymin * wd + xmin);
      t_ws = v.wsum[o];
      const float* g = v.src + 3 * (size_t)o;
      t_g0 = g[0]; t_g1 = g[1]; t_g2 = g[2];
    }
  }
  const unsigned long long hits = __ballot(hit);
  if (lane == 0) wave_cnt[wave] = __popcll(hits);
  __syncthreads();
  int n_rec = 0, first = 0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    if (j == wave) first = n_rec;
    n_rec += wave_cnt[j];
  }
  if (n_rec == 0) return;  // uniform over the workgroup
  if (hit) {
    const int j = first + __popcll(hits & ((1ull << lane) - 1ull));
    r_base[j] = t_base; r_wd[j] = wd; r_x[j] = px; r_y[j] = py;
    r_ws[j] = t_ws; r_g0[j] = t_g0; r_g1[j] = t_g1; r_g2[j] = t_g2;
  }
  __syncthreads();

  const int qx0 = tx0 + (wave & 1) * 8, qy0 = ty0 + (wave >> 1) * 8;
  if (qx0 >= N || qy0 >= N) return;  // uniform over the wave; no barrier follows
  // the records that meet this wave's quadrant, in record order
  unsigned short* mine = q_rec[wave];
  int n_q = 0;
  for (int j0 = 0; j0 < n_rec; j0 += 64) {
    const int j = j0 + lane;
    bool t = false;
    if (j < n_rec) {
      const int xr = r_x[j], yr = r_y[j];
      t = (xr & 0xffff) <= qx0 + 7 && (xr >> 16) >= qx0 && (yr & 0xffff) <= qy0 + 7 && (yr >> 16) >= qy0;
    }
    const unsigned long long m = __ballot(t);
    if (t) mine[n_q + __popcll(m & ((1ull << lane) - 1ull))] = (unsigned short)j;
    n_q += __popcll(m);
  }
  if (n_q == 0) return;
  // written and read by lanes of the same wave only: LDS operations of a wave complete in order
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");

  const int x = qx0 + (lane & 7), y = qy0 + (lane >> 3);
  const bool inside = x < N && y < N;
  float a0[kSpU], a1[kSpU], a2[kSpU];
#pragma unroll
  for (int u = 0; u < kSpU; u++) { a0[u] = 0.0f; a1[u] = 0.0f; a2[u] = 0.0f; }
  for (int i0 = 0; i0 < n_q; i0 += kSpU) {
    float w[kSpU];
    int rec[kSpU];
#pragma unroll
    for (int u = 0; u < kSpU; u++) {
      const int j = mine[min(i0 + u, n_q - 1)];
      rec[u] = j;
      const int xr = r_x[j], yr = r_y[j];
      const bool in = inside && i0 + u < n_q && x >= (xr & 0xffff) && x <= (xr >> 16) && y >= (yr & 0xffff) && y <= (yr >> 16);
      // every lane loads (a lane outside the rectangle reads its first weight, one line for all of them): kSpU
      // independent loads in flight, no branch between them
      const int rw = r_wd[j];
      const uint32_t at = in ? (uint32_t)(y * rw + x) : (uint32_t)((yr & 0xffff) * rw + (xr & 0xffff));
      const float wl = v.Wfwd[(size_t)(uint32_t)(r_base[j] + at)];
      w[u] = in ? wl : -1.0f;
    }
#pragma unroll
    for (int u = 0; u < kSpU; u++) {
      const int j = rec[u];
      if (w[u] >= 0.0f) {  // -1 marks a candidate outside the cone; a NaN quotient (0 / 0) reaches dst like the gather's
        const float q = w[u] / r_ws[j];
        a0[u] += q * r_g0[j]; a1[u] += q * r_g1[j]; a2[u] += q * r_g2[j];
      }
    }
  }
#pragma unroll
  for (int h = kSpU / 2; h > 0; h >>= 1)
#pragma unroll
    for (int u = 0; u < h; u++) { a0[u] += a0[u + h]; a1[u] += a1[u + h]; a2[u] += a2[u + h]; }
  if (!inside) return;
  float* d = v.dst + 3 * ((size_t)(face * N + y) * N + x);
  const float val[3] = {a0[0], a1[0], a2[0]};
#pragma unroll
  for (int c = 0; c < 3; c++) {
    if (!(val[c] != 0.0f)) continue;  // dst holds the census' zeros
    if (v.parts == 1) d[c] = val[c];
    else atomicAdd(d + c, val[c]);
  }
}

// A level whose windows are no wider than a tile (the 256^2 level: 81 candidates a window) is SCATTERED instead, one
// wave per slot of its list: there the tile gather's test -- tiles x listed texels -- outweighs the sums, and the
// scatter's adds are few (measured, tools/spec_sparse_sweep.py).  A lane forms the quotient w / wsum[o] and the texel of
// ONE candidate; the adds are then issued by DWORD of dst -- three instructions per 64 candidates, lane L of instruction
// j adding channel (64 j + L) % 3 of candidate (64 j + L) / 3, fetched from that candidate's lane -- so that one atomic
// instruction covers 64 consecutive floats of dst wherever the window's row goes on (256 contiguous bytes, the shape the
// memory-side adders take at full rate).  The run of the table and the face rectangles are read exactly as
// specular_apply_body reads them: rectangles in face order, row-major inside one.
constexpr int kScatterU = 2;  // weights requested before one is consumed

__device__ __forceinline__ void specular_scatter_body(const SparseLevel& v, int slot, int count) {
  const int lane = threadIdx.x & 63;
  if (slot >= count || slot >= v.cap) return;  // past the end of the list
  const int o = __builtin_amdgcn_readfirstlane(v.list[slot]);
  const int N = v.N;
  int pre[7], wd[6], base[6];
  float inv[6];
  pre[0] = 0;
  const float4* b4 = reinterpret_cast<const float4*>(v.bounds + 24 * (size_t)o);
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    const float4 b = b4[s];
    const int xmin = (int)b.x, xmax = (int)b.y, ymin = (int)b.z, ymax = (int)b.w;
    const bool empty = xmin > xmax || ymin > ymax;
    wd[s] = empty ? 1 : xmax - xmin + 1;
    inv[s] = 1.0f / (float)wd[s];  // as specular_weights_kernel laid the run out
    pre[s + 1] = pre[s] + (empty ? 0 : wd[s] * (ymax - ymin + 1));
    base[s] = empty ? 0 : (s * N + ymin) * N + xmin;
  }
  const int n = pre[6];
  const float* W = v.Wfwd + v.offsets[6 * (size_t)o];
  const float ws = v.wsum[o];
  const float* g = v.src + 3 * (size_t)o;
  const float g0 = g[0], g1 = g[1], g2 = g[2];
  // lane L of add instruction j: candidate lane (64 j + L) / 3 and channel (64 j + L) % 3
  int from[3];
  float gch[3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const int D = 64 * j + lane, ch = D % 3;
    from[j] = D / 3;
    gch[j] = ch == 0 ? g0 : ch == 1 ? g1 : g2;
  }
  const int ch0 = lane % 3;  // channels of the three instructions: ch0, (ch0 + 1) % 3, (ch0 + 2) % 3 (64 % 3 = 1)
  for (int c0 = 0; c0 < n; c0 += 64 * kScatterU) {
    float w[kScatterU];
#pragma unroll
    for (int u = 0; u < kScatterU; u++) {
      const int c = c0 + u * 64 + lane;
      w[u] = c < n ? W[c] : -1.0f;  // -1 marks a candidate outside the cone
    }
#pragma unroll
    for (int u = 0; u < kScatterU; u++) {
      if (c0 + u * 64 >= n) break;  // wave-uniform
      const int c = c0 + u * 64 + lane;
      float q = -1.0f;
      int texel = 0;
      if (w[u] >= 0.0f) {
        int f = 0;
#pragma unroll
        for (int j = 1; j < 6; j++) f += c >= pre[j] ? 1 : 0;  // the last face with pre <= c: empty faces are skipped
        int f_pre = pre[0], f_wd = wd[0], f_base = base[0];
        float f_inv = inv[0];
#pragma unroll
        for (int j = 1; j < 6; j++)
          if (f == j) { f_pre = pre[j]; f_wd = wd[j]; f_base = base[j]; f_inv = inv[j]; }
        const int loc = c - f_pre;
        const int row = (int)(((float)loc + 0.5f) * f_inv);
        texel = f_base + row * N + (loc - row * f_wd);
        q = w[u] / ws;  // the float the gather's pre-divided table holds for this pair
      }
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const float qq = __shfl(q, from[j]);
        const int tt = __shfl(texel, from[j]);
        const int ch = ch0 + j >= 3 ? ch0 + j - 3 : ch0 + j;
        const float val = qq * gch[j];
        // NaN quotients (0 / 0) must reach dst like the gather's: only the -1 marker and exact zeros are skipped
        if (!(qq < 0.0f) && val != 0.0f) atomicAdd(v.dst + 3 * (size_t)tt + ch, val);
      }
    }
  }
}

// One launch behind the census for every level of the chain: the tile workgroups of the sparse levels first (tile gather or scatter; they wait
// for memory round trips, the gather for bandwidth: started together they overlap), then specular_apply_multi_kernel<true>'s
// workgroups.  Each workgroup reads its level's count and returns at entry where the level took the other path.
__global__ void __launch_bounds__(256)
specular_apply_multi_bwd_sparse_kernel(SpecLevels L, SparseLevels S, int tile_units, const int* __restrict__ state) {
  if ((int)blockIdx.x < tile_units) {
    int k = 0;
#pragma unroll
    for (int i = 1; i < 8; i++)
      if (i < S.n && (int)blockIdx.x >= S.lv[i].unit_begin) k = i;
    const SparseLevel& v = S.lv[k];
    const int count = state[k];
    if (count > v.cap) return;  // a gathered level
    const int unit = (int)blockIdx.x - v.unit_begin;
    if (v.narrow) specular_scatter_body(v, unit * 4 + ((int)threadIdx.x >> 6), count);
    else specular_tile_gather_body(v, unit, count);
    return;
  }
  const int gblock = (int)blockIdx.x - tile_units;
  int k = 0;
#pragma unroll
  for (int i = 1; i < 8; i++)
    if (i < L.n && gblock >= L.lv[i].block_begin) k = i;
  if (state[k] <= S.lv[k].cap) return;  // a sparse level
  const SpecLevel& v = L.lv[k];
  const int block = gblock - v.block_begin;
  if (v.lanes == 8) specular_apply_body<true, true, 8>(block, v.N, v.src, v.bounds, v.offsets, v.W, v.dst, v.wsum_out);
  else if (v.lanes == 16) specular_apply_body<true, true, 16>(block, v.N, v.src, v.bounds, v.offsets, v.W, v.dst, v.wsum_out);
  else specular_apply_body<true, true, 64>(block, v.N, v.src, v.bounds, v.offsets, v.W, v.dst, v.wsum_out);
}

// Runs last: the report the caller may read, and the working counters cleared for the next call (every workgroup of the
// launch before it has read its level's count by then).
struct SparseCaps { int n; int cap[8]; };
__global__ void __launch_bounds__(64) specular_sparse_finish_kernel(SparseCaps c, int* __restrict__ state) {
  const int t = threadIdx.x;
  if (t >= 8) return;
  const int count = state[t];
  if (t < c.n) {
    state[8 + t] = count <= c.cap[t] ? 1 : 0;
    state[16 + t] = count;
  }
  state[t] = 0;
}

// The forward over the listed texels of the fine levels (gigs_specular_cubemap_multi_fwd_sparse), one launch behind the
// list census: first the workgroups of the listed texels -- a level's capacity worth of groups; a workgroup past the
// count returns at entry --, then specular_apply_multi_kernel<false>'s workgroups for the levels whose count exceeds
// their capacity (they return at entry where the level is listed).  Same report in `state` as the backward's.
__global__ void __launch_bounds__(256)
specular_apply_multi_fwd_sparse_kernel(SpecLevels L, SparseLevels S, int listed_blocks, const int* __restrict__ state) {
  if ((int)blockIdx.x < listed_blocks) {
    int k = 0;
#pragma unroll
    for (int i = 1; i < 8; i++)
      if (i < S.n && (int)blockIdx.x >= S.lv[i].unit_begin) k = i;
    const SparseLevel& q = S.lv[k];
    const int count = state[k];
    if (count > q.cap) return;  // a dense level
    const SpecLevel& v = L.lv[k];
    const int block = (int)blockIdx.x - q.unit_begin;
    if (block * 4 * (64 / v.lanes) >= count) return;  // uniform over the workgroup
    if (v.lanes == 8) specular_apply_body<false, true, 8, true>(block, v.N, v.src, v.bounds, v.offsets, v.W, v.dst, v.wsum_out, q.list, count);
    else if (v.lanes == 16) specular_apply_body<false, true, 16, true>(block, v.N, v.src, v.bounds, v.offsets, v.W, v.dst, v.wsum_out, q.list, count);
    else specular_apply_body<false, true, 64, true>(block, v.N, v.src, v.bounds, v.offsets, v.W, v.dst, v.wsum_out, q.list, count);
    return;
  }
  const int gblock = (int)blockIdx.x - listed_blocks;
  int k = 0;
#pragma unroll
  for (int i = 1; i < 8; i++)
    if (i < L.n && gblock >= L.lv[i].block_begin) k = i;
  if (state[k] <= S.lv[k].cap) return;  // a listed level
  const SpecLevel& v = L.lv[k];
  const int block = gblock - v.block_begin;
  if (v.lanes == 8) specular_apply_body<false, true, 8>(block, v.N, v.src, v.bounds, v.offsets, v.W, v.dst, v.wsum_out);
  else if (v.lanes == 16) specular_apply_body<false, true, 16>(block, v.N, v.src, v.bounds, v.offsets, v.W, v.dst, v.wsum_out);
  else specular_apply_body<false, true, 64>(block, v.N, v.src, v.bounds, v.offsets, v.W, v.dst, v.wsum_out);
}

static int spec_sparse_capacity(const Options& o, int res) {
  return (int)((long long)6 * res * res * o.spec_sparse_permille / 1000);
}

}  // namespace gigs

// ------------------------------------------------------------------------------------------
// C ABI (declared in include/gigs_hip.h)
// ------------------------------------------------------------------------------------------
#include "gigs_internal.h"

extern "C" {

int gigs_diffuse_cubemap_fwd(int res, const float* cubemap, float* out, void* stream) {
  if (res <= 0 || !cubemap || !out) return gigs_internal_fail(GIGS_ERR_INVALID, "diffuse_cubemap_fwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const float4* table = gigs::texel_table(res, s);
  if (!table) return gigs_internal_fail(GIGS_ERR_HIP, "texel table");
  gigs::StageTimer timer(gigs::Stage::kCubemapFwd, stream);
  hipLaunchKernelGGL(gigs::diffuse_cubemap_kernel<false>, dim3((6 * res * res + 3) / 4), dim3(256), 0, s, res, table, cubemap, out);
  return gigs_internal_check_launch("diffuse_cubemap_fwd");
}

int gigs_diffuse_cubemap_bwd(int res, const float* grad_out, float* grad_cubemap, void* stream) {
  if (res <= 0 || !grad_out || !grad_cubemap) return gigs_internal_fail(GIGS_ERR_INVALID, "diffuse_cubemap_bwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const float4* table = gigs::texel_table(res, s);
  if (!table) return gigs_internal_fail(GIGS_ERR_HIP, "texel table");
  gigs::StageTimer timer(gigs::Stage::kCubemapBwd, stream);
  hipLaunchKernelGGL(gigs::diffuse_cubemap_kernel<true>, dim3((6 * res * res + 3) / 4), dim3(256), 0, s, res, table, grad_out, grad_cubemap);
  return gigs_internal_check_launch("diffuse_cubemap_bwd");
}

int gigs_specular_bounds(int res, float costheta_cutoff, float* bounds, void* stream) {
  if (res <= 0 || !bounds) return gigs_internal_fail(GIGS_ERR_INVALID, "specular_bounds: bad argument");
  hipLaunchKernelGGL(gigs::specular_bounds_kernel, dim3((6 * res * res + 63) / 64), dim3(64), 0, (hipStream_t)stream, res, costheta_cutoff, bounds);
  return gigs_internal_check_launch("specular_bounds");
}

int gigs_specular_cubemap_fwd(int res, const float* cubemap, const float* bounds, float roughness,
                              float costheta_cutoff, float* out, void* stream) {
  if (res <= 0 || !cubemap || !bounds || !out) return gigs_internal_fail(GIGS_ERR_INVALID, "specular_cubemap_fwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const float4* table = gigs::texel_table(res, s);
  if (!table) return gigs_internal_fail(GIGS_ERR_HIP, "texel table");
  gigs::StageTimer timer(gigs::Stage::kCubemapFwd, stream);
  hipLaunchKernelGGL(gigs::specular_cubemap_kernel<false>, dim3((6 * res * res + 3) / 4), dim3(256), 0, s, res, table, cubemap, bounds, roughness, costheta_cutoff, out);
  return gigs_internal_check_launch("specular_cubemap_fwd");
}

int gigs_specular_cubemap_bwd(int res, const float* bounds, const float* grad_out, float roughness,
                              float costheta_cutoff, float* grad_cubemap, void* stream) {
  if (res <= 0 || !bounds || !grad_out || !grad_cubemap) return gigs_internal_fail(GIGS_ERR_INVALID, "specular_cubemap_bwd: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const float4* table = gigs::texel_table(res, s);
  if (!table) return gigs_internal_fail(GIGS_ERR_HIP, "texel table");
  const int symmetric = gigs::window_symmetric(res, costheta_cutoff, s);
  if (symmetric < 0) return gigs_internal_fail(GIGS_ERR_HIP, "specular_cubemap_bwd: symmetry verdict");
  gigs::StageTimer timer(gigs::Stage::kCubemapBwd, stream);
  const dim3 grid((6 * res * res + 3) / 4);
  if (symmetric) {
    hipLaunchKernelGGL(gigs::specular_cubemap_kernel<true>, grid, dim3(256), 0, s, res, table, grad_out, bounds, roughness, costheta_cutoff, grad_cubemap);
  } else {
    if (hipMemsetAsync(grad_cubemap, 0, (size_t)18 * res * res * sizeof(float), s) != hipSuccess)
      return gigs_internal_fail(GIGS_ERR_HIP, "specular_cubemap_bwd: clearing the gradient");
    hipLaunchKernelGGL((gigs::specular_cubemap_kernel<false, true>), grid, dim3(256), 0, s, res, table, grad_out, bounds, roughness, costheta_cutoff, grad_cubemap);
  }
  return gigs_internal_check_launch("specular_cubemap_bwd");
}

int gigs_specular_window_symmetric(int res, float costheta_cutoff, void* stream) {
  if (res <= 0) return gigs_internal_fail(GIGS_ERR_INVALID, "specular_window_symmetric: bad argument");
  const int symmetric = gigs::window_symmetric(res, costheta_cutoff, (hipStream_t)stream);
  if (symmetric < 0) return gigs_internal_fail(GIGS_ERR_HIP, "specular_window_symmetric");
  return symmetric;
}

int gigs_specular_cubemap_bwd_scatter_w(int res, const float* bounds, const uint32_t* offsets, const float* weights_fwd,
                                        const float* wsum, const float* grad_out, int grad_is_rgb, float* grad_cubemap,
                                        void* stream) {
  if (res <= 0 || !bounds || !offsets || !weights_fwd || !grad_out || !grad_cubemap)
    return gigs_internal_fail(GIGS_ERR_INVALID, "specular_cubemap_bwd_scatter_w: bad argument");
  hipStream_t s = (hipStream_t)stream;
  gigs::StageTimer timer(gigs::Stage::kCubemapBwd, stream);
  if (hipMemsetAsync(grad_cubemap, 0, (size_t)18 * res * res * sizeof(float), s) != hipSuccess)
    return gigs_internal_fail(GIGS_ERR_HIP, "specular_cubemap_bwd_scatter_w: clearing the gradient");
  hipLaunchKernelGGL(gigs::specular_table_scatter_kernel, dim3((6 * res * res + 3) / 4), dim3(256), 0, s, res, grad_out,
                     grad_is_rgb ? 3 : 4, bounds, offsets, weights_fwd, wsum, grad_cubemap);
  return gigs_internal_check_launch("specular_cubemap_bwd_scatter_w");
}

int gigs_specular_weights(int res, const float* bounds, const uint32_t* offsets, float roughness,
                          float costheta_cutoff, int swap_roles, float* weights, void* stream) {
  if (res <= 0 || !bounds || !offsets || !weights) return gigs_internal_fail(GIGS_ERR_INVALID, "specular_weights: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const float4* table = gigs::texel_table(res, s);
  if (!table) return gigs_internal_fail(GIGS_ERR_HIP, "texel table");
  const dim3 grid((6 * res * res + 3) / 4);
  if (swap_roles)
    hipLaunchKernelGGL(gigs::specular_weights_kernel<true>, grid, dim3(256), 0, s, res, table, bounds, offsets, roughness, costheta_cutoff, weights);
  else
    hipLaunchKernelGGL(gigs::specular_weights_kernel<false>, grid, dim3(256), 0, s, res, table, bounds, offsets, roughness, costheta_cutoff, weights);
  return gigs_internal_check_launch("specular_weights");
}

int gigs_specular_weights_divide(int res, const float* bounds, const uint32_t* offsets, const float* weights,
                                 const float* texel_divisor, float* out_weights, void* stream) {
  if (res <= 0 || !bounds || !offsets || !weights || !texel_divisor || !out_weights)
    return gigs_internal_fail(GIGS_ERR_INVALID, "specular_weights_divide: bad argument");
  hipLaunchKernelGGL(gigs::specular_divide_weights_kernel, dim3((6 * res * res + 3) / 4), dim3(256), 0, (hipStream_t)stream,
                     res, bounds, offsets, weights, texel_divisor, out_weights);
  return gigs_internal_check_launch("specular_weights_divide");
}

int gigs_specular_cubemap_fwd_w(gigs_ctx* ctx, int res, const float* cubemap, const float* bounds, const uint32_t* offsets,
                                const float* weights, int avg_window, float* out, float* wsum_out, void* stream) {
  const gigs::Options& o = *gigs_internal_options(ctx);
  if (res <= 0 || !cubemap || !bounds || !offsets || !weights || !out) return gigs_internal_fail(GIGS_ERR_INVALID, "specular_cubemap_fwd_w: bad argument");
  hipStream_t s = (hipStream_t)stream;
  gigs::StageTimer timer(gigs::Stage::kCubemapFwd, stream);
  if (wsum_out)
    gigs::launch_specular_apply<false, true>(o, res, avg_window, cubemap, bounds, offsets, weights, out, wsum_out, s);
  else
    gigs::launch_specular_apply<false, false>(o, res, avg_window, cubemap, bounds, offsets, weights, out, nullptr, s);
  return gigs_internal_check_launch("specular_cubemap_fwd_w");
}

int gigs_specular_cubemap_bwd_w(gigs_ctx* ctx, int res, const float* bounds, const uint32_t* offsets, const float* weights_swapped,
                                int avg_window, const float* grad_out, int grad_is_rgb, float* grad_cubemap, void* stream) {
  const gigs::Options& o = *gigs_internal_options(ctx);
  if (res <= 0 || !bounds || !offsets || !weights_swapped || !grad_out || !grad_cubemap) return gigs_internal_fail(GIGS_ERR_INVALID, "specular_cubemap_bwd_w: bad argument");
  hipStream_t s = (hipStream_t)stream;
  gigs::StageTimer timer(gigs::Stage::kCubemapBwd, stream);
  if (grad_is_rgb)
    gigs::launch_specular_apply<true, true>(o, res, avg_window, grad_out, bounds, offsets, weights_swapped, grad_cubemap, nullptr, s);
  else
    gigs::launch_specular_apply<true, false>(o, res, avg_window, grad_out, bounds, offsets, weights_swapped, grad_cubemap, nullptr, s);
  return gigs_internal_check_launch("specular_cubemap_bwd_w");
}

// One level of a multi-level apply launch: its arrays, its lane group and its first workgroup; `blocks` advances past
// the level.  Returns the level's texel count.
static int fill_spec_level(const gigs::Options& o, const gigs_spec_level& a, gigs::SpecLevel& v, int& blocks) {
  v.N = a.res; v.lanes = gigs::spec_lanes_for(o, a.avg_window); v.block_begin = blocks;
  v.src = a.src; v.bounds = a.bounds; v.offsets = a.offsets; v.W = a.weights; v.dst = a.dst; v.wsum_out = a.wsum;
  const int total = 6 * a.res * a.res;
  const int waves = v.lanes == 64 ? total : (total + (64 / v.lanes) - 1) / (64 / v.lanes);
  blocks += (waves + 3) / 4;
  return total;
}

int gigs_specular_cubemap_multi_w(gigs_ctx* ctx, int n_levels, const gigs_spec_level* levels, int backward, void* stream) {
  const gigs::Options& o = *gigs_internal_options(ctx);
  if (n_levels <= 0 || n_levels > 8 || !levels) return gigs_internal_fail(GIGS_ERR_INVALID, "specular_cubemap_multi_w: bad level count");
  gigs::SpecLevels L;
  L.n = n_levels;
  int blocks = 0;
  for (int i = 0; i < n_levels; i++) {
    const gigs_spec_level& a = levels[i];
    if (a.res <= 0 || !a.src || !a.bounds || !a.offsets || !a.weights || !a.dst || (!backward && !a.wsum))
      return gigs_internal_fail(GIGS_ERR_INVALID, "specular_cubemap_multi_w: bad level");
    fill_spec_level(o, a, L.lv[i], blocks);
  }
  gigs::StageTimer timer(backward ? gigs::Stage::kCubemapBwd : gigs::Stage::kCubemapFwd, stream);
  if (backward) hipLaunchKernelGGL(gigs::specular_apply_multi_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, L);
  else hipLaunchKernelGGL(gigs::specular_apply_multi_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, L);
  return gigs_internal_check_launch("specular_cubemap_multi_w");
}

int gigs_spec_sparse_capacity(const gigs_ctx* ctx, int res) {
  if (res <= 0 || res > 4096) return gigs_internal_fail(GIGS_ERR_INVALID, "spec_sparse_capacity: bad resolution");
  return gigs::spec_sparse_capacity(*gigs_internal_options(ctx), res);
}

int gigs_specular_cubemap_multi_bwd_sparse(gigs_ctx* ctx, int n_levels, const gigs_spec_level* levels,
                                           const float* const* weights_fwd, const float* const* wsum, int* state,
                                           int* lists, void* stream) {
  const gigs::Options& o = *gigs_internal_options(ctx);
  if (!o.spec_sparse) return gigs_specular_cubemap_multi_w(ctx, n_levels, levels, 1, stream);
  if (n_levels <= 0 || n_levels > 8 || !levels || !weights_fwd || !wsum || !state || !lists)
    return gigs_internal_fail(GIGS_ERR_INVALID, "specular_cubemap_multi_bwd_sparse: bad argument");
  gigs::SpecLevels L;
  gigs::SparseLevels S;
  L.n = S.n = n_levels;
  int blocks = 0, census_blocks = 0, units = 0;
  gigs::SparseCaps caps = {};
  caps.n = n_levels;
  size_t list_begin = 0;
  for (int i = 0; i < n_levels; i++) {
    const gigs_spec_level& a = levels[i];
    if (a.res <= 0 || a.res > 4096 || !a.src || !a.bounds || !a.offsets || !a.weights || !a.dst || !weights_fwd[i] || !wsum[i])
      return gigs_internal_fail(GIGS_ERR_INVALID, "specular_cubemap_multi_bwd_sparse: bad level");
    const int total = fill_spec_level(o, a, L.lv[i], blocks);
    gigs::SparseLevel& q = S.lv[i];
    q.total = total; q.cap = gigs::spec_sparse_capacity(o, a.res); q.block_begin = census_blocks; q.unit_begin = units; q.N = a.res;
    q.vec = ((((uintptr_t)a.src) | ((uintptr_t)a.dst)) & 15) == 0;
    q.src = a.src; q.dst = a.dst; q.bounds = a.bounds; q.offsets = a.offsets; q.Wfwd = weights_fwd[i]; q.wsum = wsum[i];
    q.list = lists + list_begin;
    const int per_block = 256 * gigs::kCensusPerThread;
    census_blocks += (total + per_block - 1) / per_block;
    // windows no wider than a tile are scattered (see specular_scatter_body)
    q.narrow = a.avg_window <= gigs::kSpTile * gigs::kSpTile;
    q.nt = (a.res + gigs::kSpTile - 1) / gigs::kSpTile;
    q.parts = (q.cap + gigs::kSpSlice - 1) / gigs::kSpSlice;
    units += q.narrow ? (q.cap + 3) / 4 : 6 * q.nt * q.nt * q.parts;
    caps.cap[i] = q.cap;
    list_begin += (size_t)q.cap;
  }
  hipStream_t s = (hipStream_t)stream;
  gigs::StageTimer timer(gigs::Stage::kCubemapBwd, stream);
  hipLaunchKernelGGL(gigs::specular_census_kernel, dim3(census_blocks), dim3(256), 0, s, S, state);
  hipLaunchKernelGGL(gigs::specular_apply_multi_bwd_sparse_kernel, dim3(units + blocks), dim3(256), 0, s, L, S, units, state);
  hipLaunchKernelGGL(gigs::specular_sparse_finish_kernel, dim3(1), dim3(64), 0, s, caps, state);
  return gigs_internal_check_launch("specular_cubemap_multi_bwd_sparse");
}

int gigs_specular_cubemap_multi_fwd_sparse(gigs_ctx* ctx, int n_levels, const gigs_spec_level* levels, float* const* needed,
                                           const int* capacities, int* state, int* lists, void* stream) {
  const gigs::Options& o = *gigs_internal_options(ctx);
  if (n_levels <= 0 || n_levels > 8 || !levels || !needed || !capacities || !state || !lists)
    return gigs_internal_fail(GIGS_ERR_INVALID, "specular_cubemap_multi_fwd_sparse: bad argument");
  gigs::SpecLevels L;
  gigs::SparseLevels S;
  L.n = S.n = n_levels;
  int blocks = 0, census_blocks = 0, units = 0;
  gigs::SparseCaps caps = {};
  caps.n = n_levels;
  size_t list_begin = 0;
  for (int i = 0; i < n_levels; i++) {
    const gigs_spec_level& a = levels[i];
    if (a.res <= 0 || a.res > 4096 || !a.src || !a.bounds || !a.offsets || !a.weights || !a.dst || !a.wsum || !needed[i] ||
        capacities[i] < 0)
      return gigs_internal_fail(GIGS_ERR_INVALID, "specular_cubemap_multi_fwd_sparse: bad level");
    const int total = fill_spec_level(o, a, L.lv[i], blocks);
    gigs::SparseLevel& q = S.lv[i];
    memset(&q, 0, sizeof(q));
    // the listed body addresses a level's whole table with a 32-bit byte offset (avg_window is the floor of the mean)
    const bool addressable = ((long long)a.avg_window + 1) * total < (1ll << 29);
    q.total = total; q.cap = addressable ? (capacities[i] < total ? capacities[i] : total) : 0;
    q.block_begin = census_blocks; q.unit_begin = units; q.N = a.res;
    // the list census reads the marks and clears them for the next call: src = dst = needed
    q.vec = (((uintptr_t)needed[i]) & 15) == 0;
    q.src = needed[i]; q.dst = needed[i];
    q.list = lists + list_begin;
    const int per_block = 256 * gigs::kCensusPerThread;
    census_blocks += (total + per_block - 1) / per_block;
    const int per_wg = 4 * (64 / L.lv[i].lanes);  // listed texels per workgroup
    units += (q.cap + per_wg - 1) / per_wg;
    caps.cap[i] = q.cap;
    list_begin += (size_t)capacities[i];
  }
  hipStream_t s = (hipStream_t)stream;
  // no StageTimer, as for gigs_spec_tap_census: beside the march these launches take 7 times what they take alone
  hipLaunchKernelGGL(gigs::specular_census_kernel, dim3(census_blocks), dim3(256), 0, s, S, state);
  hipLaunchKernelGGL(gigs::specular_apply_multi_fwd_sparse_kernel, dim3(units + blocks), dim3(256), 0, s, L, S, units, state);
  hipLaunchKernelGGL(gigs::specular_sparse_finish_kernel, dim3(1), dim3(64), 0, s, caps, state);
  return gigs_internal_check_launch("specular_cubemap_multi_fwd_sparse");
}

}  // extern "C"
