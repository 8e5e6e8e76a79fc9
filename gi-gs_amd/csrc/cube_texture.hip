// cube_texture.hip -- cube maps as textures: the mip chain, lookups of a list of directions (forward, backward as
// scatter and as gather) and the conversion of a lat-long panorama to a cube.
//
// Reference behaviour restated:
//   cubemap_mip                          pbr/light.py:54-79
//   latlong_to_cubemap                   relight.py:92-111
// The lookups are nvdiffrast `dr.texture` calls in the reference (third party, unpinned -> parity unpinned); the
// sampling rule is cube.h's cube_taps, written down in include/gigs_hip.h and oracle/pbr_oracle.cpp.
#include <cmath>

#include "cube.h"

namespace gigs {

// cubemap_mip: forward 2x2 average, backward = bilinear cube lookup of 0.25 * dout
__global__ void __launch_bounds__(256)
cubemap_mip_fwd_kernel(int r, int C, const float* __restrict__ in, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 6 * r * r * C) return;
  const int c = i % C, x = (i / C) % r, y = (i / (C * r)) % r, f = i / (C * r * r);
  const int R2 = 2 * r;
  const float* p = in + ((size_t)(f * R2 + 2 * y) * R2 + 2 * x) * C + c;
  out[i] = (p[0] + p[C] + p[(size_t)R2 * C] + p[(size_t)R2 * C + C]) * 0.25f;
}

__global__ void __launch_bounds__(256)
cubemap_mip_bwd_kernel(int r, const float* __restrict__ dout, float* __restrict__ din, const float* __restrict__ add,
                       const float* __restrict__ dout2) {
  const int res = 2 * r;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= 6 * res * res) return;
  const int x = i % res, y = (i / res) % res, s = i / (res * res);
  const float start = -1.0f + 1.0f / (float)res, end = 1.0f - 1.0f / (float)res;
  const float stepv = (end - start) / (float)(res - 1);
  const float gx = x < res / 2 ? start + stepv * (float)x : end - stepv * (float)(res - 1 - x);
  const float gy = y < res / 2 ? start + stepv * (float)y : end - stepv * (float)(res - 1 - y);
  v3 d = cube_dir_raw(gx, gy, s);
  const float n = fmaxf(sqrtf(d.x * d.x + d.y * d.y + d.z * d.z), 1e-12f);
  d = {d.x / n, d.y / n, d.z / n};
  Taps t;
  v3 v = {0, 0, 0};
  if (cube_taps(r, d.x, d.y, d.z, t)) {
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (t.idx[k] >= 0) {
        const float* p = dout + 3 * (size_t)t.idx[k];
        float p0 = p[0], p1 = p[1], p2 = p[2];
        if (dout2) {  // a second gradient of the coarse level (it fed two filters): the sum autograd would have formed first
          const float* q = dout2 + 3 * (size_t)t.idx[k];
          p0 += q[0]; p1 += q[1]; p2 += q[2];
        }
        v.x += (p0 * 0.25f) * t.w[k];
        v.y += (p1 * 0.25f) * t.w[k];
        v.z += (p2 * 0.25f) * t.w[k];
      }
  }
  if (add) {  // the level's own gradient (it also feeds a filter): summed here instead of by a separate pass
    v.x += add[3 * (size_t)i]; v.y += add[3 * (size_t)i + 1]; v.z += add[3 * (size_t)i + 2];
  }
  din[3 * (size_t)i] = v.x; din[3 * (size_t)i + 1] = v.y; din[3 * (size_t)i + 2] = v.z;
}

// dr.texture(cubemap[None], dirs[None], filter_mode="linear", boundary_mode="cube") for a list of directions
// (train.py:409-417 envmap TV, render.py:80 / relight.py:108 envmap export): out is [n,3], or [3,n] planes if planar.
__global__ void __launch_bounds__(256)
cube_texture_fwd_kernel(int res, const float* __restrict__ tex, int n, const float* __restrict__ dirs,
                        float* __restrict__ out, int planar) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Taps t;
  v3 v = {0, 0, 0};
  if (cube_taps(res, dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2], t)) v = cube_sample(tex, t);
  if (planar) {
    out[i] = v.x; out[(size_t)n + i] = v.y; out[2 * (size_t)n + i] = v.z;
  } else {
    out[3 * (size_t)i] = v.x; out[3 * (size_t)i + 1] = v.y; out[3 * (size_t)i + 2] = v.z;
  }
}

// The same lookup with double-precision texel coordinates (cube_taps_precise): out is [n,3].
__global__ void __launch_bounds__(256)
cube_texture_fwd_precise_kernel(int res, const float* __restrict__ tex, int n, const float* __restrict__ dirs,
                                float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Taps t;
  v3 v = {0, 0, 0};
  if (cube_taps_precise(res, dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2], t)) v = cube_sample(tex, t);
  out[3 * (size_t)i] = v.x; out[3 * (size_t)i + 1] = v.y; out[3 * (size_t)i + 2] = v.z;
}

// latlong_to_cubemap (relight.py:92-111): every cube texel looks its direction up in an equirectangular map.
//   gy, gx = linspace(-1 + 1/res, 1 - 1/res, res)   (torch: start + i*step below the middle, end - (n-1-i)*step above)
//   v = normalize(cube_to_dir(face, gx, gy));  tu = atan2(v.x, -v.z) / (2 pi) + 0.5;  tv = acos(clamp(v.y, -1, 1)) / pi
//   out = dr.texture(latlong[None], (tu, tv), filter_mode="linear")   -- nvdiffrast, third party and absent: restated
//   from its documented behaviour (bilinear, texel centres at (i + 0.5)/size, boundary_mode "wrap"): PARITY UNPINNED.
__global__ void __launch_bounds__(256)
latlong_to_cubemap_kernel(int res_y, int res_x, int Hl, int Wl, int C, const float* __restrict__ latlong,
                          float* __restrict__ cube) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int n = 6 * res_y * res_x;
  if (i >= n) return;
  const int face = i / (res_y * res_x), rem = i - face * res_y * res_x;
  const int ty = rem / res_x, tx = rem - ty * res_x;
  const float gy = torch_linspace(-1.0f + 1.0f / (float)res_y, 1.0f - 1.0f / (float)res_y, res_y, ty);
  const float gx = torch_linspace(-1.0f + 1.0f / (float)res_x, 1.0f - 1.0f / (float)res_x, res_x, tx);
  float rx, ry, rz;  // cube_to_dir (relight.py:75-89)
  switch (face) {
    case 0: rx = 1.0f; ry = -gy; rz = -gx; break;
    case 1: rx = -1.0f; ry = -gy; rz = gx; break;
    case 2: rx = gx; ry = 1.0f; rz = gy; break;
    case 3: rx = gx; ry = -1.0f; rz = -gy; break;
    case 4: rx = gx; ry = -gy; rz = 1.0f; break;
    default: rx = -gx; ry = -gy; rz = -1.0f; break;
  }
  const float inv = 1.0f / fmaxf(sqrtf(rx * rx + ry * ry + rz * rz), 1e-12f);  // F.normalize
  rx *= inv; ry *= inv; rz *= inv;
  const float kPi = 3.14159265358979323846f;
  const float tu = atan2f(rx, -rz) / (2.0f * kPi) + 0.5f;
  const float tv = acosf(fminf(fmaxf(ry, -1.0f), 1.0f)) / kPi;
  const float u = tu * (float)Wl - 0.5f, v = tv * (float)Hl - 0.5f;
  const float fu0 = floorf(u), fv0 = floorf(v);
  const float fu = u - fu0, fv = v - fv0;
  auto wrap = [](int a, int m) { a %= m; return a < 0 ? a + m : a; };
  const int iu0 = wrap((int)fu0, Wl), iu1 = wrap((int)fu0 + 1, Wl);
  const int iv0 = wrap((int)fv0, Hl), iv1 = wrap((int)fv0 + 1, Hl);
  for (int c = 0; c < C; c++) {
    const float a = latlong[((size_t)iv0 * Wl + iu0) * C + c] * (1.0f - fu) + latlong[((size_t)iv0 * Wl + iu1) * C + c] * fu;
    const float b = latlong[((size_t)iv1 * Wl + iu0) * C + c] * (1.0f - fu) + latlong[((size_t)iv1 * Wl + iu1) * C + c] * fu;
    cube[(size_t)i * C + c] = a * (1.0f - fv) + b * fv;
  }
}

// The same conversion under n_rot rotations of the environment (gigs_latlong_to_cubemap_rot; blockIdx.y = rotation):
// env_R(d) = env(R^T d), so the texel's normalised direction is replaced by R^T dir before the lookup and everything else is
// latlong_to_cubemap_kernel's expression for expression (kept as two bodies: a shared templated body compiles to other
// code for both kernels, see profiles/r24/pbr_split_device_code.txt).  The matrix is wave-uniform; one that is exactly the identity
// skips the product (x * 1 + y * 0 + z * 0 is not x for a non-finite or negative-zero component), which makes that slice the
// unrotated kernel's bit for bit.
__global__ void __launch_bounds__(256)
latlong_to_cubemap_rot_kernel(int res_y, int res_x, int Hl, int Wl, int C, const float* __restrict__ latlong,
                              const float* __restrict__ rotations, float* __restrict__ cube) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int n = 6 * res_y * res_x;
  if (i >= n) return;
  const float* R = rotations + 9 * (size_t)blockIdx.y;
  const float r00 = R[0], r01 = R[1], r02 = R[2], r10 = R[3], r11 = R[4], r12 = R[5], r20 = R[6], r21 = R[7], r22 = R[8];
  const bool identity = r00 == 1.0f && r11 == 1.0f && r22 == 1.0f && r01 == 0.0f && r02 == 0.0f && r10 == 0.0f &&
                        r12 == 0.0f && r20 == 0.0f && r21 == 0.0f;
  const int face = i / (res_y * res_x), rem = i - face * res_y * res_x;
  const int ty = rem / res_x, tx = rem - ty * res_x;
  const float gy = torch_linspace(-1.0f + 1.0f / (float)res_y, 1.0f - 1.0f / (float)res_y, res_y, ty);
  const float gx = torch_linspace(-1.0f + 1.0f / (float)res_x, 1.0f - 1.0f / (float)res_x, res_x, tx);
  float rx, ry, rz;  // cube_to_dir (relight.py:75-89)
  switch (face) {
    case 0: rx = 1.0f; ry = -gy; rz = -gx; break;
    case 1: rx = -1.0f; ry = -gy; rz = gx; break;
    case 2: rx = gx; ry = 1.0f; rz = gy; break;
    case 3: rx = gx; ry = -1.0f; rz = -gy; break;
    case 4: rx = gx; ry = -gy; rz = 1.0f; break;
    default: rx = -gx; ry = -gy; rz = -1.0f; break;
  }
  const float inv = 1.0f / fmaxf(sqrtf(rx * rx + ry * ry + rz * rz), 1e-12f);  // F.normalize
  rx *= inv; ry *= inv; rz *= inv;
  if (!identity) {  // R^T dir: column j of R against dir, x then y then z
    const float qx = (r00 * rx + r10 * ry) + r20 * rz;
    const float qy = (r01 * rx + r11 * ry) + r21 * rz;
    const float qz = (r02 * rx + r12 * ry) + r22 * rz;
    rx = qx; ry = qy; rz = qz;
  }
  const float kPi = 3.14159265358979323846f;
  const float tu = atan2f(rx, -rz) / (2.0f * kPi) + 0.5f;
  const float tv = acosf(fminf(fmaxf(ry, -1.0f), 1.0f)) / kPi;
  const float u = tu * (float)Wl - 0.5f, v = tv * (float)Hl - 0.5f;
  const float fu0 = floorf(u), fv0 = floorf(v);
  const float fu = u - fu0, fv = v - fv0;
  auto wrap = [](int a, int m) { a %= m; return a < 0 ? a + m : a; };
  const int iu0 = wrap((int)fu0, Wl), iu1 = wrap((int)fu0 + 1, Wl);
  const int iv0 = wrap((int)fv0, Hl), iv1 = wrap((int)fv0 + 1, Hl);
  float* out = cube + ((size_t)blockIdx.y * n + i) * C;
  for (int c = 0; c < C; c++) {
    const float a = latlong[((size_t)iv0 * Wl + iu0) * C + c] * (1.0f - fu) + latlong[((size_t)iv0 * Wl + iu1) * C + c] * fu;
    const float b = latlong[((size_t)iv1 * Wl + iu0) * C + c] * (1.0f - fu) + latlong[((size_t)iv1 * Wl + iu1) * C + c] * fu;
    out[c] = a * (1.0f - fv) + b * fv;
  }
}

// scatters g_out through the same taps; accumulates into d_tex (caller zeroes).  Neighbouring samples that hit the same
// texel are pre-summed per 16-lane row (run_add3): the envmap TV's latlong grid (losses.get_envmap_dirs) sends whole rows
// of 512 samples to the four texels around a pole, which serialised 0.32 ms of memory-side atomics.
__global__ void __launch_bounds__(256)
cube_texture_bwd_kernel(int res, int n, const float* __restrict__ dirs, const float* __restrict__ g_out,
                        float* __restrict__ d_tex, int planar) {
  const int gi = blockIdx.x * 256 + threadIdx.x;
  const bool live = gi < n;
  const int i = live ? gi : 0;  // dead lanes add nothing: the DPP scans need every lane
  Taps t;
  const bool ok = cube_taps(res, dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2], t) && live;
  const float g0 = planar ? g_out[i] : g_out[3 * (size_t)i];
  const float g1 = planar ? g_out[(size_t)n + i] : g_out[3 * (size_t)i + 1];
  const float g2 = planar ? g_out[2 * (size_t)n + i] : g_out[3 * (size_t)i + 2];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int idx = (ok && t.idx[k] >= 0 && t.w[k] != 0.0f) ? t.idx[k] : -1;
    const float w = idx >= 0 ? t.w[k] : 0.0f;
    run_add3<false>(d_tex + 3 * (size_t)max(idx, 0), idx, g0 * w, g1 * w, g2 * w);
  }
}

// The same backward as a gather, for direction sets that do not change (the envmap TV's latlong grid): the taps of every
// sample are exported once (cube_taps_export_kernel), the host sorts them by texel into a CSR list (pbr/texture.py), and
// each texel then sums its own entries in sample order -- no atomics (6.3 M of them bound the scatter at 0.11 ms for the
// 512 x 1024 grid), no zero-fill, reproducible.  Texels with more than `heavy` entries (the poles) get a wave each.
__global__ void __launch_bounds__(256)
cube_taps_export_kernel(int res, int n, const float* __restrict__ dirs, int* __restrict__ idx, float* __restrict__ w) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  Taps t;
  const bool ok = cube_taps(res, dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2], t);
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const bool use = ok && t.idx[k] >= 0 && t.w[k] != 0.0f;
    idx[4 * (size_t)i + k] = use ? t.idx[k] : -1;
    w[4 * (size_t)i + k] = use ? t.w[k] : 0.0f;
  }
}

__global__ void __launch_bounds__(256)
cube_texture_bwd_gather_kernel(int n_tex, const int* __restrict__ offsets, const int* __restrict__ ent_sample,
                               const float* __restrict__ ent_w, const float* __restrict__ g_out, int n, int planar,
                               float* __restrict__ d_tex, int heavy, int light_blocks, const int* __restrict__ heavy_ids,
                               int n_heavy) {
  auto grad = [&](int s, float& a, float& b, float& c) {
    if (planar) { a = g_out[s]; b = g_out[(size_t)n + s]; c = g_out[2 * (size_t)n + s]; }
    else { a = g_out[3 * (size_t)s]; b = g_out[3 * (size_t)s + 1]; c = g_out[3 * (size_t)s + 2]; }
  };
  if ((int)blockIdx.x < light_blocks) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n_tex) return;
    const int b = offsets[t], e = offsets[t + 1];
    if (e - b > heavy) return;  // summed by a wave below
    float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
    for (int k = b; k < e; k++) {
      float g0, g1, g2;
      grad(ent_sample[k], g0, g1, g2);
      const float w = ent_w[k];
      c0 += g0 * w; c1 += g1 * w; c2 += g2 * w;
    }
    d_tex[3 * (size_t)t] = c0; d_tex[3 * (size_t)t + 1] = c1; d_tex[3 * (size_t)t + 2] = c2;
    return;
  }
  const int h = ((int)blockIdx.x - light_blocks) * 4 + (threadIdx.x >> 6);
  if (h >= n_heavy) return;  // wave-uniform
  const int lane = threadIdx.x & 63;
  const int t = heavy_ids[h];
  const int b = offsets[t], e = offsets[t + 1];
  float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f;
  for (int k = b + lane; k < e; k += 64) {
    float g0, g1, g2;
    grad(ent_sample[k], g0, g1, g2);
    const float w = ent_w[k];
    c0 += g0 * w; c1 += g1 * w; c2 += g2 * w;
  }
  c0 = wave_sum63(c0); c1 = wave_sum63(c1); c2 = wave_sum63(c2);
  if (lane == 63) { d_tex[3 * (size_t)t] = c0; d_tex[3 * (size_t)t + 1] = c1; d_tex[3 * (size_t)t + 2] = c2; }
}

}  // namespace gigs

// ------------------------------------------------------------------------------------------
// C ABI (declared in include/gigs_hip.h)
// ------------------------------------------------------------------------------------------
#include "gigs_internal.h"

extern "C" {

int gigs_cubemap_mip_fwd(int res_out, int channels, const float* in, float* out, void* stream) {
  if (res_out <= 0 || channels <= 0 || !in || !out) return gigs_internal_fail(GIGS_ERR_INVALID, "cubemap_mip_fwd: bad argument");
  gigs::StageTimer timer(gigs::Stage::kCubemapFwd, stream);
  hipLaunchKernelGGL(gigs::cubemap_mip_fwd_kernel, dim3((6 * res_out * res_out * channels + 255) / 256), dim3(256), 0, (hipStream_t)stream, res_out, channels, in, out);
  return gigs_internal_check_launch("cubemap_mip_fwd");
}

// din = 2x2 box backward of dout (+ dout2) (+ add): the three entry points differ in which addends they pass
static int cubemap_mip_bwd(const char* entry, int res_out, const float* dout, const float* dout2, const float* add, float* din,
                           void* stream) {
  const int res = 2 * res_out;
  gigs::StageTimer timer(gigs::Stage::kCubemapBwd, stream);
  hipLaunchKernelGGL(gigs::cubemap_mip_bwd_kernel, dim3((6 * res * res + 255) / 256), dim3(256), 0, (hipStream_t)stream, res_out, dout, din, add,
                     dout2);
  return gigs_internal_check_launch(entry);
}

int gigs_cubemap_mip_bwd(int res_out, const float* dout, float* din, void* stream) {
  if (res_out <= 0 || !dout || !din) return gigs_internal_fail(GIGS_ERR_INVALID, "cubemap_mip_bwd: bad argument");
  return cubemap_mip_bwd("cubemap_mip_bwd", res_out, dout, nullptr, nullptr, din, stream);
}

int gigs_cubemap_mip_bwd_add(int res_out, const float* dout, const float* add, float* din, void* stream) {
  if (res_out <= 0 || !dout || !add || !din) return gigs_internal_fail(GIGS_ERR_INVALID, "cubemap_mip_bwd_add: bad argument");
  return cubemap_mip_bwd("cubemap_mip_bwd_add", res_out, dout, nullptr, add, din, stream);
}

int gigs_cubemap_mip_bwd_add2(int res_out, const float* dout, const float* dout2, const float* add, float* din, void* stream) {
  if (res_out <= 0 || !dout || !din) return gigs_internal_fail(GIGS_ERR_INVALID, "cubemap_mip_bwd_add2: bad argument");
  return cubemap_mip_bwd("cubemap_mip_bwd_add2", res_out, dout, dout2, add, din, stream);
}

int gigs_cube_texture_fwd(int res, const float* cubemap, int n, const float* dirs, float* out, int planar,
                          void* stream) {
  if (res <= 0 || n < 0 || !cubemap || (n > 0 && (!dirs || !out)))
    return gigs_internal_fail(GIGS_ERR_INVALID, "cube_texture_fwd: bad argument");
  if (n == 0) return 0;
  gigs::StageTimer timer(gigs::Stage::kCubemapFwd, stream);
  hipLaunchKernelGGL(gigs::cube_texture_fwd_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, res,
                     cubemap, n, dirs, out, planar);
  return gigs_internal_check_launch("cube_texture_fwd");
}

int gigs_cube_texture_fwd_precise(int res, const float* cubemap, int n, const float* dirs, float* out, void* stream) {
  if (res <= 0 || n < 0 || !cubemap || (n > 0 && (!dirs || !out)))
    return gigs_internal_fail(GIGS_ERR_INVALID, "cube_texture_fwd_precise: bad argument");
  if (n == 0) return 0;
  gigs::StageTimer timer(gigs::Stage::kCubemapFwd, stream);
  hipLaunchKernelGGL(gigs::cube_texture_fwd_precise_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, res,
                     cubemap, n, dirs, out);
  return gigs_internal_check_launch("cube_texture_fwd_precise");
}

int gigs_latlong_to_cubemap(int res_y, int res_x, int lat_h, int lat_w, int channels, const float* latlong, float* cubemap,
                            void* stream) {
  if (res_y <= 0 || res_x <= 0 || lat_h <= 0 || lat_w <= 0 || channels <= 0 || !latlong || !cubemap)
    return gigs_internal_fail(GIGS_ERR_INVALID, "latlong_to_cubemap: bad argument");
  const int n = 6 * res_y * res_x;
  gigs::StageTimer timer(gigs::Stage::kCubemapFwd, stream);
  hipLaunchKernelGGL(gigs::latlong_to_cubemap_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, res_y, res_x,
                     lat_h, lat_w, channels, latlong, cubemap);
  return gigs_internal_check_launch("latlong_to_cubemap");
}

int gigs_latlong_to_cubemap_rot(int res_y, int res_x, int lat_h, int lat_w, int channels, const float* latlong, int n_rot,
                                const float* rotations, float* cubemap, void* stream) {
  if (n_rot < 1 || n_rot > 1024)
    return gigs_internal_fail(GIGS_ERR_INVALID, "latlong_to_cubemap_rot: n_rot outside 1..1024");
  if (res_y <= 0 || res_x <= 0 || lat_h <= 0 || lat_w <= 0 || channels <= 0 || !latlong || !rotations || !cubemap)
    return gigs_internal_fail(GIGS_ERR_INVALID, "latlong_to_cubemap_rot: bad argument");
  const int n = 6 * res_y * res_x;
  gigs::StageTimer timer(gigs::Stage::kCubemapFwd, stream);
  hipLaunchKernelGGL(gigs::latlong_to_cubemap_rot_kernel, dim3((n + 255) / 256, n_rot), dim3(256), 0, (hipStream_t)stream,
                     res_y, res_x, lat_h, lat_w, channels, latlong, rotations, cubemap);
  return gigs_internal_check_launch("latlong_to_cubemap_rot");
}

int gigs_cube_texture_bwd(int res, int n, const float* dirs, const float* g_out, float* d_cubemap, int planar,
                          void* stream) {
  if (res <= 0 || n < 0 || !d_cubemap || (n > 0 && (!dirs || !g_out)))
    return gigs_internal_fail(GIGS_ERR_INVALID, "cube_texture_bwd: bad argument");
  if (n == 0) return 0;
  gigs::StageTimer timer(gigs::Stage::kCubemapBwd, stream);
  hipLaunchKernelGGL(gigs::cube_texture_bwd_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, res, n,
                     dirs, g_out, d_cubemap, planar);
  return gigs_internal_check_launch("cube_texture_bwd");
}

int gigs_cube_taps(int res, int n, const float* dirs, int* idx, float* w, void* stream) {
  if (res <= 0 || n < 0 || (n > 0 && (!dirs || !idx || !w))) return gigs_internal_fail(GIGS_ERR_INVALID, "cube_taps: bad argument");
  if (n == 0) return 0;
  hipLaunchKernelGGL(gigs::cube_taps_export_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, res, n, dirs, idx, w);
  return gigs_internal_check_launch("cube_taps");
}

int gigs_cube_texture_bwd_gather(int res, int n, int planar, const int* offsets, const int* ent_sample, const float* ent_w,
                                 int heavy, int n_heavy, const int* heavy_ids, const float* g_out, float* d_cubemap,
                                 void* stream) {
  if (res <= 0 || n <= 0 || !offsets || !ent_sample || !ent_w || !g_out || !d_cubemap || heavy < 0 || n_heavy < 0 ||
      (n_heavy > 0 && !heavy_ids))
    return gigs_internal_fail(GIGS_ERR_INVALID, "cube_texture_bwd_gather: bad argument");
  const int n_tex = 6 * res * res;
  const int light_blocks = (n_tex + 255) / 256, heavy_blocks = (n_heavy + 3) / 4;
  gigs::StageTimer timer(gigs::Stage::kCubemapBwd, stream);
  hipLaunchKernelGGL(gigs::cube_texture_bwd_gather_kernel, dim3(light_blocks + heavy_blocks), dim3(256), 0, (hipStream_t)stream,
                     n_tex, offsets, ent_sample, ent_w, g_out, n, planar, d_cubemap, heavy, light_blocks, heavy_ids, n_heavy);
  return gigs_internal_check_launch("cube_texture_bwd_gather");
}

}  // extern "C"
