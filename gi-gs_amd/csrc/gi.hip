// gi.hip -- the screen-space marches over the G-buffer: SSAO and SSR (indirect diffuse), their ray table and their
// certification table.  The per-lane arithmetic of a march is gi_march.h; the gather over a recorded hit list is
// ssr_apply.hip; depth->normal and the 3x3 filters the operator applies around them are normal_filters.hip.
//
// Reference behaviour restated (R/ = submodules/diff-gaussian-rasterization):
//   SSAOCUDA              R/cuda_rasterizer/forward.cu:635-724    (get_coord   ssr.h:120-135)
//   SSRCUDA               forward.cu:726-909                      (fresnelSchlick ssr.h:13-16)
//
// MI355X design for SSAO / SSR (the dominant cost at start < step: rays * steps dependent
// gathers per pixel):
//   * the (phi, theta) ray set is pixel-invariant.  The host builds it ONCE per `delta` with
//     the reference's fp32 loop accumulation (`phi += d*pi`, `theta += d*pi/2`) and libm
//     sinf/cosf, and keeps it in a small per-device table.  In the kernel the ray index is
//     wave-uniform, so the table is read with scalar loads (s_load_dwordx4/x8) into SGPRs
//     and costs no vector memory or LDS traffic; the loop-count subtleties (16 not 17 theta
//     samples at delta = 0.0625) are decided on the host exactly as the oracle decides them;
//   * 8x8 pixels per wave so the z-plane gathers of neighbouring lanes share cache lines (the
//     z plane is 2.5 MB at 800x800 and stays L2 resident).
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <type_traits>
#include <vector>

#include "gi_march.h"
#include "gigs_internal.h"

namespace gigs {

// ------------------------------------------------------------------------------------------
// Ray table: per ray two float4 -- {ts.x, ts.y, ts.z, cos(theta)}, {sin(theta), w, 0, 0}
// with ts = normalize(sin t cos p, sin t sin p, cos t) and w = cos t * sin t.
//
// Zero-weight rays.  The reference's theta loop starts at 0 (forward.cu:681, 797): sin(0) = 0, so for every azimuth
// the first ray is the SAME direction (0, 0, 1) -- the pixel's normal -- with weight w = cos * sin = 0.  SSAO adds
// `w` for a hit (forward.cu:711: occ += 0, a no-op) and `w` to the sample sum (:690, again + 0); SSR adds
// rgb * cos * sin = +-0, or NaN when the hit pixel's rgb is not finite (forward.cu:824-826), identically for all of
// them.  So the table holds the rays with w != 0 first, in the reference's loop order (`n_live`), and the zero-weight
// ones behind them (`n_dead`; 32 of 512 at delta = 0.0625): SSAO marches the live ones only, SSR the live ones plus ONE
// of the dead ones (its +-0 / NaN applied once is the same as applied 32 times: x + 0 = x, NaN is sticky); the
// sample counts (SSAO's sum of weights, SSR's nrSamples = all rays) are unchanged.  gigs_options.gi_zero_rays = 1
// marches every dead ray as well, after the live ones -- same partial sums, same bits (tested): the proof that the
// cut is exact.  The dead rays are recognised by value (sin = 0 and ts.xy = 0, all with the same ts.z / cos), not by
// index; if a delta ever produced zero-weight rays of different directions they would simply count as live.
// The cache is keyed by (device, delta) and an entry is never modified once built, so concurrent streams and
// contexts share it safely.  RayTable is declared in gigs_internal.h: ssr_apply.hip reads the table through
// get_ray_table too, and this unit stays the only owner of the cache.
// ------------------------------------------------------------------------------------------
static std::mutex g_ray_mu;
static std::vector<RayTable> g_ray;  // immutable entries

int get_ray_table(float delta, hipStream_t s, RayTable& out) {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0) return -2;
  std::lock_guard<std::mutex> lk(g_ray_mu);
  for (const RayTable& t : g_ray)
    if (t.device == dev && t.delta == delta) { out = t; return 0; }
  if (!(delta > 1e-4f)) return -1;  // would not terminate / absurd table
  std::vector<float4> h;
  const float sampleDelta = delta * kPiF;
  float sum_w = 0.0f;
  for (float phi = 0.0f; (double)phi < 2.0 * (double)kPiF; phi += sampleDelta) {
    for (float theta = 0.0f; (double)theta <= 0.5 * (double)kPiF;
         theta = (float)((double)theta + (double)sampleDelta * 0.5)) {
      const float ct = cosf(theta), st = sinf(theta);
      float tx = st * cosf(phi), ty = st * sinf(phi), tz = ct;
      const float inv = 1.0f / sqrtf(tx * tx + ty * ty + tz * tz);
      tx *= inv; ty *= inv; tz *= inv;
      const float w = ct * st;
      sum_w += w;
      h.push_back(make_float4(tx, ty, tz, ct));
      h.push_back(make_float4(st, w, 0.0f, 0.0f));
      if (h.size() > (1u << 21)) return -1;
    }
  }
  // live rays first, the (identical) zero-weight rays behind them
  const size_t n = h.size() / 2;
  std::vector<size_t> dead;
  for (size_t r = 0; r < n; r++) {
    const float4 a = h[2 * r], b = h[2 * r + 1];
    if (b.x == 0.0f && b.y == 0.0f && a.x == 0.0f && a.y == 0.0f) dead.push_back(r);
  }
  for (size_t k = 1; k < dead.size(); k++)
    if (h[2 * dead[k]].z != h[2 * dead[0]].z || h[2 * dead[k]].w != h[2 * dead[0]].w) { dead.clear(); break; }
  std::vector<float4> ordered;
  ordered.reserve(h.size());
  {
    size_t k = 0;
    for (size_t r = 0; r < n; r++) {
      if (k < dead.size() && dead[k] == r) { k++; continue; }
      ordered.push_back(h[2 * r]); ordered.push_back(h[2 * r + 1]);
    }
    for (size_t r : dead) { ordered.push_back(h[2 * r]); ordered.push_back(h[2 * r + 1]); }
  }
  RayTable t;
  const size_t bytes = ordered.size() * sizeof(float4);
  // one-time (per device and delta) internal allocation; never freed, never rewritten
  if (hipMalloc(&t.dev, bytes ? bytes : 16) != hipSuccess) return -2;
  if (bytes) {
    // a blocking copy: the entry is complete before any stream can read it.  (First use of a delta on a device must
    // therefore happen outside a hipGraph capture -- every capture in this package is preceded by an eager warm-up.)
    if (hipMemcpy(t.dev, ordered.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return -2;
  }
  (void)s;
  t.device = dev;
  t.delta = delta;
  t.nrays = (int)n;
  t.n_dead = (int)dead.size();
  t.n_live = (int)(n - dead.size());
  t.sum_w = sum_w;
  g_ray.push_back(t);
  out = t;
  return 0;
}

#ifndef GIGS_GI_GROUP
#define GIGS_GI_GROUP 4
#endif
#ifndef GIGS_GI_RAYS
#define GIGS_GI_RAYS 2
#endif
constexpr int kGiGroup = GIGS_GI_GROUP;  // steps whose gathers are issued together
constexpr int kGiRays = GIGS_GI_RAYS;    // rays marched together per lane (independent instruction streams)
constexpr int kGiWaves = 4;
constexpr int kGiTileLog2W = 3;

// One 256-lane workgroup per 8x8 pixel tile: the four waves cover the SAME 64 pixels and split the
// ray set into four contiguous chunks (25 000 x 4 waves at 800x800 instead of 10 000 long-running
// ones: the tail of the launch is short and empty tiles retire immediately).  Partial sums are
// combined through LDS in the fixed order ((w0 + w1) + w2) + w3.
// `tid` is threadIdx.x (a parameter: the SSR kernel derives its pixel a second time behind the march, see there)
__device__ __forceinline__ bool gi_pixel(const GiParams& p, unsigned tid, int& x, int& y, int& wave) {
  const int lane = tid & 63;
  wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // provably uniform: the ray table is then read with s_load
  x = (blockIdx.x << p.tile_log2w) + (lane & ((1 << p.tile_log2w) - 1));
  y = blockIdx.y * (64 >> p.tile_log2w) + (lane >> p.tile_log2w);
  return x < p.W && y < p.H;
}
__device__ __forceinline__ bool gi_pixel(const GiParams& p, int& x, int& y, int& wave) {
  return gi_pixel(p, threadIdx.x, x, y, wave);
}

#ifndef GIGS_GI_WAVES
#define GIGS_GI_WAVES 0
#endif
#if GIGS_GI_WAVES > 0
#define GIGS_GI_OCC __attribute__((amdgpu_waves_per_eu(GIGS_GI_WAVES, GIGS_GI_WAVES)))
#define GIGS_SSR_OCC GIGS_GI_OCC
#else
#define GIGS_GI_OCC
// The single-light SSR march asks for GIGS_SSR_WAVES waves per SIMD.  On its own the certified march allocated 100 VGPRs
// (4 waves); asked for 5 it fitted 96 and ran 9 % faster (1.29 -> 1.17 ms at C2), and 6 spilled in the march and lost it
// again -- as long as the finish's position and tangent frame (12 VGPRs), the planes' offsets (6) and the in-image mask
// and wave index (3 SGPRs, which at the scalar limit cost a VGPR for their lanes) lived across the march.  They no
// longer do (see ssr_kernel): at 6 waves the default instance takes 80 VGPRs, the exact marches 79, none with scratch;
// only the hit-list fill (kHits 2) keeps two register pairs of the per-pixel frame in scratch (20 B), reloaded once per
// ray pair, outside the per-group loop (DESIGN.md section 5 and profiles/r29/gi_resource_usage.txt have the listing).
// LDS allows 6: at 800^2 a workgroup holds 3 072 B static + 21 632 B of table = 24 704 B, six of them 148 224 B of the
// CU's 163 840 (a seventh does not fit; SSAO's 1 024 + 21 632 = 22 656 B would, 158 592 B).
#ifndef GIGS_SSR_WAVES
#define GIGS_SSR_WAVES 6
#endif
#define GIGS_SSR_OCC __attribute__((amdgpu_waves_per_eu(GIGS_SSR_WAVES)))
#endif
// The march over K radiance planes (kLights > 1, gigs_ssr_multi) holds 3 (K - 1) more accumulators: they do not fit the
// single-light budget, so those instances ask for GIGS_SSR_MULTI_WAVES ("Relighting under K maps").
#ifndef GIGS_SSR_MULTI_WAVES
#define GIGS_SSR_MULTI_WAVES 4
#endif
#if GIGS_GI_WAVES > 0
#define GIGS_SSR_OCC_L(L) GIGS_SSR_OCC
#else
#define GIGS_SSR_OCC_L(L) __attribute__((amdgpu_waves_per_eu((L) == 1 ? GIGS_SSR_WAVES : GIGS_SSR_MULTI_WAVES)))
#endif

// What a kernel instance marches with (gi_dispatch_march picks it).  The exact march has a cheaper form for a power-of-two
// step; certification exists in front of the projective march only.
enum class March { kExactPow2, kExact, kProj, kProjCert };
constexpr bool march_is_proj(March m) { return m == March::kProj || m == March::kProjCert; }

// The certification table of a kProjCert instance, staged into its dynamic LDS: march2_cert addresses the table by the
// constant kCertOff, so the dynamic LDS has to start right behind the kernel's static array of that size.
template <int kCertOff>
__device__ __forceinline__ void stage_cert_table(const GiParams& p, const float2* __restrict__ cert_tab) {
  extern __shared__ float2 s_cert[];
  if ((unsigned)(size_t)s_cert != (unsigned)kCertOff) __builtin_trap();
  const int nb = (p.cert_w + 1) * (p.cert_h + 1);
  for (int i = threadIdx.x; i < nb; i += 256) s_cert[i] = cert_tab[i];
  __syncthreads();
}
// Does any pixel of the workgroup march?  `marches` must be a function of the lane's PIXEL and the launch parameters alone
// (inside the image, start < step, a frame that can hit, magnitudes the march accepts) -- never of the wave or its share of
// the rays: the four waves of a workgroup hold the same 64 pixels in the same lanes (gi_pixel), so each of them takes the
// same vote, and a workgroup either stages the table -- barrier included -- with all four waves or with none.  A workgroup
// that marches nothing (background tiles, start >= step) goes straight to its tail.
__device__ __forceinline__ bool gi_any_lane_marches(bool marches) { return __builtin_amdgcn_ballot_w64(marches) != 0ull; }
// A pointer the compiler cannot relate to the one it was made from: loads through it are not merged with, nor kept alive
// from, earlier loads of the same address.
template <class T>
__device__ __forceinline__ const T* launder_ptr(const T* q) {
  asm volatile("" : "+s"(q));
  return q;
}

// ssao_kernel and ssr_kernel each state the per-pixel preamble and the two ray drivers (projective: pairs; exact: groups,
// singles, tail) and differ only in what they do with a hit.  They are kept in step by hand: one shared driver compiled
// to different code for every instance in every form tried (profiles/r25/gi_split_device_code.txt).
template <March kMarch>
__global__ void __launch_bounds__(256) GIGS_GI_OCC
ssao_kernel(GiParams p, const float4* __restrict__ rays, float sum_w,
            const float* __restrict__ nrm, const float* __restrict__ pos_map,
            float* __restrict__ occlusion, const float2* __restrict__ cert_tab) {
  __shared__ float s_part[kGiWaves][64];
  constexpr bool kPow2 = kMarch == March::kExactPow2, kCert = kMarch == March::kProjCert;
  constexpr int kCertOff = sizeof(float) * kGiWaves * 64;  // dynamic LDS follows the static array
  int x, y, wave;
  const bool inside = gi_pixel(p, x, y, wave);
  const int lane = threadIdx.x & 63;
  const unsigned HW = (unsigned)(p.H * p.W), pix_id = inside ? (unsigned)(p.W * y + x) : 0u;  // W, H < 2^15: 3 HW < 2^32
  float occ = 0.0f;
  // the pixel's frame and position are read in front of the table's staging: what they decide -- does this lane march --
  // decides whether the workgroup needs the table at all
  Tbn tbn = {};
  v3 pos = {};
  float a = 0.0f;
  bool mag_ok = false, marches = false;
  if (inside && p.start < p.step) {
    tbn = make_tbn({nrm[pix_id], nrm[HW + pix_id], nrm[2 * HW + pix_id]});
    if (!tbn_never_hits(tbn)) {
      pos = {pos_map[pix_id], pos_map[HW + pix_id], pos_map[2 * HW + pix_id]};
      a = 1 + pos.z / 100;
      mag_ok = gi_mag_ok(pos, a, p.radius);
      marches = march_is_proj(kMarch) ? mag_ok : true;  // see below: the projective march takes no pixel of absurd magnitude
    }
  }
  if constexpr (kCert) {
    if (gi_any_lane_marches(marches)) stage_cert_table<kCertOff>(p, cert_tab);
  }
  if (inside && p.start < p.step) {
    if (!tbn_never_hits(tbn)) {
      const __amdgpu_buffer_rsrc_t pos_z = z_plane_rsrc(pos_map + 2 * (size_t)HW, HW);
      const float cx = float(p.W) / 2.0f, cy = float(p.H) / 2.0f;
      // the live rays [0, n_live) are split across the waves; rays behind them (zero-weight ones a caller asked to be
      // marched all the same: none by default) go round-robin to the waves afterwards, so the live rays' partial sums do
      // not depend on them
      const int chunk = (p.n_live + kGiWaves - 1) / kGiWaves;
      const int r0 = wave * chunk, r1 = min(p.n_live, r0 + chunk);
      if constexpr (march_is_proj(kMarch)) {
        // absurd magnitudes (|pos| >= 2^59) are outside the projective march's contract: such a pixel takes no hits
        if (mag_ok) {
          const FastPix c = make_fast(p, pos, cx, cy);
          const float inv_scale = kCert ? __uint_as_float((127u - (unsigned)p.cert_shift) << 23) : 1.0f;  // 2^-shift
          const FastTbn ft = make_fast_tbn(p, tbn, a, inv_scale);
          const CertPix cp = make_cert(p, c, inv_scale);
          // the four waves of a workgroup share its 64 pixels and split the ray set: contiguous quarters (a quarter of the
          // azimuths each), or interleaved pairs (every wave sees every direction: equal work per wave -- the workgroup
          // holds its slots until its slowest wave is done)
          const int rs = p.ray_interleave ? 2 * wave : r0, re = p.ray_interleave ? p.n_live : r1;
          const int rstep = p.ray_interleave ? 2 * kGiWaves : 2;
          auto pair = [&](int r, int rb) {
            f32x2 Bxy[2], Bz2;
            float bz0, bz1;
            fast_ray(ft, rays[2 * r], Bxy[0], bz0);
            fast_ray(ft, rays[2 * rb], Bxy[1], bz1);
            Bz2 = f32x2{bz0, bz1};
            int hit[2];
            if constexpr (kCert) march2_cert<kGiGroup, kCertOff>(p, c, cp, Bxy, Bz2, pos_z, hit);
            else march2_fast<kGiGroup>(p, c, Bxy, Bz2, pos_z, hit);
            occ += hit[0] >= 0 ? rays[2 * r + 1].y : 0.0f;
            occ += (hit[1] >= 0 && rb != r) ? rays[2 * rb + 1].y : 0.0f;
          };
          for (int r = rs; r < re; r += rstep) pair(r, min(r + 1, re - 1));  // an odd chunk marches its last ray twice and counts it once
          for (int r = p.n_live + wave; r < p.nrays; r += kGiWaves) pair(r, r);
        }
      } else {
      const unsigned sv_min_bits = gi_sv_min_bits(a, p.radius, p.inv_step);
      int r = r0;
      for (; r + kGiRays <= r1; r += kGiRays) {
        v3 sv[kGiRays];
        float w[kGiRays];
        int hit[kGiRays];
#pragma unroll
        for (int k = 0; k < kGiRays; k++) {
          const float4 ra = rays[2 * (r + k)];  // wave-uniform -> scalar loads
          w[k] = rays[2 * (r + k) + 1].y;
          sv[k] = tbn_apply(tbn, ra.x, ra.y, ra.z);
        }
        march<kPow2, kGiGroup, kGiRays>(p, pos, a, sv, cx, cy, pos_z, mag_ok, sv_min_bits, hit);
#pragma unroll
        for (int k = 0; k < kGiRays; k++) occ += hit[k] >= 0 ? w[k] : 0.0f;  // x + 0 is exact: ray order kept
      }
      auto single = [&](int q) {
        const float4 ra = rays[2 * q];
        const v3 sv = tbn_apply(tbn, ra.x, ra.y, ra.z);
        int hit;
        march<kPow2, kGiGroup, 1>(p, pos, a, &sv, cx, cy, pos_z, mag_ok, sv_min_bits, &hit);
        occ += hit >= 0 ? rays[2 * q + 1].y : 0.0f;
      };
      for (; r < r1; r++) single(r);
      for (r = p.n_live + wave; r < p.nrays; r += kGiWaves) single(r);
      }
    }
  }
  s_part[wave][lane] = occ;
  __syncthreads();
  if (wave == 0 && inside) {
    const float tot = ((s_part[0][lane] + s_part[1][lane]) + s_part[2][lane]) + s_part[3][lane];
    if (sum_w > 0.0f)
      occlusion[pix_id] = fmaxf(0.0f, fminf(1.0f, (float)(1.0 - (double)(tot / sum_w))));
    else
      occlusion[pix_id] = 1.0f;
  }
}

// wave 0's sum of the four waves' partial sums of one light, in the fixed order ((w0 + w1) + w2) + w3
__device__ __forceinline__ v3 fold_waves(const float (&s_part)[kGiWaves][3][64], int lane) {
  return {((s_part[0][0][lane] + s_part[1][0][lane]) + s_part[2][0][lane]) + s_part[3][0][lane],
          ((s_part[0][1][lane] + s_part[1][1][lane]) + s_part[2][1][lane]) + s_part[3][1][lane],
          ((s_part[0][2][lane] + s_part[1][2][lane]) + s_part[2][2][lane]) + s_part[3][2][lane]};
}

// The SSR march of one workgroup, gathering kLights radiance planes at once (rgb, color and abd are [kLights,3,H,W]): WHICH
// pixel a ray hits does not depend on the radiance (see SsrHits), so every light's sum takes the same hits in the same
// order, each with the single-light expression -- light l's outputs are the single-light march's with rgb = rgb[l], bit
// for bit.  The per-wave partial sums go through the same 3 KB of LDS one light at a time.
template <March kMarch, int kHits = 0, int kLights = 1>
__global__ void __launch_bounds__(256) GIGS_SSR_OCC_L(kLights)
ssr_kernel(GiParams p, const float4* __restrict__ rays, const float* __restrict__ nrm,
           const float* __restrict__ pos_map, const float* __restrict__ rgb,
           const float* __restrict__ albedo_map, const float* __restrict__ metallic_map,
           const float* __restrict__ F0_map, float* __restrict__ color, float* __restrict__ abd,
           const float2* __restrict__ cert_tab, SsrHits hits) {
  __shared__ float s_part[kGiWaves][3][64];
  extern __shared__ float2 s_cert[];
  static_assert(kHits == 0 || march_is_proj(kMarch), "hit lists exist for the projective march only");
  constexpr bool kPow2 = kMarch == March::kExactPow2, kCert = kMarch == March::kProjCert;
  constexpr int kCertOff = sizeof(float) * kGiWaves * 3 * 64;  // dynamic LDS follows the static array
  int x, y, wave;
  const bool inside = gi_pixel(p, x, y, wave);
  const unsigned HW = (unsigned)(p.H * p.W), pix_id = inside ? (unsigned)(p.W * y + x) : 0u;  // W, H < 2^15: 3 HW < 2^32
  v3 diffuse[kLights];
#pragma unroll
  for (int l = 0; l < kLights; l++) diffuse[l] = {0, 0, 0};
  unsigned hpos = 0;  // kHits: hits of this (pixel, wave) so far / the next entry's position
  // The pixel's position and tangent frame belong to the march's PREAMBLE: they are folded into the march's own per-pixel
  // state (FastPix, FastTbn, CertPix; the exact marches keep them for their sample vectors) and end with it.  The finish
  // behind the march builds its own copies -- twelve registers that would otherwise live across every ray of every lane
  // for the sake of wave 0's last forty instructions.
  const v3 pos = {pos_map[pix_id], pos_map[HW + pix_id], pos_map[2 * HW + pix_id]};
  const Tbn tbn = make_tbn({nrm[pix_id], nrm[HW + pix_id], nrm[2 * HW + pix_id]});
  const float a = 1 + pos.z / 100;
  const bool mag_ok = gi_mag_ok(pos, a, p.radius);
  const bool enters = inside && p.start < p.step && !tbn_never_hits(tbn);
  if constexpr (kCert) {
    if (gi_any_lane_marches(enters && mag_ok)) stage_cert_table<kCertOff>(p, cert_tab);  // else: nothing reads the table
  }
  if (enters) {
    const __amdgpu_buffer_rsrc_t pos_z = z_plane_rsrc(pos_map + 2 * (size_t)HW, HW);
    const float cx = float(p.W) / 2.0f, cy = float(p.H) / 2.0f;
    const int chunk = (p.n_live + kGiWaves - 1) / kGiWaves;  // see ssao_kernel
    const int r0 = wave * chunk, r1 = min(p.n_live, r0 + chunk);
    if constexpr (kHits == 2) hpos = hits.offsets[4 * pix_id + wave];
    auto add_hit = [&](int q, float cos_t, float sin_t, int ray) {
      if (q >= 0) {
        // rgb * cosf(theta) * sinf(theta), left to right (forward.cu:824-826)
#pragma unroll
        for (int l = 0; l < kLights; l++) {
          const float* c = rgb + (size_t)l * 3 * HW;
          diffuse[l].x += c[q] * cos_t * sin_t;
          diffuse[l].y += c[HW + q] * cos_t * sin_t;
          diffuse[l].z += c[2 * HW + q] * cos_t * sin_t;
        }
        if constexpr (kHits == 1) hpos++;
        if constexpr (kHits == 2) {
          if (hpos < hits.capacity) hits.entries[hpos] = make_uint2((unsigned)q, (unsigned)ray);
          hpos++;
        }
      }
      (void)ray;
    };
    if constexpr (march_is_proj(kMarch)) {
      if (mag_ok) {  // see ssao_kernel
        const FastPix c = make_fast(p, pos, cx, cy);
        const float inv_scale = kCert ? __uint_as_float((127u - (unsigned)p.cert_shift) << 23) : 1.0f;  // 2^-shift
        const FastTbn ft = make_fast_tbn(p, tbn, a, inv_scale);
        const CertPix cp = make_cert(p, c, inv_scale);
        const int rs = p.ray_interleave ? 2 * wave : r0, re = p.ray_interleave ? p.n_live : r1;
        const int rstep = p.ray_interleave ? 2 * kGiWaves : 2;
        auto pair = [&](int r, int rb) {
          const float4 ra0 = rays[2 * r], ra1 = rays[2 * rb];
          f32x2 Bxy[2], Bz2;
          float bz0, bz1;
          fast_ray(ft, ra0, Bxy[0], bz0);
          fast_ray(ft, ra1, Bxy[1], bz1);
          Bz2 = f32x2{bz0, bz1};
          int hit[2];
          if constexpr (kCert) march2_cert<kGiGroup, kCertOff>(p, c, cp, Bxy, Bz2, pos_z, hit);
          else march2_fast<kGiGroup>(p, c, Bxy, Bz2, pos_z, hit);
          if (rb == r) hit[1] = -1;
          if (__any(hit[0] >= 0 || hit[1] >= 0)) {
            add_hit(hit[0], ra0.w, rays[2 * r + 1].x, r);
            add_hit(hit[1], ra1.w, rays[2 * rb + 1].x, rb);
          }
        };
        for (int r = rs; r < re; r += rstep) pair(r, min(r + 1, re - 1));
        // the zero-weight ray (ONE representative by default): rgb * cos * 0 = +-0, or NaN for a non-finite hit pixel
        for (int r = p.n_live + wave; r < p.nrays; r += kGiWaves) pair(r, r);
      }
    } else {
    const unsigned sv_min_bits = gi_sv_min_bits(a, p.radius, p.inv_step);
    int r = r0;
    for (; r + kGiRays <= r1; r += kGiRays) {
      v3 sv[kGiRays];
      float ct[kGiRays], st[kGiRays];
      int hit[kGiRays];
#pragma unroll
      for (int k = 0; k < kGiRays; k++) {
        const float4 ra = rays[2 * (r + k)];
        ct[k] = ra.w;
        st[k] = rays[2 * (r + k) + 1].x;
        sv[k] = tbn_apply(tbn, ra.x, ra.y, ra.z);
      }
      march<kPow2, kGiGroup, kGiRays>(p, pos, a, sv, cx, cy, pos_z, mag_ok, sv_min_bits, hit);
      bool any_hit = false;
#pragma unroll
      for (int k = 0; k < kGiRays; k++) any_hit = any_hit || hit[k] >= 0;
      if (__any(any_hit)) {  // hits are rare: one wave-uniform test per ray pair
#pragma unroll
        for (int k = 0; k < kGiRays; k++) add_hit(hit[k], ct[k], st[k], r + k);
      }
    }
    auto single = [&](int q) {
      const float4 ra = rays[2 * q];
      const v3 sv = tbn_apply(tbn, ra.x, ra.y, ra.z);
      int hit;
      march<kPow2, kGiGroup, 1>(p, pos, a, &sv, cx, cy, pos_z, mag_ok, sv_min_bits, &hit);
      add_hit(hit, ra.w, rays[2 * q + 1].x, q);
    };
    for (; r < r1; r++) single(r);
    for (r = p.n_live + wave; r < p.nrays; r += kGiWaves) single(r);
    }
  }
  // Behind the march the lane, the wave, the pixel and the planes' offsets are derived again from the thread index (which
  // the compiler cannot relate to the preamble's): otherwise the three 64-bit plane offsets, the in-image mask and the
  // wave index stay allocated across the march.
  unsigned tid = threadIdx.x;
  asm volatile("" : "+v"(tid));
  const int lane = tid & 63;
  int xf, yf, wave_f;
  const bool inside_f = gi_pixel(p, tid, xf, yf, wave_f);
  const unsigned pix_f = inside_f ? (unsigned)(p.W * yf + xf) : 0u;
  if constexpr (kHits == 1) {
    if (inside_f) hits.counts[4 * pix_f + wave_f] = hpos;
  }
  // lights 0 .. kLights - 2 through LDS one at a time (multi-light instances only) ...
#pragma unroll
  for (int l = 0; l < kLights - 1; l++) {
    s_part[wave_f][0][lane] = diffuse[l].x;
    s_part[wave_f][1][lane] = diffuse[l].y;
    s_part[wave_f][2][lane] = diffuse[l].z;
    __syncthreads();
    if (wave_f == 0 && inside_f) diffuse[l] = fold_waves(s_part, lane);
    __syncthreads();  // wave 0 has read them before the next light overwrites them
  }
  // ... and the last one
  constexpr int kLast = kLights - 1;
  s_part[wave_f][0][lane] = diffuse[kLast].x;
  s_part[wave_f][1][lane] = diffuse[kLast].y;
  s_part[wave_f][2][lane] = diffuse[kLast].z;
  __syncthreads();
  if (wave_f != 0 || !inside_f) return;
  diffuse[kLast] = fold_waves(s_part, lane);
  // the finish's own position and frame: the same planes, the same make_tbn, hence the same bits as the preamble's -- for
  // every pixel, a NaN frame or one that never marched included -- read through pointers the compiler cannot trace back
  const float *nrm_f = launder_ptr(nrm), *pos_f = launder_ptr(pos_map);
  const v3 pos_fin = {pos_f[pix_f], pos_f[HW + pix_f], pos_f[2 * HW + pix_f]};
  const Tbn tbn_fin = make_tbn({nrm_f[pix_f], nrm_f[HW + pix_f], nrm_f[2 * HW + pix_f]});
#pragma unroll
  for (int l = 0; l < kLights; l++)
    ssr_finish(diffuse[l], tbn_fin, pos_fin, pix_f, HW, p.nrays_total, albedo_map, metallic_map, F0_map,
               color + (size_t)l * 3 * HW, abd + (size_t)l * 3 * HW);
}

constexpr int kSsrMaxLights = 4;  // GIGS_SSR_LIGHTS_PER_MARCH (include/gigs_hip.h)

static GiParams make_params(const Options& o, int W, int H, float fx, float fy, float radius, float bias, float thick,
                            int step, int start, const RayTable& t, bool ssr, bool& pow2) {
  GiParams p;
  p.W = W; p.H = H; p.fx = fx; p.fy = fy; p.radius = radius; p.bias = bias; p.thick = thick;
  p.step = step; p.start = start;
  p.n_live = t.n_live;
  // zero-weight rays (see the ray table): all of them on request, else one for SSR (NaN propagation) and none for SSAO
  p.nrays = t.n_live + (o.gi_zero_rays ? t.n_dead : (ssr && t.n_dead > 0 ? 1 : 0));
  p.nrays_total = t.nrays;
  pow2 = step > 0 && (step & (step - 1)) == 0 && step <= (1 << 20);
  p.inv_step = pow2 ? 1.0f / (float)step : 0.0f;
  if (step - start > 64 - kGiGroup) pow2 = false;  // a partial last group may index kGiGroup - 1 entries past step - 1
  // j / step: exact for a power-of-two step; otherwise the correctly rounded quotient (read by the projective march only)
  for (int k = 0; k < 64; k++) p.fjt[k] = pow2 ? (float)(start + k) * p.inv_step : (float)(start + k) / (float)step;
  for (int k = 0; k < 64; k++) p.fjc[k] = p.fjt[k < step - 1 - start ? k : (step - 1 - start > 0 ? step - 1 - start : 0)];
  // gi_tile_log2w: tuning knob for the pixel rectangle of a workgroup (3 = 8x8 ... 6 = 64x1)
  p.tile_log2w = (o.gi_tile_log2w >= 0 && o.gi_tile_log2w <= 6) ? o.gi_tile_log2w : kGiTileLog2W;
  p.ray_interleave = o.gi_interleave ? 1 : 0;  // measured at C2: SSAO 0.94 -> 0.89, SSR 0.93 -> 0.90 ms (0: quarters)
  return p;
}
// Certification table, (bw + 1) x (bh + 1) entries.  Per (1 << shift)^2 block of the z plane: the minimum over its non-zero
// pixels (+inf if none) and max(maximum, 0) -- NaN pixels are ignored (a NaN never passes the depth test) -- turned into
// the two thresholds {t_lo, t_hi} on a sample's denominator (CertK): the march then certifies with three compares and no
// arithmetic.  The last column / row (indices bw / bh: where out-of-image block coordinates clamp to, negative ones
// included, being huge as unsigned) and blocks the image covers only partly hold {-inf, +inf}: nothing is ever certified
// there, so samples that may lie outside the image always take the exact path.  One wave per entry.
__global__ void __launch_bounds__(64)
gi_minmax_kernel(int W, int H, int shift, int bw, int bh, CertK ck, const float* __restrict__ z, float2* __restrict__ tab) {
  const int bx = (int)blockIdx.x, by = (int)blockIdx.y, B = 1 << shift;
  float mn = __builtin_inff(), mx = 0.0f;
  const bool full = bx < bw && by < bh && ((bx + 1) << shift) <= W && ((by + 1) << shift) <= H;
  if (full) {
    for (int i = threadIdx.x; i < B * B; i += 64) {
      const float v = z[(size_t)((by << shift) + (i >> shift)) * W + (bx << shift) + (i & (B - 1))];
      if (v != 0.0f) mn = fminf(mn, v);  // false for NaN too: fminf would ignore it anyway
      mx = fmaxf(mx, v);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      mn = fminf(mn, __shfl_xor(mn, o));
      mx = fmaxf(mx, __shfl_xor(mx, o));
    }
  } else {
    mn = -__builtin_inff();
    mx = __builtin_inff();
  }
  if (threadIdx.x == 0) {
    // thresholds on den (see CertK), each moved away from certification by 2^-20 relative
    float t_hi = (mx - ck.lo_k) / (1.0f - 0x1p-16f);
    t_hi = t_hi + fabsf(t_hi) * 0x1p-20f + 1e-30f;
    float t_lo = (mn - ck.hi_k) / (1.0f + 0x1p-16f);
    t_lo = t_lo - fabsf(t_lo) * 0x1p-20f - 1e-30f;
    if (!(mx == mx) || !(mn == mn)) { t_hi = __builtin_inff(); t_lo = -__builtin_inff(); }  // NaN depths: never certify
    tab[(size_t)by * (bw + 1) + bx] = make_float2(t_lo, t_hi);
  }
}

// block size of the certification table: the smallest of 16 / 32 / 64 pixels whose table fits kCertMaxBytes of LDS
constexpr int kCertMaxBytes = 40 * 1024;
static size_t cert_table_bytes(int W, int H, int sh) {
  return (size_t)(((W + (1 << sh) - 1) >> sh) + 2) * (((H + (1 << sh) - 1) >> sh) + 2) * sizeof(float2);
}
static int cert_shift_for(int W, int H) {
  for (int sh = 4; sh <= 6; sh++)
    if (cert_table_bytes(W, H, sh) <= (size_t)kCertMaxBytes) return sh;
  return 0;
}
size_t gi_scratch_bytes(int W, int H) {
  const int sh = cert_shift_for(W, H);
  return sh ? cert_table_bytes(W, H, sh) : 0;
}
// fills p.cert_*; returns the table's byte size (0 = run without certification)
static size_t prepare_cert(const Options& o, GiParams& p, int mode, const float* pos, void* scratch, hipStream_t s) {
  p.cert_shift = p.cert_w = p.cert_h = 0;
  p.cert_d0 = cert_consts(p.bias, p.thick).d0;
  if (!scratch || mode != 4 || !o.gi_cert) return 0;
  const int sh = cert_shift_for(p.W, p.H);
  if (!sh) return 0;
  p.cert_shift = sh;
  p.cert_w = (p.W + (1 << sh) - 1) >> sh;
  p.cert_h = (p.H + (1 << sh) - 1) >> sh;
  hipLaunchKernelGGL(gi_minmax_kernel, dim3(p.cert_w + 1, p.cert_h + 1), dim3(64), 0, s, p.W, p.H, sh, p.cert_w, p.cert_h,
                     cert_consts(p.bias, p.thick), pos + 2 * (size_t)p.H * p.W, (float2*)scratch);
  return cert_table_bytes(p.W, p.H, sh);
}

// gigs_options.gi_march: 0 exact | 4 proj (see the block comment above march2_fast; GIGS_GI_MARCH names them in the
// environment).  The projective march reads the j/step table, so marches of more than 64 - kGiGroup steps take the exact
// path.
#ifndef GIGS_GI_DEFAULT_MODE
#define GIGS_GI_DEFAULT_MODE 4  // "proj": measured 1.3e-7 mean L1 / 1e-4 changed pixels vs the exact march at C2
#endif
static int gi_march_mode(const Options& o, int step, int start) {
  int mode = (o.gi_march == 0 || o.gi_march == 4) ? o.gi_march : GIGS_GI_DEFAULT_MODE;
  if (step - start > 64 - kGiGroup || step <= 0) mode = 0;
  return mode;
}
// Calls f(the march as a std::integral_constant, the kernel's dynamic LDS bytes) for what gi_march_mode, make_params
// (pow2) and prepare_cert (the certification table's size, 0 = none) decided.
template <March kMarch> using MarchTag = std::integral_constant<March, kMarch>;
template <class F>
static void gi_dispatch_march(int mode, bool pow2, size_t cert, F&& f) {
  if (mode == 4) {
    if (cert) f(MarchTag<March::kProjCert>{}, cert);
    else f(MarchTag<March::kProj>{}, (size_t)0);
  } else {
    if (pow2) f(MarchTag<March::kExactPow2>{}, (size_t)0);
    else f(MarchTag<March::kExact>{}, (size_t)0);
  }
}
static dim3 gi_grid(const GiParams& p) {
  const int tw = 1 << p.tile_log2w, th = 64 >> p.tile_log2w;
  return dim3((p.W + tw - 1) / tw, (p.H + th - 1) / th);
}

// What the three march launchers decide before their own kernels: the ray table entry, the kernel parameters, the
// grid, which march runs and -- queued on `s` here, in front of every march that follows -- the certification table.
struct MarchPlan {
  RayTable t;
  GiParams p;
  dim3 grid;
  int mode;    // gi_march_mode
  bool pow2;   // make_params
  size_t cert;  // bytes of the certification table = the kernels' dynamic LDS; 0 = no certification
  const float2* tab;
};
// 0, or the launcher's status: get_ray_table's, or -2 for an oversized image (rejected with a message by the C-ABI wrapper)
static int plan_march(const Options& o, int W, int H, float fx, float fy, float radius, float bias, float thick, float delta,
                      int step, int start, bool ssr, const float* pos, void* scratch, hipStream_t s, MarchPlan& m) {
  const int rc = get_ray_table(delta, s, m.t);
  if (rc) return rc;
  m.p = make_params(o, W, H, fx, fy, radius, bias, thick, step, start, m.t, ssr, m.pow2);
  if (W >= (1 << 15) || H >= (1 << 15)) return -2;
  m.grid = gi_grid(m.p);
  m.mode = gi_march_mode(o, step, start);
  m.cert = (start < step) ? prepare_cert(o, m.p, m.mode, pos, scratch, s) : 0;
  m.tab = (const float2*)scratch;
  return 0;
}

int launch_ssao(const Options& o, int W, int H, float fx, float fy, float radius, float bias, float thick,
                float delta, int step, int start, const float* normal, const float* pos,
                float* occlusion, void* scratch, hipStream_t s) {
  MarchPlan m;
  const int rc = plan_march(o, W, H, fx, fy, radius, bias, thick, delta, step, start, /*ssr*/ false, pos, scratch, s, m);
  if (rc) return rc;
  gi_dispatch_march(m.mode, m.pow2, m.cert, [&](auto march, size_t lds) {
    hipLaunchKernelGGL((ssao_kernel<decltype(march)::value>), m.grid, dim3(256), lds, s, m.p, m.t.dev, m.t.sum_w, normal, pos,
                       occlusion, m.tab);
  });
  return 0;
}

int launch_ssr(const Options& o, int W, int H, float fx, float fy, float radius, float bias, float thick,
               float delta, int step, int start, const float* normal, const float* pos,
               const float* rgb, const float* albedo, const float* /*roughness*/,
               const float* metallic, const float* F0, float* color, float* abd, void* scratch, hipStream_t s,
               int hits_mode, unsigned* hit_counts, const unsigned* hit_offsets, void* hit_entries, unsigned hit_capacity) {
  MarchPlan m;
  const int rc = plan_march(o, W, H, fx, fy, radius, bias, thick, delta, step, start, /*ssr*/ true, pos, scratch, s, m);
  if (rc) return rc;
  const SsrHits hits = {hit_counts, hit_offsets, (uint2*)hit_entries, hit_capacity};
  // the hit-list variants exist for the default march only (mode 4, with or without certification); -3 = not available
  if (hits_mode != 0 && (m.mode != 4 || (hits_mode != 1 && hits_mode != 2) || !(start < step))) return -3;
  gi_dispatch_march(m.mode, m.pow2, m.cert, [&](auto march, size_t lds) {
    constexpr March kMarch = decltype(march)::value;
    auto launch = [&](auto kernel) {
      hipLaunchKernelGGL(kernel, m.grid, dim3(256), lds, s, m.p, m.t.dev, normal, pos, rgb, albedo, metallic, F0, color, abd,
                         m.tab, hits);
    };
    if constexpr (march_is_proj(kMarch)) {
      if (hits_mode == 1) return launch(ssr_kernel<kMarch, 1>);
      if (hits_mode == 2) return launch(ssr_kernel<kMarch, 2>);
    }
    launch(ssr_kernel<kMarch>);
  });
  return 0;
}

// K radiance planes over one geometry (gigs_ssr_multi): the certification table is built once, then ceil(K / kSsrMaxLights)
// marches gather up to kSsrMaxLights planes each; a chunk of one light is the single-light kernel itself.
template <int kLights>
static void launch_ssr_chunk(const MarchPlan& m, const float* normal, const float* pos, const float* rgb, const float* albedo,
                             const float* metallic, const float* F0, float* color, float* abd, hipStream_t s) {
  const SsrHits hits = {nullptr, nullptr, nullptr, 0};
  gi_dispatch_march(m.mode, m.pow2, m.cert, [&](auto march, size_t lds) {
    hipLaunchKernelGGL((ssr_kernel<decltype(march)::value, 0, kLights>), m.grid, dim3(256), lds, s, m.p, m.t.dev, normal, pos, rgb,
                       albedo, metallic, F0, color, abd, m.tab, hits);
  });
}

int launch_ssr_multi(const Options& o, int n_lights, int W, int H, float fx, float fy, float radius, float bias, float thick,
                     float delta, int step, int start, const float* normal, const float* pos, const float* rgb,
                     const float* albedo, const float* metallic, const float* F0, float* color, float* abd, void* scratch,
                     hipStream_t s) {
  MarchPlan m;
  const int rc = plan_march(o, W, H, fx, fy, radius, bias, thick, delta, step, start, /*ssr*/ true, pos, scratch, s, m);
  if (rc) return rc;
  const size_t plane = (size_t)3 * W * H;
  for (int l0 = 0; l0 < n_lights; l0 += kSsrMaxLights) {
    const int n = min(kSsrMaxLights, n_lights - l0);
    const float* c_rgb = rgb + l0 * plane;
    float *c_color = color + l0 * plane, *c_abd = abd + l0 * plane;
    static_assert(kSsrMaxLights == 4, "one case per chunk size");
    switch (n) {
      case 1: launch_ssr_chunk<1>(m, normal, pos, c_rgb, albedo, metallic, F0, c_color, c_abd, s); break;
      case 2: launch_ssr_chunk<2>(m, normal, pos, c_rgb, albedo, metallic, F0, c_color, c_abd, s); break;
      case 3: launch_ssr_chunk<3>(m, normal, pos, c_rgb, albedo, metallic, F0, c_color, c_abd, s); break;
      default: launch_ssr_chunk<4>(m, normal, pos, c_rgb, albedo, metallic, F0, c_color, c_abd, s);
    }
  }
  return 0;
}

// diagnostic: fast shared-reciprocal division vs the compiler's IEEE division
__global__ void __launch_bounds__(256)
selftest_div2_kernel(int n, const float* __restrict__ nx, const float* __restrict__ ny,
                     const float* __restrict__ d, float* __restrict__ out_fast, float* __restrict__ out_ref,
                     int* __restrict__ out_round) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float big = fmaxf(fmaxf(fabsf(nx[i]), fabsf(ny[i])), fabsf(d[i]));
  const float small = fminf(fabsf(nx[i]), fabsf(ny[i]));
  // numerators below 2^-60 are exercised only through the march (absorbed by + cx), not here
  const f32x2 q = div2_exact(f32x2{nx[i], ny[i]}, d[i], big < 0x1p60f && small > 0x1p-60f);
  out_fast[2 * i] = q.x;
  out_fast[2 * i + 1] = q.y;
  out_ref[2 * i] = nx[i] / d[i];
  out_ref[2 * i + 1] = ny[i] / d[i];
  out_round[2 * i] = round_to_int(nx[i]);
  out_round[2 * i + 1] = f2i(roundf(nx[i]));
}

// exhaustive: every fp32 bit pattern; counts the t for which round_pix and (int)roundf would decide differently
__global__ void __launch_bounds__(256) selftest_round_kernel(unsigned long long* __restrict__ bad) {
  unsigned long long local = 0;
  for (unsigned long long b = (unsigned long long)blockIdx.x * 256 + threadIdx.x; b < (1ull << 32);
       b += (unsigned long long)gridDim.x * 256) {
    const float t = __uint_as_float((unsigned)b);
    const int a = f2i(roundf(t)), r = round_pix(t);
    const bool same = a == r || (a < 0 && r < 0) || (a >= 32767 && r >= 32767);
    local += same ? 0 : 1;
  }
  if (local) atomicAdd(bad, local);
}

}  // namespace gigs

extern "C" int gigs_selftest_round(unsigned long long* mismatches, void* stream) {
  if (!mismatches) return -1;
  if (hipMemsetAsync(mismatches, 0, sizeof(unsigned long long), (hipStream_t)stream) != hipSuccess) return -2;
  hipLaunchKernelGGL(gigs::selftest_round_kernel, dim3(16384), dim3(256), 0, (hipStream_t)stream, mismatches);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}

extern "C" int gigs_selftest_div2(int n, const float* nx, const float* ny, const float* d, float* out_fast,
                                  float* out_ref, int* out_round, void* stream) {
  if (n <= 0 || !nx || !ny || !d || !out_fast || !out_ref || !out_round) return -1;
  hipLaunchKernelGGL(gigs::selftest_div2_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, n, nx, ny, d,
                     out_fast, out_ref, out_round);
  return hipGetLastError() == hipSuccess ? 0 : -2;
}
