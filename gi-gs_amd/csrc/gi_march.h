// gi_march.h -- the device arithmetic of the screen-space ray march: what one lane does with one pixel and one or two
// rays.  Shared by the SSAO / SSR march kernels (gi.hip) and, for the part behind the march (Tbn, ssr_finish, SsrHits),
// by the hit-list gather (ssr_apply.hip).  Device-inline code and plain structs only: no kernel, no host function, no
// state.
//
// Reference behaviour restated (R/ = submodules/diff-gaussian-rasterization):
//   the ray loop of SSAOCUDA  R/cuda_rasterizer/forward.cu:691-714   (get_coord   ssr.h:120-135)
//   the ray loop of SSRCUDA   forward.cu:805-830, its tail :833-909   (fresnelSchlick ssr.h:13-16)
//
// MI355X design of the march (the dominant cost at start < step: rays * steps dependent gathers per pixel):
//   * per-step arithmetic of the exact march keeps the reference's operation order and IEEE division, so pixel
//     coordinates (roundf of a projected float) are bit-identical to the oracle's; the only
//     exact rewrite is `x / step` -> `x * (1/step)` when step is a power of two;
//   * the projective march (the default) spends the tolerance of the fp planes on 3 packed FMAs + one rcp per sample,
//     and a conservative certification table in LDS lets ~92 % of its wave-samples skip the z-plane gather;
//   * SSR reads the rgb planes only on a hit (the reference reads them every step but uses
//     them only on a hit: forward.cu:820-826).
#pragma once

#include <cmath>

#include "gigs_common.h"
#include "pixel_ops.h"

namespace gigs {

constexpr float kPiF = 3.14159265358979323846f;

struct GiParams {
  int W, H;
  float fx, fy, radius, bias, thick;
  int step, start;
  float inv_step;  // exact 1/step when step is a power of two
  int n_live;       // rays [0, n_live) are split across the four waves of a workgroup
  int nrays;        // rays [n_live, nrays) behind them go round-robin to the waves (zero-weight rays: none for SSAO, one for SSR)
  int nrays_total;  // all rays of the reference's loops (SSR's nrSamples)
  int tile_log2w;  // the 64 pixels of a workgroup form a (1 << tile_log2w) x (64 >> tile_log2w) rectangle
  int ray_interleave;  // projective march: wave w takes ray pairs w, w + 4, ... instead of the w-th quarter of the ray set
  int cert_shift;      // certification blocks are (1 << cert_shift)^2 pixels; 0 = no certification table
  int cert_w, cert_h;  // blocks per row / column of the image; the table is (cert_w + 1) x (cert_h + 1): last column / row = border
  float cert_d0;       // certification needs den > cert_d0 (CertK::d0)
  // j / step for j = start .. start + 63 (exact for a power-of-two step): the fast path reads its per-step factor from
  // here with a scalar load instead of converting and multiplying on the vector ALU for every group (marches of more
  // than kFjTable - kGiGroup steps take the general path)
  float fjt[64];
  float fjc[64];  // fjt with the entries past the last step (step - 1 - start) repeating the last one
};

typedef float f32x2 __attribute__((ext_vector_type(2)));

// (x / d, y / d) with both quotients correctly rounded, i.e. bit-identical to two IEEE
// divisions.  hipcc expands an fp32 division into v_div_scale x2, v_rcp, a Newton step on the
// reciprocal, three residual FMAs, v_div_fmas and v_div_fixup.  When neither operand needs the
// exponent pre-scaling of v_div_scale (|values| within 2^-60 .. 2^60) the scale and fixup are
// identities and the quotient is exactly the FMA chain below; the reciprocal refinement is
// shared between the two numerators and the residual steps run as packed fp32 FMAs
// (v_pk_fma_f32): 1 rcp + 2 FMA + 5 packed ops instead of 22 instructions.
// (Checked bit-for-bit against `/` on the device: tests/test_gpu_parity.py::test_fast_div2.)
// `mag_ok` = the caller guarantees |n.x|, |n.y|, |d| < 2^60 (no overflow / pre-scaling); the
// denominator must also be away from zero.  A tiny or zero NUMERATOR is harmless here: the chain
// then returns the correctly signed tiny quotient or a zero of either sign, and the caller adds
// cx/cy (>= 0.5) to q * fx, which absorbs both.
__device__ __forceinline__ f32x2 div2_exact(f32x2 n, float d, bool mag_ok) {
  if (mag_ok && fabsf(d) > 0x1p-60f) {
    const float r0 = __builtin_amdgcn_rcpf(d);
    const float e0 = __builtin_fmaf(-d, r0, 1.0f);
    const float r1 = __builtin_fmaf(e0, r0, r0);
    const f32x2 nd = {-d, -d}, rr = {r1, r1};
    const f32x2 q0 = n * rr;
    const f32x2 e1 = __builtin_elementwise_fma(nd, q0, n);
    const f32x2 q1 = __builtin_elementwise_fma(e1, rr, q0);
    const f32x2 e2 = __builtin_elementwise_fma(nd, q1, n);
    return __builtin_elementwise_fma(e2, rr, q1);
  }
  return f32x2{n.x / d, n.y / d};
}

// The FMA chain alone (valid under the conditions stated above; garbage otherwise).
__device__ __forceinline__ f32x2 div2_fast(f32x2 n, float d) {
  const float r0 = __builtin_amdgcn_rcpf(d);
  const float e0 = __builtin_fmaf(-d, r0, 1.0f);
  const float r1 = __builtin_fmaf(e0, r0, r0);
  const f32x2 nd = {-d, -d}, rr = {r1, r1};
  const f32x2 q0 = n * rr;
  const f32x2 e1 = __builtin_elementwise_fma(nd, q0, n);
  const f32x2 q1 = __builtin_elementwise_fma(e1, rr, q0);
  const f32x2 e2 = __builtin_elementwise_fma(nd, q1, n);
  return __builtin_elementwise_fma(e2, rr, q1);
}

// (int)roundf(t) for the GPU's saturating conversion: exhaustively verified over all 2^32 floats
// that trunc(t + copysign(0.5 - 2^-25, t)) rounds half away from zero like roundf.
__device__ __forceinline__ int round_to_int(float t) { return f2i(t + copysignf(0.49999997f, t)); }

// The march only asks "which pixel, if inside the image".  For that, floor(t + (0.5 - 2^-25)) serves as well as
// (int)roundf(t): the two agree for every t >= -0.5 + 2^-25 (above -0.5 the sum is >= 0 and floor = trunc, which is
// the identity above), at t <= -0.5 both are negative, and a NaN converts to 0 either way; beyond +-2^31 both
// saturate.  So they select the same pixel whenever one of them is a valid coordinate of an image side < 2^15, and
// are both outside otherwise.  v_floor_f32 (VOP1) replaces v_bfi_b32 (VOP3: ~1.5 cycles more per coordinate).
// Checked over ALL 2^32 floats on the device: gigs_selftest_round.
__device__ __forceinline__ int round_pix(float t) { return f2i(floorf(t + 0.49999997f)); }
// the same for a coordinate pair whose +(0.5 - 2^-25) is done as one packed add
__device__ __forceinline__ int floor_pix(float t_plus_half) { return f2i(floorf(t_plus_half)); }

// Buffer descriptor of one fp32 image plane with a 4-byte stride: an `idxen` load takes the pixel index itself (the
// hardware scales it) and range-checks it against the pixel count, an `offen` load with a byte offset works too.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t z_plane_rsrc(const float* plane, size_t HW) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(plane), /*stride*/ 4, (int)HW, 0x00020000);
}

// N indexed gathers in flight, then one wait.  Inline assembly because clang has no builtin for the indexed (struct)
// buffer load; the destinations are not tracked by the compiler's wait-count insertion, hence the explicit s_waitcnt
// that every result passes through before it is used.
__device__ __forceinline__ float gather_idx_issue(unsigned i, __amdgpu_buffer_rsrc_t rsrc) {
  float z;
  asm volatile("buffer_load_dword %0, %1, %2, 0 idxen" : "=&v"(z) : "v"(i), "s"(rsrc));
  return z;
}
template <int N>
__device__ __forceinline__ void gather_idx(float* z, const unsigned* i, __amdgpu_buffer_rsrc_t rsrc) {
  static_assert(N == 4 || N == 8 || N == 16, "group sizes of the march");
#pragma unroll
  for (int k = 0; k < N; k++) z[k] = gather_idx_issue(i[k], rsrc);
  if constexpr (N == 16) {
    asm volatile("s_waitcnt vmcnt(0)"
                 : "+v"(z[0]), "+v"(z[1]), "+v"(z[2]), "+v"(z[3]), "+v"(z[4]), "+v"(z[5]), "+v"(z[6]), "+v"(z[7]));
    asm volatile("" : "+v"(z[8]), "+v"(z[9]), "+v"(z[10]), "+v"(z[11]), "+v"(z[12]), "+v"(z[13]), "+v"(z[14]), "+v"(z[15]));
  } else if constexpr (N == 8)
    asm volatile("s_waitcnt vmcnt(0)"
                 : "+v"(z[0]), "+v"(z[1]), "+v"(z[2]), "+v"(z[3]), "+v"(z[4]), "+v"(z[5]), "+v"(z[6]), "+v"(z[7]));
  else
    asm volatile("s_waitcnt vmcnt(0)" : "+v"(z[0]), "+v"(z[1]), "+v"(z[2]), "+v"(z[3]));
}

// Sample coordinates of one group of steps for kRays rays: byte offset into the z plane (0 when the sample
// is outside the image), the in-image flag and the sample's z.  kExact = false uses the shared-reciprocal
// FMA chain for every lane and returns the smallest |den| seen, so that the caller can decide ONCE per
// group whether any lane needed the IEEE slow path; kExact = true re-evaluates with per-lane selection.
template <bool kPow2, int kGroup, int kRays, bool kExact>
__device__ __forceinline__ float group_coords(const GiParams& p, v3 pos, float a, const v3* sv, float cx, float cy,
                                              bool mag_ok, int j0, unsigned (*off)[kGroup], bool (*inb)[kGroup],
                                              float (*spzv)[kGroup]) {
  const f32x2 posxy = {pos.x, pos.y}, fxy = {p.fx, p.fy}, cxy = {cx, cy};
  float min_den = __builtin_inff();
#pragma unroll
  for (int g = 0; g < kGroup; g++) {
    // pos + sampleVec * j * (1 + z/100) * (1 + z/100) * radius / step, left to right (forward.cu:693).  For a
    // power-of-two step the final division is an exact scaling, and an exact scaling commutes with every
    // rounding of the chain as long as no intermediate falls into the subnormal range: the fast path folds it
    // into j (j / step is exact) and saves three multiplies per sample; `sv_scale_ok` (checked per ray by the
    // caller) rules the subnormal case out, otherwise the exact path below runs.
    const float fj = (kPow2 && !kExact) ? p.fjt[j0 - p.start + g] : (float)(j0 + g);
    const bool in_range = (j0 + g) < p.step;
#pragma unroll
    for (int k = 0; k < kRays; k++) {
      f32x2 m = f32x2{sv[k].x, sv[k].y} * fj;
      float mz = sv[k].z * fj;
      m = m * a; mz = mz * a;
      m = m * a; mz = mz * a;
      m = m * p.radius; mz = mz * p.radius;
      if (kPow2) {
        if (kExact) { m = m * p.inv_step; mz = mz * p.inv_step; }
      } else {
        const float fs = (float)p.step;
        m = f32x2{m.x / fs, m.y / fs}; mz = mz / fs;
      }
      const f32x2 sp = posxy + m;
      const float spz = pos.z + mz;
      // get_coord (ssr.h:120-135)
      const float den = spz + 0.0000001f;
      f32x2 qv = div2_fast(sp, den);
      if (kExact) {
        if (!(mag_ok && fabsf(den) > 0x1p-60f)) qv = f32x2{sp.x / den, sp.y / den};
      } else {
        min_den = fminf(min_den, fabsf(den));  // a NaN den is not recorded: both paths then give NaN -> pixel (0, 0)
      }
      const f32x2 t = (qv * fxy + cxy) + 0.49999997f;  // round_pix's addend, packed
      const int ix = floor_pix(t.x);
      const int iy = floor_pix(t.y);
      inb[k][g] = in_range && (unsigned)ix < (unsigned)p.W && (unsigned)iy < (unsigned)p.H;
      // The gather goes through a buffer descriptor of exactly the z plane: an out-of-image sample (never
      // used: inb is false) yields some wrapped offset that the hardware range check either reads harmlessly
      // or answers with 0 -- no clamp, no predication.  W, H < 2^15 (checked by the C-ABI wrapper), so the
      // in-image pixel index is exact in the 24-bit multiply.
      off[k][g] = __umul24((unsigned)iy, (unsigned)p.W) + (unsigned)ix;
      spzv[k][g] = spz;
    }
  }
  return min_den;
}

// The same for exactly two rays, with every z-lane scalar of the pair (sample z, denominator, reciprocal
// refinement, the two depth-test bounds) held as one fp32 pair: the kernel is bound by VALU issue and a
// v_pk_* instruction (~4.7 cycles for two elements) is cheaper than two scalar ones that carry an SGPR / literal
// operand or a VOP3 encoding (~4 cycles each; only VGPR-only VOP2 forms reach ~2.5: tools/microbench/pk_forms.hip).  Same IEEE operations per element, same results.  hi2 / lo2 receive spz + bias and
// spz - thick of the two rays (ssr.h hit test operands).
template <bool kPow2, int kGroup, bool kExact>
__device__ __forceinline__ float group_coords2(const GiParams& p, v3 pos, float a, const v3* sv, float cx, float cy,
                                               bool mag_ok, int j0, unsigned (*off)[kGroup], bool (*inb)[kGroup],
                                               f32x2* hi2, f32x2* lo2) {
  const f32x2 posxy = {pos.x, pos.y}, fxy = {p.fx, p.fy}, cxy = {cx, cy};
  const f32x2 posz2 = {pos.z, pos.z}, svz = {sv[0].z, sv[1].z};
  const f32x2 sxy[2] = {f32x2{sv[0].x, sv[0].y}, f32x2{sv[1].x, sv[1].y}};
  float min_den = __builtin_inff();
#pragma unroll
  for (int g = 0; g < kGroup; g++) {
    const float fj = (kPow2 && !kExact) ? p.fjt[j0 - p.start + g] : (float)(j0 + g);  // see group_coords
    const bool in_range = (j0 + g) < p.step;
    f32x2 m[2] = {sxy[0] * fj, sxy[1] * fj};
    f32x2 mz = svz * fj;
    m[0] = m[0] * a; m[1] = m[1] * a; mz = mz * a;
    m[0] = m[0] * a; m[1] = m[1] * a; mz = mz * a;
    m[0] = m[0] * p.radius; m[1] = m[1] * p.radius; mz = mz * p.radius;
    if (kPow2) {
      if (kExact) { m[0] = m[0] * p.inv_step; m[1] = m[1] * p.inv_step; mz = mz * p.inv_step; }
    } else {
      const float fs = (float)p.step;
      m[0] = f32x2{m[0].x / fs, m[0].y / fs}; m[1] = f32x2{m[1].x / fs, m[1].y / fs}; mz = f32x2{mz.x / fs, mz.y / fs};
    }
    const f32x2 spz = posz2 + mz;
    const f32x2 den = spz + 0.0000001f;  // get_coord (ssr.h:120-135)
    // shared-reciprocal division (div2_fast) with the reciprocal refinement of both rays packed
    const f32x2 r0 = {__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)};
    const f32x2 e0 = __builtin_elementwise_fma(-den, r0, f32x2{1.0f, 1.0f});
    const f32x2 r1 = __builtin_elementwise_fma(e0, r0, r0);
    if (!kExact) min_den = fminf(fminf(fabsf(den.x), fabsf(den.y)), min_den);  // NaN dens are not recorded (see group_coords)
    hi2[g] = spz + p.bias;
    lo2[g] = spz - p.thick;
#pragma unroll
    for (int k = 0; k < 2; k++) {
      const f32x2 sp = posxy + m[k];
      const float d = k == 0 ? den.x : den.y, r = k == 0 ? r1.x : r1.y;
      const f32x2 nd = {-d, -d}, rr = {r, r};
      const f32x2 q0 = sp * rr;
      const f32x2 e1 = __builtin_elementwise_fma(nd, q0, sp);
      const f32x2 q1 = __builtin_elementwise_fma(e1, rr, q0);
      const f32x2 e2 = __builtin_elementwise_fma(nd, q1, sp);
      f32x2 qv = __builtin_elementwise_fma(e2, rr, q1);
      if (kExact) {
        if (!(mag_ok && fabsf(d) > 0x1p-60f)) qv = f32x2{sp.x / d, sp.y / d};
      }
      const f32x2 t = (qv * fxy + cxy) + 0.49999997f;  // round_pix's addend, packed
      const int ix = floor_pix(t.x);
      const int iy = floor_pix(t.y);
      inb[k][g] = in_range && (unsigned)ix < (unsigned)p.W && (unsigned)iy < (unsigned)p.H;
      off[k][g] = __umul24((unsigned)iy, (unsigned)p.W) + (unsigned)ix;  // see group_coords
    }
  }
  return min_den;
}

// Marches kRays rays of one pixel together; hit[k] = pixel index of ray k's hit or -1.
// The reference walks j = start..step-1 per ray and stops at the first sample that leaves the image
// or hits (forward.cu:691-714).  ~98 % of the rays of a real frame run all their steps, so:
//   * steps are evaluated in groups of kGroup: the coordinates of the whole group (times kRays) are
//     computed and their z-plane gathers issued together -- memory-level parallelism instead of one
//     dependent L2 round trip per step;
//   * the group is then resolved IN ORDER with per-lane selects, not branches (`open` = ray still
//     marching), which is exactly the sequential outcome; the only branches left are wave-uniform
//     (all rays of the wave resolved; the rare IEEE-division re-march, decided once per ray pair), so the
//     scalar unit is not spent on exec-mask bookkeeping.
template <bool kPow2, int kGroup, int kRays, bool kExact>
__device__ __forceinline__ bool march_impl(const GiParams& p, v3 pos, float a, const v3* sv, float cx, float cy,
                                           __amdgpu_buffer_rsrc_t pos_z, bool mag_ok, int* hit) {
  bool open[kRays];
#pragma unroll
  for (int k = 0; k < kRays; k++) { open[k] = true; hit[k] = -1; }
  float min_den = __builtin_inff();
  for (int j0 = p.start; j0 < p.step; j0 += kGroup) {
    unsigned off[kRays][kGroup];
    float zv[kRays][kGroup];
    bool inb[kRays][kGroup];
    f32x2 hi2[kGroup], lo2[kGroup];           // kRays == 2: depth-test bounds of the pair
    float spzv[kRays == 2 ? 1 : kRays][kGroup];  // otherwise: the sample z
    if constexpr (kRays == 2)
      min_den = fminf(min_den, group_coords2<kPow2, kGroup, kExact>(p, pos, a, sv, cx, cy, mag_ok, j0, off, inb, hi2, lo2));
    else
      min_den = fminf(min_den, group_coords<kPow2, kGroup, kRays, kExact>(p, pos, a, sv, cx, cy, mag_ok, j0, off, inb, spzv));
    {
      constexpr int kN = kRays * kGroup;
      unsigned in[kN];
      float zn[kN];
#pragma unroll
      for (int g = 0; g < kGroup; g++)
#pragma unroll
        for (int k = 0; k < kRays; k++) in[g * kRays + k] = off[k][g];
      gather_idx<kN>(zn, in, pos_z);
#pragma unroll
      for (int g = 0; g < kGroup; g++)
#pragma unroll
        for (int k = 0; k < kRays; k++) zv[k][g] = zn[g * kRays + k];
    }
    bool any_open = false;
#pragma unroll
    for (int k = 0; k < kRays; k++) {
#pragma unroll
      for (int g = 0; g < kGroup; g++) {
        float hi, lo;
        if constexpr (kRays == 2) {
          hi = k == 0 ? hi2[g].x : hi2[g].y;
          lo = k == 0 ? lo2[g].x : lo2[g].y;
        } else {
          hi = spzv[k][g] + p.bias;
          lo = spzv[k][g] - p.thick;
        }
        const bool h = inb[k][g] && (zv[k][g] <= hi) && (zv[k][g] >= lo);
        hit[k] = (open[k] && h) ? (int)off[k][g] : hit[k];
        open[k] = open[k] && inb[k][g] && !h;
      }
      any_open = any_open || open[k];
    }
    if (!__any(any_open)) break;
  }
  return !(mag_ok && min_den > 0x1p-60f);  // this lane needed an IEEE division somewhere
}

// The fast pass assumes no sample of the pixel needs the operand pre-scaling of an IEEE division and
// reports per lane whether that held; if any lane of the wave says no (never, on real frames) the
// rays are marched again with the per-lane exact selection -- two separate code paths, so the common
// one carries neither the branches nor the registers of the rare one.
template <bool kPow2, int kGroup, int kRays>
__device__ __forceinline__ void march(const GiParams& p, v3 pos, float a, const v3* sv, float cx, float cy,
                                      __amdgpu_buffer_rsrc_t pos_z, bool mag_ok, unsigned sv_min_bits, int* hit) {
  bool bad = march_impl<kPow2, kGroup, kRays, false>(p, pos, a, sv, cx, cy, pos_z, mag_ok, hit);
  if (kPow2) {
    // folding 1/step into j is exact unless a product of the chain is subnormal: every non-zero component of the
    // sample vectors must stay above sv_min (= 2^-120 / the smallest cumulative factor of the chain; a zero
    // component gives exact zeros either way).  As unsigned integers: (|bits| - 1) >= (sv_min_bits - 1).
    unsigned lowest = 0xffffffffu;
#pragma unroll
    for (int k = 0; k < kRays; k++)
      lowest = min(lowest, min(min((__float_as_uint(sv[k].x) & 0x7fffffffu) - 1u, (__float_as_uint(sv[k].y) & 0x7fffffffu) - 1u),
                               (__float_as_uint(sv[k].z) & 0x7fffffffu) - 1u));
    bad = bad || lowest < sv_min_bits - 1u;
  }
  if (__builtin_expect(__any(bad), 0)) march_impl<kPow2, kGroup, kRays, true>(p, pos, a, sv, cx, cy, pos_z, mag_ok, hit);
}

struct Tbn { v3 t, b, n; };
__device__ __forceinline__ Tbn make_tbn(v3 normal_un) {
  Tbn r;
  r.n = normalize3(normal_un);
  const v3 up = {0.0f, 1.0f, 0.0f};
  const float rndot = dot3(up, r.n);
  const v3 untangent = {up.x - r.n.x * rndot, up.y - r.n.y * rndot, up.z - r.n.z * rndot};
  r.t = normalize3(untangent);
  r.b = normalize3(cross3(r.n, r.t));
  return r;
}
// transformVec3x3(ts, TBN) with TBN rows (t, b, n): auxiliary.h:90-98
__device__ __forceinline__ v3 tbn_apply(const Tbn& m, float x, float y, float z) {
  return {m.t.x * x + m.b.x * y + m.n.x * z, m.t.y * x + m.b.y * y + m.n.y * z,
          m.t.z * x + m.b.z * y + m.n.z * z};
}
// |sample position| <= |pos| + |sv| * (j/step) * a^2 * radius with |sv| <= sqrt(3): when this bound
// is far below 2^60 for the pixel, no step of any ray needs the operand pre-scaling of IEEE division.
__device__ __forceinline__ bool gi_mag_ok(v3 pos, float a, float radius) {
  const float bound = fmaxf(fmaxf(fabsf(pos.x), fabsf(pos.y)), fabsf(pos.z)) + 2.0f * fabsf(a * a * radius) + 1.0f;
  return bound < 0x1p59f;  // false for NaN / inf
}

// Smallest non-zero |sample-vector component| for which folding 1/step into j is exact (see group_coords): the
// chain multiplies by j/step >= 1/step, a, a, radius; its smallest cumulative factor must keep the product
// above 2^-120.  Returned as fp32 bits (positive floats order like unsigned integers); NaN / zero factors give
// +inf bits, i.e. "never exact" -> the exact path.
__device__ __forceinline__ unsigned gi_sv_min_bits(float a, float radius, float inv_step) {
  const float aa = fabsf(a), a2 = aa * aa;
  const float lo = fminf(fminf(1.0f, aa), fminf(a2, a2 * fabsf(radius))) * inv_step;
  const float sv_min = 0x1p-120f / lo;  // lo == 0 or NaN -> inf / NaN
  return (sv_min == sv_min) ? __float_as_uint(sv_min) : 0x7f800000u;
}

// Every sample direction contains t * ts.x, so a tangent that is NaN in all three components
// (empty pixel: N = 0 -> NaN normal; or N parallel to `up`) makes every sample position NaN:
// the projected pixel is (0, 0), the depth test against NaN is false, no ray ever hits.  Such
// pixels -- the whole background of an object-centric frame -- skip the march with the same result.
__device__ __forceinline__ bool tbn_never_hits(const Tbn& m) {
  return (m.t.x != m.t.x) && (m.t.y != m.t.y) && (m.t.z != m.t.z);
}

// ------------------------------------------------------------------------------------------
// The projective march (GIGS_GI_MARCH=proj, the default)
// ------------------------------------------------------------------------------------------
// The exact march above reproduces the oracle's pixel choice bit for bit and pays for it with ~31 VALU
// instructions per ray-step.  north_star's bar for the fp planes is 1e-4 mean per-pixel L1, and the reference's
// own binary is an FMA-contracted compilation of the same lines (nvcc -fmad=true), so its projected coordinates
// already differ from the contraction-free oracle in the last place.  The projective march spends that tolerance:
// per sample the numerators (pos.xy*f + fj*Bxy) and the denominator (pos.z + 1e-7 + fj*Bz) with fj = j/step and
// B the per-ray step vector, one raw (1-ulp) v_rcp_f32, t = n*r + (c + 0.5): 3 packed FMAs + rcp.
// The depth test z in [spz - thick, spz + bias] is evaluated as |z - (den + cm)| <= hh with
// cm = (bias - thick)/2 - 1e-7, hh = (bias + thick)/2 (same interval, different rounding of its ends).
// The march's control flow is kept: in-order resolution, break on leaving the image, first hit wins.
// tools/gi_variants.py measures it against the exact march (= the oracle, bit for bit) on the C2 view and the GI test
// scenes; DESIGN.md section 5 holds the table and the choice of default.  (Three intermediate formulations were measured
// in round 2, profiles/r02/gi_variants.json, and removed: see the git history.)
struct FastPix {
  f32x2 Axy;      // pos.xy * (fx, fy)
  float Dz;       // pos.z + 1e-7
  f32x2 cxy;      // (cx, cy) + round_pix's addend
  float cm, hh;
};

__device__ __forceinline__ int cvt_flr(float t) {  // (int)floor(t), saturating, NaN -> 0: one VOP1 instruction
  int r;
  asm("v_cvt_flr_i32_f32 %0, %1" : "=v"(r) : "v"(t));
  return r;
}

template <int kGroup>
__device__ __forceinline__ void march2_fast(const GiParams& p, const FastPix& c, const f32x2* Bxy, f32x2 Bz2,
                                            __amdgpu_buffer_rsrc_t pos_z, int* hit) {
  bool open[2] = {true, true};
  hit[0] = hit[1] = -1;
  const f32x2 Dz2 = {c.Dz, c.Dz};
  for (int j0 = p.start; j0 < p.step; j0 += kGroup) {
    unsigned off[2][kGroup];
    bool inb[2][kGroup];
    f32x2 ta[kGroup];  // middle of the hit interval
#pragma unroll
    for (int g = 0; g < kGroup; g++) {
      const float fj = p.fjt[j0 - p.start + g];  // j / step
      const f32x2 fj2 = {fj, fj};
      const bool in_range = (j0 + g) < p.step;
      const f32x2 den = __builtin_elementwise_fma(Bz2, fj2, Dz2);
      ta[g] = den + c.cm;
      const f32x2 r = {__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)};
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const float rk = k == 0 ? r.x : r.y;
        const f32x2 rr = {rk, rk};
        const f32x2 n = __builtin_elementwise_fma(Bxy[k], fj2, c.Axy);
        const f32x2 t = __builtin_elementwise_fma(n, rr, c.cxy);
        const int ix = cvt_flr(t.x);
        const int iy = cvt_flr(t.y);
        inb[k][g] = in_range && (unsigned)ix < (unsigned)p.W && (unsigned)iy < (unsigned)p.H;
        off[k][g] = __umul24((unsigned)iy, (unsigned)p.W) + (unsigned)ix;
      }
    }
    float zn[2 * kGroup];
    {
      unsigned in[2 * kGroup];
#pragma unroll
      for (int g = 0; g < kGroup; g++) { in[2 * g] = off[0][g]; in[2 * g + 1] = off[1][g]; }
      gather_idx<2 * kGroup>(zn, in, pos_z);
    }
    bool any_open = false;
#pragma unroll
    for (int k = 0; k < 2; k++) {
#pragma unroll
      for (int g = 0; g < kGroup; g++) {
        const float z = zn[2 * g + k];
        const bool h = inb[k][g] && fabsf(z - (k == 0 ? ta[g].x : ta[g].y)) <= c.hh;
        hit[k] = (open[k] && h) ? (int)off[k][g] : hit[k];
        open[k] = open[k] && inb[k][g] && !h;
      }
      any_open = any_open || open[k];
    }
    if (!__any(any_open)) break;
  }
}

// Conservative certification in front of the projective march.  The z plane's {non-zero minimum, max(maximum, 0)} over
// square blocks of 2^cert_shift pixels (gi_minmax_kernel) sit in LDS, with a border of "never certify" entries around
// the image and on blocks the image only partly covers.  A sample is projected in BLOCK units first (the per-pixel
// constants are pre-scaled by the exact factor 2^-shift); if its hit interval, widened by 2^-16 relative + 1e-6, lies
// entirely above the block's maximum, or entirely below its non-zero minimum and above zero (empty pixels hold 0), then
// whichever pixel of that -- fully in-image -- block the sample selects, the reference's test fails by a margin far above
// its rounding error: the sample neither hits nor leaves the image, the ray simply stays open, and nothing else has to
// be computed for it.  Only when some lane of the wave is NOT certified for a sample does the wave run the exact part
// (pixel coordinates = block coordinates * 2^shift exactly, bounds test, gather, depth test).  ~92 % of the wave-samples
// of the bench view skip it (tools/gi_cert_rate.py); every ray's outcome, hence every output bit, is unchanged
// (tests/test_gpu_parity.py::test_gi_certification_is_exact).
struct CertPix {
  f32x2 Axy, cxy;  // FastPix::Axy / cxy scaled by 2^-shift
  float scale;     // 2^shift
  int bw, bh;      // blocks per row / column of the image (the table has one more column / row: the never-certify border)
};

typedef unsigned long long u64;

// certification thresholds on the sample's denominator den = spz + 1e-7 (the hit interval is [den + cm - hh, den + cm + hh]):
//   lo = (den + cm) * (1 - 2^-16) - (hh + 1e-6) > block maximum      <=>  den > t_hi   (stored per block)
//   hi = (den + cm) * (1 + 2^-16) + (hh + 1e-6) < block non-zero min <=>  den < t_lo   (stored per block)
//   lo > 0 (empty pixels hold z = 0)                                  <=>  den > d0     (a launch constant)
// each rounded away from certification (gi_minmax_kernel).
struct CertK { float lo_k, hi_k, d0; };
__host__ __device__ __forceinline__ CertK cert_consts(float bias, float thick) {
  const float cm = 0.5f * (bias - thick) - 0.0000001f, hh = 0.5f * (bias + thick);
  CertK k;
  k.lo_k = cm * (1.0f - 0x1p-16f) - hh - 1e-6f;
  k.hi_k = cm * (1.0f + 0x1p-16f) + hh + 1e-6f;
  const float d = -k.lo_k / (1.0f - 0x1p-16f);
  k.d0 = d + fabsf(d) * 0x1p-20f + 1e-30f;
  return k;
}

// kTabOff: LDS byte address of the table (the kernels' dynamic LDS starts right after their static arrays; checked at
// kernel entry).  The lookups are written as instructions because the compiler adds the -- constant -- base with a
// v_add per lookup instead of using the ds_read offset field.
template <int kGroup, int kTabOff>
__device__ __forceinline__ void march2_cert(const GiParams& p, const FastPix& c, const CertPix& cp, const f32x2* Bxy16,
                                            f32x2 Bz2, __amdgpu_buffer_rsrc_t pos_z, int* hit) {
  // Lane predicates are kept as 64-bit wave masks in SGPRs (ballots of single compares, combined with scalar logic,
  // turned back into a lane predicate only where a select needs one): written with per-lane bools the compiler moves
  // them through VGPRs (v_cndmask 0/1 + v_cmp_ne per use) -- a third of the march's vector instructions.
  u64 open_m[2];
  open_m[0] = open_m[1] = __builtin_amdgcn_ballot_w64(true);  // the lanes that march (EXEC)
  hit[0] = hit[1] = -1;
  const f32x2 Dz2 = {c.Dz, c.Dz};
  const unsigned row8 = (unsigned)(cp.bw + 1) * 8u;
  // table entry of block (bx, by) at byte by * row8 + bx * 8; column bw / row bh never certify
  // block indices as unsigned: a negative one is a huge one, and both clamp to bw / bh (one v_min_u32 per coordinate)
  unsigned bw_v = (unsigned)cp.bw, bh_v = (unsigned)cp.bh;
  asm("" : "+v"(bw_v), "+v"(bh_v));  // in VGPRs: the VOP2 form with two VGPR operands issues faster than an SGPR-source one
  // den > d0 for every sample of a ray <=> at both of its ends (den is a correctly rounded, hence monotone, function of j):
  // decided once per ray instead of once per sample
  u64 pos[2];
  {
    const float f0 = p.fjt[0], f1 = p.fjt[p.step - 1 - p.start];
    const f32x2 da = __builtin_elementwise_fma(Bz2, f32x2{f0, f0}, Dz2), db = __builtin_elementwise_fma(Bz2, f32x2{f1, f1}, Dz2);
    pos[0] = __builtin_amdgcn_ballot_w64(da.x > p.cert_d0) & __builtin_amdgcn_ballot_w64(db.x > p.cert_d0);
    pos[1] = __builtin_amdgcn_ballot_w64(da.y > p.cert_d0) & __builtin_amdgcn_ballot_w64(db.y > p.cert_d0);
  }
  for (int j0 = p.start; j0 < p.step; j0 += kGroup) {
    f32x2 tb[2][kGroup];  // sample position in block units (+ the rounding addend, scaled)
    f32x2 dn[kGroup];
    f32x2 th[2][kGroup];  // {t_lo, t_hi} of the sample's block
    u64 cert[2][kGroup];
    // the group's j / step factors, in SGPRs before the first lookup is issued: a scalar load between the lookups would
    // bring a wait on the counter they share, i.e. on the lookups
    float fjs[kGroup];
#pragma unroll
    for (int g = 0; g < kGroup; g++) fjs[g] = p.fjc[j0 - p.start + g];
    asm volatile("" : "+s"(fjs[0]), "+s"(fjs[1]), "+s"(fjs[2]), "+s"(fjs[3]));
    // phase A: every sample of the group up to its table lookup; no branches
#pragma unroll
    for (int g = 0; g < kGroup; g++) {
      const float fj = fjs[g];  // j / step
      const f32x2 fj2 = {fj, fj};
      const f32x2 den = __builtin_elementwise_fma(Bz2, fj2, Dz2);
      dn[g] = den;
      const f32x2 r = {__builtin_amdgcn_rcpf(den.x), __builtin_amdgcn_rcpf(den.y)};
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const float rk = k == 0 ? r.x : r.y;
        const f32x2 n = __builtin_elementwise_fma(Bxy16[k], fj2, cp.Axy);
        tb[k][g] = __builtin_elementwise_fma(n, f32x2{rk, rk}, cp.cxy);
        const unsigned bx = min((unsigned)cvt_flr(tb[k][g].x), bw_v);
        const unsigned by = min((unsigned)cvt_flr(tb[k][g].y), bh_v);
        const unsigned toff = __umul24(by, row8) + (bx << 3);
        asm volatile("ds_read_b64 %0, %1 offset:%2" : "=v"(th[k][g]) : "v"(toff), "n"(kTabOff));
      }
    }
    // the lookups above are invisible to the compiler's wait-count bookkeeping: wait for them here (operands tie the order)
    static_assert(kGroup == 4, "the wait below lists the lookups of a group of four");
    asm volatile("s_waitcnt lgkmcnt(0)"
                 : "+v"(th[0][0]), "+v"(th[0][1]), "+v"(th[0][2]), "+v"(th[0][3]), "+v"(th[1][0]), "+v"(th[1][1]), "+v"(th[1][2]),
                   "+v"(th[1][3]));
#pragma unroll
    for (int g = 0; g < kGroup; g++) {
#pragma unroll
      for (int k = 0; k < 2; k++) {
        const float dk = k == 0 ? dn[g].x : dn[g].y;
        const u64 above = __builtin_amdgcn_ballot_w64(dk > th[k][g].y);
        const u64 below = __builtin_amdgcn_ballot_w64(dk < th[k][g].x);
        cert[k][g] = above | (below & pos[k]);
      }
    }
    // phase B: the exact part for the samples some lane of the wave still needs (~8 % of them).  A group that runs past the
    // last step repeats the last sample (fjc): repeating a sample changes nothing -- a ray it closed is closed, one it left
    // open it leaves open again -- so there is no per-sample range test.  Two stages, so that a group with several such
    // samples pays ONE round trip to the z plane instead of one per sample: every lookup that MAY be needed (judged with the
    // rays' state at the start of the group: a ray can only close) is requested, then the samples are resolved in order --
    // each ray's own (the two rays are independent) -- with the state as it evolves.
    u64 maybe[2][kGroup], any = 0ull;
#pragma unroll
    for (int k = 0; k < 2; k++)
#pragma unroll
      for (int g = 0; g < kGroup; g++) { maybe[k][g] = open_m[k] & ~cert[k][g]; any |= maybe[k][g]; }
    if (any != 0ull) {
      float z[2][kGroup];
      unsigned off[2][kGroup];
      u64 inb[2][kGroup];
#pragma unroll
      for (int k = 0; k < 2; k++)
#pragma unroll
        for (int g = 0; g < kGroup; g++) {
          z[k][g] = 0.0f; off[k][g] = 0u; inb[k][g] = 0ull;
          if (maybe[k][g] != 0ull) {
            const f32x2 t = tb[k][g] * cp.scale;  // exact: the pixel coordinates the uncertified march computes
            const int ix = cvt_flr(t.x);
            const int iy = cvt_flr(t.y);
            inb[k][g] = __builtin_amdgcn_ballot_w64((unsigned)ix < (unsigned)p.W) & __builtin_amdgcn_ballot_w64((unsigned)iy < (unsigned)p.H);
            off[k][g] = __umul24((unsigned)iy, (unsigned)p.W) + (unsigned)ix;
            z[k][g] = gather_idx_issue(__builtin_amdgcn_inverse_ballot_w64(maybe[k][g] & inb[k][g]) ? off[k][g] : 0xffffffffu, pos_z);
          }
        }
      static_assert(kGroup == 4, "the wait below lists the lookups of a group of four");
      asm volatile("s_waitcnt vmcnt(0)"
                   : "+v"(z[0][0]), "+v"(z[0][1]), "+v"(z[0][2]), "+v"(z[0][3]), "+v"(z[1][0]), "+v"(z[1][1]), "+v"(z[1][2]), "+v"(z[1][3]));
#pragma unroll
      for (int k = 0; k < 2; k++)
#pragma unroll
        for (int g = 0; g < kGroup; g++) {
          const u64 need = open_m[k] & maybe[k][g];  // the ray may have closed at an earlier sample of this group
          if (need != 0ull) {
            const u64 look = need & inb[k][g];
            const float mid = (k == 0 ? dn[g].x : dn[g].y) + c.cm;
            const u64 h = look & __builtin_amdgcn_ballot_w64(fabsf(z[k][g] - mid) <= c.hh);
            hit[k] = __builtin_amdgcn_inverse_ballot_w64(h) ? (int)off[k][g] : hit[k];
            open_m[k] &= ~((need & ~inb[k][g]) | h);  // left the image, or hit: the ray is closed
          }
        }
    }
    if ((open_m[0] | open_m[1]) == 0ull) break;
  }
}

// per-pixel constants of the projective march and the per-ray vectors
__device__ __forceinline__ FastPix make_fast(const GiParams& p, v3 pos, float cx, float cy) {
  FastPix c;
  c.cxy = f32x2{cx + 0.49999997f, cy + 0.49999997f};
  c.cm = 0.5f * (p.bias - p.thick) - 0.0000001f;
  c.hh = 0.5f * (p.bias + p.thick);
  c.Axy = f32x2{pos.x * p.fx, pos.y * p.fy};
  c.Dz = pos.z + 0.0000001f;
  return c;
}
// rows of the tangent frame pre-scaled so that B = M * ts is the per-ray step vector (times j/step per sample)
struct FastTbn { v3 mx, my, mz; };
__device__ __forceinline__ CertPix make_cert(const GiParams& p, const FastPix& c, float inv_scale) {
  CertPix cp;
  cp.Axy = c.Axy * inv_scale;  // exact power-of-two scalings
  cp.cxy = c.cxy * inv_scale;
  cp.scale = 1.0f / inv_scale;
  cp.bw = p.cert_w;
  cp.bh = p.cert_h;
  return cp;
}
// xy_scale = 2^-cert_shift when the march runs in block units (exact), else 1
__device__ __forceinline__ FastTbn make_fast_tbn(const GiParams& p, const Tbn& m, float a, float xy_scale = 1.0f) {
  const float s = a * a * p.radius;
  const float sx = (s * p.fx) * xy_scale, sy = (s * p.fy) * xy_scale;
  FastTbn r;
  r.mx = {m.t.x * sx, m.b.x * sx, m.n.x * sx};
  r.my = {m.t.y * sy, m.b.y * sy, m.n.y * sy};
  r.mz = {m.t.z * s, m.b.z * s, m.n.z * s};
  return r;
}
__device__ __forceinline__ void fast_ray(const FastTbn& ft, float4 ra, f32x2& bxy, float& bz) {
  const float bx = __builtin_fmaf(ft.mx.z, ra.z, __builtin_fmaf(ft.mx.y, ra.y, ft.mx.x * ra.x));
  const float by = __builtin_fmaf(ft.my.z, ra.z, __builtin_fmaf(ft.my.y, ra.y, ft.my.x * ra.x));
  bz = __builtin_fmaf(ft.mz.z, ra.z, __builtin_fmaf(ft.mz.y, ra.y, ft.mz.x * ra.x));
  bxy = f32x2{bx, by};
}

// The hit list of the indirect-light march (frozen-geometry reuse, pipeline.GeometryCache): WHICH pixel every ray of
// every pixel hits depends on normals and positions only -- not on the radiance that is gathered there -- so a view whose
// geometry does not change marches once and afterwards only gathers (ssr_apply_kernel).  kHits = 1 counts the hits of each
// (pixel, wave) -- the wave's rays are marched in a fixed order, so its hits form a sequence --, kHits = 2 writes them as
// (hit pixel, ray index) at the positions an exclusive prefix of the counts assigns.  Both also produce the normal outputs.
struct SsrHits {
  unsigned* counts;         // kHits 1: [4 N], entry 4 * pixel + wave
  const unsigned* offsets;  // kHits 2: [4 N + 1] exclusive prefix of the counts
  uint2* entries;           // kHits 2: {hit pixel, ray index}
  unsigned capacity;        // entries beyond it are dropped (the caller compares offsets[4 N] with it and repeats)
};

// the part of SSRCUDA behind the march (forward.cu:832-909; fresnelSchlick ssr.h:13-16): shared by the march and the gather
__device__ __forceinline__ void ssr_finish(v3 diffuse, const Tbn& tbn, v3 pos, size_t pix_id, size_t HW, int nrays_total,
                                           const float* __restrict__ albedo_map, const float* __restrict__ metallic_map,
                                           const float* __restrict__ F0_map, float* __restrict__ color, float* __restrict__ abd) {
  const v3 N = tbn.n;
  const v3 alb = {albedo_map[pix_id], albedo_map[HW + pix_id], albedo_map[2 * HW + pix_id]};
  const v3 F0 = {F0_map[pix_id], F0_map[HW + pix_id], F0_map[2 * HW + pix_id]};
  const float metallic = metallic_map[pix_id];
  const v3 V = normalize3({-pos.x, -pos.y, -pos.z});
  // fresnelSchlick (ssr.h:13-16): pow evaluated in double
  const float cosTheta = fmaxf(dot3(N, V), (float)0.0000001);
  const float pw = (float)pow((double)fminf(fmaxf((float)(1.0 - (double)cosTheta), (float)0.000001), 1.0f), 5.0);
  const v3 F = {F0.x + (1.0f - F0.x) * pw, F0.y + (1.0f - F0.y) * pw, F0.z + (1.0f - F0.z) * pw};
  v3 kD = {(float)(1.0 - (double)F.x), (float)(1.0 - (double)F.y), (float)(1.0 - (double)F.z)};
  kD.x = (float)((double)kD.x * (1.0 - (double)metallic));
  kD.y = (float)((double)kD.y * (1.0 - (double)metallic));
  kD.z = (float)((double)kD.z * (1.0 - (double)metallic));
  const float nrSamples = (float)nrays_total;  // += 1 per ray in fp32 is exact below 2^24
  v3 gd;
  if (nrSamples > 0.0f) {
    gd.x = (float)((double)(kPiF * diffuse.x) * (1.0 / (double)nrSamples) * (double)kD.x);
    gd.y = (float)((double)(kPiF * diffuse.y) * (1.0 / (double)nrSamples) * (double)kD.y);
    gd.z = (float)((double)(kPiF * diffuse.z) * (1.0 / (double)nrSamples) * (double)kD.z);
    diffuse = {gd.x * alb.x, gd.y * alb.y, gd.z * alb.z};
  } else {
    diffuse = {(float)0.0000001, (float)0.0000001, (float)0.0000001};
    gd = diffuse;
  }
  color[pix_id] = diffuse.x;
  color[HW + pix_id] = diffuse.y;
  color[2 * HW + pix_id] = diffuse.z;
  abd[pix_id] = gd.x;
  abd[HW + pix_id] = gd.y;
  abd[2 * HW + pix_id] = gd.z;
}

}  // namespace gigs
