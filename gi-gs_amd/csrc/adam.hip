// adam.hip -- SURVEY 8(f) rank 1: the Adam step.
//
// torch.optim.Adam as configured at scene/gaussian_model.py:346 (betas (0.9, 0.999), eps 1e-15, no weight decay, no
// amsgrad), which the reference runs once per parameter group over ten groups (scene/gaussian_model.py:325-346).  Here
// the update of up to 16 groups is one launch: HBM-streaming, 28 B per parameter.  The entry points form a chain
// (gigs_adam_step -> _dyn -> _watch -> _guarded), each adding one argument to the one before; all four are ABI.
#include <cmath>
#include <cstring>

#include "gigs_internal.h"

namespace gigs {

constexpr int kAdamMaxGroups = 16;
constexpr int kAdamChunk = 2048;  // elements per workgroup: 256 lanes x 2 x float4
struct AdamGroups {
  float* param[kAdamMaxGroups];
  float* grad[kAdamMaxGroups];
  float* exp_avg[kAdamMaxGroups];
  float* exp_avg_sq[kAdamMaxGroups];
  long long n[kAdamMaxGroups];
  unsigned first_chunk[kAdamMaxGroups + 1];
  float step_size[kAdamMaxGroups];      // lr / (1 - beta1^t)
  float bc2_sqrt[kAdamMaxGroups];       // sqrt(1 - beta2^t)
  int count;
  // hipGraph-capturable form: the two per-step scalars of group k are read from device memory, dyn[2 * (dyn_base + k)]
  // = {step_size, bc2_sqrt}, which the host refreshes before every replay (NULL: the by-value members above)
  const float* dyn;
  int dyn_base;
  // gigs_adam_step_watch: bit k set = group k of this launch is watched; *changed |= 1 when one of its parameters changes
  unsigned watch_mask;
  unsigned* changed;
  // gigs_adam_step_guarded: the launch is a no-op while *guard != 0 (a violated gradient declaration: gigs_ctx_set_materials_only)
  const unsigned* guard;
};

struct AdamConsts { float b2, omb1, omb2, eps; };  // beta2, 1 - beta1, 1 - beta2 (rounded from double as torch does), eps
__device__ __forceinline__ void adam_one(float& p, float g, float& m, float& v, const AdamConsts& k,
                                         float step_size, float bc2_sqrt) {
  const float eps = k.eps;
  m = m + k.omb1 * (g - m);                 // exp_avg.lerp_(grad, 1 - beta1)
  v = v * k.b2 + k.omb2 * (g * g);          // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
  const float denom = sqrtf(v) / bc2_sqrt + eps;
  p = p - step_size * (m / denom);          // param.addcdiv_(exp_avg, denom, value=-step_size)
}

typedef float adam_f4 __attribute__((ext_vector_type(4)));
// kStream: the three arrays a step reads and rewrites are touched once per step and are far larger than any cache: loads
// and stores carry the non-temporal hint (they do not displace what the next kernels of the iteration will read)
template <bool kStream>
__device__ __forceinline__ float4 adam_ld4(const float* p) {
  if constexpr (kStream) {
    const adam_f4 v = __builtin_nontemporal_load(reinterpret_cast<const adam_f4*>(p));
    return make_float4(v.x, v.y, v.z, v.w);
  } else {
    return *reinterpret_cast<const float4*>(p);
  }
}
template <bool kStream>
__device__ __forceinline__ void adam_st4(float* p, float4 v) {
  if constexpr (kStream) {
    adam_f4 w = {v.x, v.y, v.z, v.w};
    __builtin_nontemporal_store(w, reinterpret_cast<adam_f4*>(p));
  } else {
    *reinterpret_cast<float4*>(p) = v;
  }
}

template <bool kStream>
__global__ void __launch_bounds__(256)
adam_kernel(AdamGroups G, AdamConsts K, int zero_grad) {
  if (G.guard && *G.guard != 0u) return;  // uniform: nothing of this update is computed from gradients that were declared wrongly
  int gi = 0;
  while (gi + 1 < G.count && blockIdx.x >= G.first_chunk[gi + 1]) gi++;
  const long long n = G.n[gi];
  const long long base = (long long)(blockIdx.x - G.first_chunk[gi]) * kAdamChunk;
  float* __restrict__ P = G.param[gi];
  float* __restrict__ Gr = G.grad[gi];
  float* __restrict__ M = G.exp_avg[gi];
  float* __restrict__ V = G.exp_avg_sq[gi];
  const float ss = G.dyn ? G.dyn[2 * (G.dyn_base + gi)] : G.step_size[gi];
  const float bs = G.dyn ? G.dyn[2 * (G.dyn_base + gi) + 1] : G.bc2_sqrt[gi];
  // Gr == NULL: the group's gradient is an exact zero the caller did not materialise -- the same arithmetic with g = 0
  const bool vec = ((((uintptr_t)P | (uintptr_t)Gr | (uintptr_t)M | (uintptr_t)V) & 15) == 0) && base + kAdamChunk <= n;
  const bool watched = (G.watch_mask >> gi) & 1u;
  bool moved = false;
  if (vec) {
#pragma unroll
    for (int r = 0; r < 2; r++) {
      const long long i = base + (long long)(r * 256 + threadIdx.x) * 4;
      float4 p = adam_ld4<kStream>(P + i), m = adam_ld4<kStream>(M + i);
      float4 v = adam_ld4<kStream>(V + i);
      const float4 g = Gr ? *reinterpret_cast<const float4*>(Gr + i) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      const float4 p0 = p;
      adam_one(p.x, g.x, m.x, v.x, K, ss, bs);
      adam_one(p.y, g.y, m.y, v.y, K, ss, bs);
      adam_one(p.z, g.z, m.z, v.z, K, ss, bs);
      adam_one(p.w, g.w, m.w, v.w, K, ss, bs);
      moved |= (__float_as_uint(p.x) != __float_as_uint(p0.x)) | (__float_as_uint(p.y) != __float_as_uint(p0.y)) |
               (__float_as_uint(p.z) != __float_as_uint(p0.z)) | (__float_as_uint(p.w) != __float_as_uint(p0.w));
      adam_st4<kStream>(P + i, p);
      adam_st4<kStream>(M + i, m);
      adam_st4<kStream>(V + i, v);
      if (zero_grad && Gr) *reinterpret_cast<float4*>(Gr + i) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    }
  } else {
    for (int r = 0; r < kAdamChunk / 256; r++) {
      const long long i = base + r * 256 + threadIdx.x;
      if (i >= n) break;
      float p = P[i], m = M[i], v = V[i];
      const float p0 = p;
      adam_one(p, Gr ? Gr[i] : 0.0f, m, v, K, ss, bs);
      moved |= __float_as_uint(p) != __float_as_uint(p0);
      P[i] = p; M[i] = m; V[i] = v;
      if (zero_grad && Gr) Gr[i] = 0.0f;
    }
  }
  // frozen geometry: no wave of a watched group sees a change, no atomic is issued
  if (watched && G.changed && __any(moved) && (threadIdx.x & 63) == 0) atomicOr(G.changed, 1u);
}

}  // namespace gigs

extern "C" {

int gigs_adam_step(int n_groups, const gigs_adam_group* groups, double beta1, double beta2, double eps, int zero_grad,
                   void* stream) {
  return gigs_adam_step_dyn(n_groups, groups, beta1, beta2, eps, zero_grad, nullptr, stream);
}

void gigs_adam_scalars(double lr, int step, double beta1, double beta2, float* out2) {
  // torch/optim/adam.py (_single_tensor_adam): python-float bias corrections, then fp32 tensor ops
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  out2[0] = (float)(lr / bc1);
  out2[1] = (float)sqrt(bc2);
}

int gigs_adam_step_dyn(int n_groups, const gigs_adam_group* groups, double beta1, double beta2, double eps, int zero_grad,
                       const float* dyn, void* stream) {
  return gigs_adam_step_watch(n_groups, groups, beta1, beta2, eps, zero_grad, dyn, nullptr, nullptr, stream);
}

int gigs_adam_step_watch(int n_groups, const gigs_adam_group* groups, double beta1, double beta2, double eps, int zero_grad,
                         const float* dyn, const unsigned char* watch, unsigned* changed, void* stream) {
  return gigs_adam_step_guarded(n_groups, groups, beta1, beta2, eps, zero_grad, dyn, watch, changed, nullptr, stream);
}

int gigs_adam_step_guarded(int n_groups, const gigs_adam_group* groups, double beta1, double beta2, double eps, int zero_grad,
                           const float* dyn, const unsigned char* watch, unsigned* changed, const unsigned* guard, void* stream) {
  if (n_groups < 0 || (n_groups > 0 && !groups)) return gigs_internal_fail(GIGS_ERR_INVALID, "adam_step: bad argument");
  hipStream_t s = (hipStream_t)stream;
  gigs::StageTimer timer(gigs::Stage::kAdam, stream);
  int done = 0;
  while (done < n_groups) {
    gigs::AdamGroups G;
    memset(&G, 0, sizeof(G));
    unsigned chunks = 0;
    int k = 0;
    for (; done < n_groups && k < gigs::kAdamMaxGroups; done++) {
      const gigs_adam_group& g = groups[done];
      if (g.n < 0 || (!dyn && g.step < 1) || (g.n > 0 && (!g.param || !g.exp_avg || !g.exp_avg_sq)))  // grad == NULL: an exact-zero gradient, not materialised
        return gigs_internal_fail(GIGS_ERR_INVALID, "adam_step: bad group");
      if (g.n == 0) {
        if (dyn && k > 0) break;  // keep the (dyn_base + k) <-> group index correspondence: close this launch
        if (dyn) { G.dyn_base = done + 1; }
        continue;
      }
      const unsigned long long c = (unsigned long long)((g.n + gigs::kAdamChunk - 1) / gigs::kAdamChunk);
      if (chunks + c > 0x7fffffffull) break;  // next launch
      if (k == 0) G.dyn_base = done;
      G.param[k] = g.param; G.grad[k] = g.grad; G.exp_avg[k] = g.exp_avg; G.exp_avg_sq[k] = g.exp_avg_sq;
      G.n[k] = g.n;
      if (watch && changed && watch[done]) G.watch_mask |= 1u << k;
      G.first_chunk[k] = chunks;
      chunks += (unsigned)c;
      // torch/optim/adam.py (_single_tensor_adam): python-float bias corrections, then fp32 tensor ops
      if (!dyn) {
        float sc[2];
        gigs_adam_scalars(g.lr, g.step, beta1, beta2, sc);
        G.step_size[k] = sc[0];
        G.bc2_sqrt[k] = sc[1];
      }
      k++;
    }
    G.count = k;
    G.dyn = dyn;
    G.changed = changed;
    G.guard = guard;
    G.first_chunk[k] = chunks;
    if (k == 0 || chunks == 0) {
      if (k == 0 && done < n_groups)  // a single group too large for one grid
        return gigs_internal_fail(GIGS_ERR_INVALID, "adam_step: group too large");
      continue;
    }
    const gigs::AdamConsts K = {(float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps};
    // bit 8 of zero_grad (diagnostic, tools/adam_bw.py): the plain loads / stores instead of the streaming ones
    if (zero_grad & 0x100) hipLaunchKernelGGL(gigs::adam_kernel<false>, dim3(chunks), dim3(256), 0, s, G, K, zero_grad & 0xff);
    else hipLaunchKernelGGL(gigs::adam_kernel<true>, dim3(chunks), dim3(256), 0, s, G, K, zero_grad & 0xff);
  }
  return gigs_internal_check_launch("adam_step");
}

}  // extern "C"
