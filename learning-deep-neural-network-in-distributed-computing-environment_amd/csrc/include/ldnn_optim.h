// What the fused optimizer kernel files (optim.hip, optim_q.hip) share: streaming float4 access, the
// gradient zero ranges, the optional kernel arguments (clipping state, FedProx anchor) and the grid rule.
// Everything sits in an unnamed namespace: each kernel file gets its own copy, inlined into its kernels.
#pragma once

#include "ldnn_common.h"
#include "ldnn_kernels.h"

namespace ldnn {

extern int g_opt_max_blocks;  // optimizer grid cap (set_opt_max_blocks: a narrow side-stream update)

namespace {

constexpr int kBlock = 256;

// NT: streaming (nontemporal) loads / stores -- every optimizer byte is touched once
// per step, so it need not displace the L2 / Infinity Cache lines the next kernels
// read (headline -1.1 %, EnhancedCNN -1.4 %: profiles/optimizer_nontemporal_ab_r2.jsonl;
// every launch uses NT = true)
template <bool NT>
__device__ __forceinline__ floatx4 ld4(const float* p, int64_t i) {
  if constexpr (NT) return __builtin_nontemporal_load(reinterpret_cast<const floatx4*>(p) + i);
  else return reinterpret_cast<const floatx4*>(p)[i];
}
template <bool NT>
__device__ __forceinline__ void st4(float* p, int64_t i, floatx4 v) {
  if constexpr (NT) __builtin_nontemporal_store(v, reinterpret_cast<floatx4*>(p) + i);
  else reinterpret_cast<floatx4*>(p)[i] = v;
}

__device__ __forceinline__ bool in_zero(const GradZero& z, int64_t i) {
  return (i >= z.zb[0] && i < z.ze[0]) || (i >= z.zb[1] && i < z.ze[1]);
}

// consume-and-clear the gradient elements [4i, 4i+4) that fall in a zero range
__device__ __forceinline__ void clear4(const GradZero& z, float* grad, int64_t i) {
  const int64_t e = 4 * i;
  if (in_zero(z, e) && in_zero(z, e + 3)) {
    reinterpret_cast<floatx4*>(grad)[i] = floatx4{0.f, 0.f, 0.f, 0.f};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (in_zero(z, e + j)) grad[e + j] = 0.f;
  }
}

// CLIP: the kernel also takes the global-norm clipping state (ldnn_kernels.h ClipSlot).  The
// CLIP = false instances carry an empty argument and compile to the unclipped code.
template <bool CLIP>
struct ClipArg {
  static constexpr bool on = CLIP;
  const float* st;
};
template <>
struct ClipArg<false> {
  static constexpr bool on = false;
};

// PROX: the kernel also takes the FedProx anchor (the weights the round started from, fp32, laid out
// like the range's master) and a header whose first element is mu: mu * (p0 - anchor) joins the
// gradient where weight decay does, p0 the weight as loaded.  mu is read on the device, so a captured
// step follows a changed mu as it follows the lr.  The PROX = false instances carry an empty
// argument and compile to the code without it.
template <bool PROX>
struct ProxArg {
  static constexpr bool on = PROX;
  const float* anchor;
  const float* hdr;
};
template <>
struct ProxArg<false> {
  static constexpr bool on = false;
};

// a skipped (non-finite norm) step: only the requested gradient zero ranges are cleared
__device__ __forceinline__ void clear_only(const GradZero& z, float* grad, int64_t n) {
  if (z.ze[0] <= z.zb[0] && z.ze[1] <= z.zb[1]) return;
  const int64_t nv = n / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t i = t0; i < nv; i += stride) clear4(z, grad, i);
  for (int64_t i = nv * 4 + t0; i < n; i += stride)
    if (in_zero(z, i)) grad[i] = 0.f;
}

inline int grid_for(int64_t n4) {
  int64_t g = (n4 + kBlock - 1) / kBlock;
  return (int)(g < 1 ? 1 : (g > g_opt_max_blocks ? g_opt_max_blocks : g));
}

// launch(ClipArg<..>): the CLIP instance when a clipping state is given, else the unclipped one
template <class Launch>
void with_clip(const float* clip, Launch launch) {
  if (clip != nullptr) launch(ClipArg<true>{clip});
  else launch(ClipArg<false>{});
}

// launch(ProxArg<..>): the PROX instance when an anchor is given, else the one without the term
template <class Launch>
void with_prox(const float* anchor, const float* hdr, Launch launch) {
  if (anchor != nullptr) launch(ProxArg<true>{anchor, hdr});
  else launch(ProxArg<false>{});
}

}  // namespace
}  // namespace ldnn
