// Fused optimizer updates over flat fp32 master buffers.
//
// The reference steps torch.optim.Adam per tensor (BAR/main.py:53,
// BAR/trainer.py:210: 65 tensors, 44.6 M elements).  Here a model's parameters
// live in ONE flat fp32 buffer (views per tensor keep the reference state_dict
// keys), so one launch updates all of them and, in the same pass, refreshes
// the bf16 compute shadow that the MFMA kernels read.  The all-reduce average
// (1/world_size) and any loss scaling are folded into `grad_scale`.
//
// Hyper-parameters that change between steps (lr, Adam step count) are read
// from a device buffer `hp`, so a captured hipGraph replays with the current
// schedule value and no host sync.
#include <cstdlib>

#include "ldnn_common.h"
#include "ldnn_kernels.h"

namespace ldnn {

namespace {

constexpr int kBlock = 256;
constexpr int kSegChunk = 4096;  // elements of a seg_sumsq chunk: four float4 per thread and buffer

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

// LARS: the kernel also takes the per-tensor trust ratios (lars_finalize) and the map from each
// 64-element block of this launch's range to its ratio slot.  The LARS = false instances carry
// an empty argument and compile to the code without it.
template <bool LARS>
struct LarsArg {
  const float* ratio;
  const uint16_t* map;
};
template <>
struct LarsArg<false> {};

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

// one float4 of the SGD(-momentum) update: master, momentum, gradient clear; returns the
// new bf16 shadow values.  LARS: (g + weight_decay * p) is scaled by the trust ratio of the
// 64-element block the float4 lies in (segments start on 64-element boundaries).
template <bool NT, bool LARS, bool PROX>
__device__ __forceinline__ u16x4 sgd4(float* __restrict__ param, float* __restrict__ grad, float* __restrict__ mom,
                                      float lr, float grad_scale, const SgdParams& sp, int64_t i,
                                      const LarsArg<LARS>& lars, const ProxArg<PROX>& prox, float mu) {
  floatx4 p = ld4<NT>(param, i);
  floatx4 g = ld4<NT>(grad, i) * grad_scale;
  clear4(sp.zero, grad, i);
  if (sp.weight_decay != 0.f) g += sp.weight_decay * p;
  if constexpr (PROX) g += mu * (p - ld4<NT>(prox.anchor, i));
  if constexpr (LARS) g *= lars.ratio[lars.map[i >> 4]];
  if (sp.momentum != 0.f) {
    floatx4 b;
    if (sp.first_step) b = g;
    else b = sp.momentum * ld4<NT>(mom, i) + (1.f - sp.dampening) * g;
    st4<NT>(mom, i, b);
    g = sp.nesterov ? g + sp.momentum * b : b;
  }
  p -= lr * g;
  st4<NT>(param, i, p);
  return u16x4{f2bf(p[0]), f2bf(p[1]), f2bf(p[2]), f2bf(p[3])};
}

// TR: the flat range holds one [rows][cols] weight matrix at element `tr.begin` whose bf16
// shadow is also kept TRANSPOSED (tr.out = [cols][rows]; the MLP dgrad reads it so both
// GEMM operands are k-contiguous).  The first (rows / 64) x (cols / 64) workgroups update
// that matrix one 64 x 64 tile each and write the transposed tile through LDS; the rest
// stride over the remaining elements -- one launch instead of the update plus a
// transpose pass that re-reads the 32 MB shadow.
template <bool NT, bool TR, bool CLIP, bool LARS, bool PROX>
__global__ void sgd_kernel(float* __restrict__ param, float* __restrict__ grad, float* __restrict__ mom,
                           bf16_t* __restrict__ shadow, const float* __restrict__ hp, float grad_scale,
                           SgdParams sp, int64_t n, ShadowT tr, ClipArg<CLIP> clip, LarsArg<LARS> lars,
                           ProxArg<PROX> prox) {
  static_assert(!(TR && LARS), "the transposed-shadow form has no LARS instance");
  static_assert(!(PROX && (TR || LARS)), "the proximal term has no transposed-shadow and no LARS instance");
  if constexpr (CLIP) {
    if (clip.st[kClipSkip] != 0.f) {
      clear_only(sp.zero, grad, n);
      return;
    }
    grad_scale *= clip.st[kClipCoef];
  }
  const float lr = hp[0];
  float mu = 0.f;
  if constexpr (PROX) mu = prox.hdr[0];
  const int64_t nv = n / 4;
  int64_t bid = blockIdx.x, nblk = gridDim.x, skip_b = 0, skip_n = 0;
  if constexpr (TR) {
    __shared__ uint16_t t[64][66];
    const int tiles_c = tr.cols >> 6;
    const int ntiles = (tr.rows >> 6) * tiles_c;
    if (blockIdx.x < (unsigned)ntiles) {
      const int r0 = (blockIdx.x / tiles_c) * 64, c0 = (blockIdx.x % tiles_c) * 64;
      const int c4 = threadIdx.x & 15, rg = threadIdx.x >> 4;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int r = rg * 4 + k;
        const int64_t i = (tr.begin + (int64_t)(r0 + r) * tr.cols + c0 + c4 * 4) >> 2;
        const u16x4 b = sgd4<NT, LARS, PROX>(param, grad, mom, lr, grad_scale, sp, i, lars, prox, mu);
        if (shadow) reinterpret_cast<u16x4*>(shadow)[i] = b;
#pragma unroll
        for (int q = 0; q < 4; ++q) t[r][c4 * 4 + q] = b[q];
      }
      __syncthreads();
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int ch = threadIdx.x + h * 256;
        const int c = ch >> 3, r8 = (ch & 7) * 8;
        u16x8 v;
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = t[r8 + e][c];
        *reinterpret_cast<u16x8*>(tr.out + (size_t)(c0 + c) * tr.rows + r0 + r8) = v;
      }
      return;
    }
    bid -= ntiles;
    nblk -= ntiles;
    skip_b = tr.begin >> 2;
    skip_n = ((int64_t)tr.rows * tr.cols) >> 2;
  }
  const int64_t stride = nblk * blockDim.x;
  for (int64_t j = bid * (int64_t)blockDim.x + threadIdx.x; j < nv - skip_n; j += stride) {
    const int64_t i = (TR && j >= skip_b) ? j + skip_n : j;
    const u16x4 b = sgd4<NT, LARS, PROX>(param, grad, mom, lr, grad_scale, sp, i, lars, prox, mu);
    if (shadow) reinterpret_cast<u16x4*>(shadow)[i] = b;
  }
  for (int64_t i = nv * 4 + bid * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
    float p = param[i];
    float g = grad[i] * grad_scale;
    if (in_zero(sp.zero, i)) grad[i] = 0.f;
    if (sp.weight_decay != 0.f) g += sp.weight_decay * p;
    if constexpr (PROX) g += mu * (p - prox.anchor[i]);
    if constexpr (LARS) g *= lars.ratio[lars.map[i >> 6]];
    if (sp.momentum != 0.f) {
      const float b = sp.first_step ? g : sp.momentum * mom[i] + (1.f - sp.dampening) * g;
      mom[i] = b;
      g = sp.nesterov ? g + sp.momentum * b : b;
    }
    p -= lr * g;
    param[i] = p;
    if (shadow) shadow[i] = f2bf(p);
  }
}

// PROX: px = mu * (p0 - anchor), added behind the coupled weight decay
template <bool PROX>
__device__ __forceinline__ float adam_elem(float p, float g, float& m, float& v, float lr, float bc1,
                                           float bc2s, const AdamParams& ap, float px) {
  if (ap.weight_decay != 0.f) {
    if (ap.decoupled) p *= (1.f - lr * ap.weight_decay);
    else g += ap.weight_decay * p;
  }
  if constexpr (PROX) g += px;
  m = ap.beta1 * m + (1.f - ap.beta1) * g;
  v = ap.beta2 * v + (1.f - ap.beta2) * g * g;
  const float denom = sqrtf(v) / bc2s + ap.eps;
  return p - (lr / bc1) * m / denom;
}

template <bool NT, bool CLIP, bool PROX>
__global__ void adam_kernel(float* __restrict__ param, float* __restrict__ grad, float* __restrict__ mm,
                            float* __restrict__ vv, bf16_t* __restrict__ shadow, const float* __restrict__ hp,
                            float grad_scale, AdamParams ap, int64_t n, ClipArg<CLIP> clip, ProxArg<PROX> prox) {
  if constexpr (CLIP) {
    if (clip.st[kClipSkip] != 0.f) {
      clear_only(ap.zero, grad, n);
      return;
    }
    grad_scale *= clip.st[kClipCoef];
  }
  const float lr = hp[0];
  const float t = hp[1];
  float mu = 0.f;
  if constexpr (PROX) mu = prox.hdr[0];
  const float bc1 = 1.f - powf(ap.beta1, t);
  const float bc2s = sqrtf(1.f - powf(ap.beta2, t));
  const int64_t nv = n / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv; i += stride) {
    floatx4 p = ld4<NT>(param, i);
    const floatx4 g = ld4<NT>(grad, i) * grad_scale;
    clear4(ap.zero, grad, i);
    floatx4 m = ld4<NT>(mm, i);
    floatx4 v = ld4<NT>(vv, i);
    floatx4 px = {0.f, 0.f, 0.f, 0.f};
    if constexpr (PROX) px = mu * (p - ld4<NT>(prox.anchor, i));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float mj = m[j], vj = v[j];
      p[j] = adam_elem<PROX>(p[j], g[j], mj, vj, lr, bc1, bc2s, ap, px[j]);
      m[j] = mj;
      v[j] = vj;
    }
    st4<NT>(param, i, p);
    st4<NT>(mm, i, m);
    st4<NT>(vv, i, v);
    if (shadow) reinterpret_cast<u16x4*>(shadow)[i] = u16x4{f2bf(p[0]), f2bf(p[1]), f2bf(p[2]), f2bf(p[3])};
  }
  for (int64_t i = nv * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
    float m = mm[i], v = vv[i];
    const float p0 = param[i];
    float px = 0.f;
    if constexpr (PROX) px = mu * (p0 - prox.anchor[i]);
    const float p = adam_elem<PROX>(p0, grad[i] * grad_scale, m, v, lr, bc1, bc2s, ap, px);
    if (in_zero(ap.zero, i)) grad[i] = 0.f;
    param[i] = p;
    mm[i] = m;
    vv[i] = v;
    if (shadow) shadow[i] = f2bf(p);
  }
}

// ---- Lion (Chen et al. 2023): the sign of an interpolated momentum, ONE moment buffer ----
// c = beta1 m + (1 - beta1) g;  w = w (1 - lr wd) - lr sign(c);  m = beta2 m + (1 - beta2) g (from the
// old m).  sign: +-1, 0 at +-0, NaN at NaN (a NaN gradient reaches the weight, as in the other updates).
// No step count and no per-tensor norm: 22 B per element (w, g, m read; w, m, shadow written).
__device__ __forceinline__ float lion_elem(float p, float g, float& m, float lr, const LionParams& lp) {
  const float c = lp.beta1 * m + (1.f - lp.beta1) * g;
  const float s = c > 0.f ? 1.f : (c < 0.f ? -1.f : (c == c ? 0.f : c));
  if (lp.weight_decay != 0.f) p *= (1.f - lr * lp.weight_decay);
  m = lp.beta2 * m + (1.f - lp.beta2) * g;
  return p - lr * s;
}

template <bool NT, bool CLIP, bool PROX>
__global__ void lion_kernel(float* __restrict__ param, float* __restrict__ grad, float* __restrict__ mm,
                            bf16_t* __restrict__ shadow, const float* __restrict__ hp, float grad_scale,
                            LionParams lp, int64_t n, ClipArg<CLIP> clip, ProxArg<PROX> prox) {
  if constexpr (CLIP) {
    if (clip.st[kClipSkip] != 0.f) {
      clear_only(lp.zero, grad, n);
      return;
    }
    grad_scale *= clip.st[kClipCoef];
  }
  const float lr = hp[0];
  float mu = 0.f;
  if constexpr (PROX) mu = prox.hdr[0];
  const int64_t nv = n / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv; i += stride) {
    floatx4 p = ld4<NT>(param, i);
    floatx4 g = ld4<NT>(grad, i) * grad_scale;
    clear4(lp.zero, grad, i);
    floatx4 m = ld4<NT>(mm, i);
    if constexpr (PROX) g += mu * (p - ld4<NT>(prox.anchor, i));
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float mj = m[j];
      p[j] = lion_elem(p[j], g[j], mj, lr, lp);
      m[j] = mj;
    }
    st4<NT>(param, i, p);
    st4<NT>(mm, i, m);
    if (shadow) reinterpret_cast<u16x4*>(shadow)[i] = u16x4{f2bf(p[0]), f2bf(p[1]), f2bf(p[2]), f2bf(p[3])};
  }
  for (int64_t i = nv * 4 + blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += stride) {
    float m = mm[i];
    const float p0 = param[i];
    float g = grad[i] * grad_scale;
    if constexpr (PROX) g += mu * (p0 - prox.anchor[i]);
    const float p = lion_elem(p0, g, m, lr, lp);
    if (in_zero(lp.zero, i)) grad[i] = 0.f;
    param[i] = p;
    mm[i] = m;
    if (shadow) shadow[i] = f2bf(p);
  }
}

__global__ void bump_kernel(float* hp) { hp[1] += 1.f; }
// (a skipped step does not advance Adam's step count)
__global__ void bump_clip_kernel(float* hp, const float* __restrict__ clip) {
  if (clip[kClipSkip] == 0.f) hp[1] += 1.f;
}

// Sum of squares of g[0, n): float4 loads from the first 16-byte aligned element on (the head
// and tail scalars are peeled), four independent float4 accumulators per thread, wave64
// shuffle reduce, cross-wave through LDS; ONE plain store per workgroup and no atomics, so
// the partials -- and the fixed-order sum over them -- are the same bits on every run.
__global__ void sumsq_kernel(const float* __restrict__ g, int64_t n, float* __restrict__ partials) {
  const int64_t mis = (int64_t)((reinterpret_cast<uintptr_t>(g) >> 2) & 3);
  int64_t head = (4 - mis) & 3;
  if (head > n) head = n;
  const float* gb = g + head;
  const int64_t nv = (n - head) / 4;
  const int64_t tail0 = head + nv * 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  floatx4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = a0, a2 = a0, a3 = a0;
  int64_t i = t0;
  for (; i + 3 * stride < nv; i += 4 * stride) {
    const floatx4 v0 = ld4<false>(gb, i), v1 = ld4<false>(gb, i + stride), v2 = ld4<false>(gb, i + 2 * stride),
                  v3 = ld4<false>(gb, i + 3 * stride);
    a0 += v0 * v0;
    a1 += v1 * v1;
    a2 += v2 * v2;
    a3 += v3 * v3;
  }
  for (; i < nv; i += stride) {
    const floatx4 v = ld4<false>(gb, i);
    a0 += v * v;
  }
  a0 = (a0 + a1) + (a2 + a3);
  float acc = (a0[0] + a0[1]) + (a0[2] + a0[3]);
  if (t0 < head) acc += g[t0] * g[t0];
  if (tail0 + t0 < n) acc += g[tail0 + t0] * g[tail0 + t0];
  acc = wave_sum(acc);
  static_assert(kBlock == 256, "the cross-wave sum below adds exactly four waves");
  __shared__ float w[kBlock / 64];
  if ((threadIdx.x & 63) == 0) w[threadIdx.x >> 6] = acc;
  __syncthreads();
  if (threadIdx.x == 0) partials[blockIdx.x] = (w[0] + w[1]) + (w[2] + w[3]);
}

// One workgroup.  Fixed summation order: thread t adds its contiguous run of partials in index
// order, the 256 run sums meet in a fixed binary tree; all in double.
// sum_out: write the sum alone (the sharded path's local sum); else finalize `state`.
__global__ void clip_finalize_kernel(const float* __restrict__ partials, int nparts, const float* __restrict__ ext,
                                     float* __restrict__ state, float grad_scale, float* __restrict__ sum_out) {
  __shared__ double red[kBlock];
  const int per = (nparts + kBlock - 1) / kBlock;
  const int b = threadIdx.x * per;
  const int e = b + per < nparts ? b + per : nparts;
  double acc = 0.0;
  for (int i = b; i < e; ++i) acc += (double)partials[i];
  red[threadIdx.x] = acc;
  __syncthreads();
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x != 0) return;
  double sum = red[0];
  if (ext != nullptr) sum += (double)ext[0];
  if (sum_out != nullptr) {
    sum_out[0] = (float)sum;
    return;
  }
  const float norm = (float)((double)grad_scale * sqrt(sum));
  const bool finite = fabsf(norm) <= 3.402823466e38f;  // false for inf and NaN
  const float c = finite ? fminf(1.f, state[kClipMaxNorm] / (norm + 1e-6f)) : 0.f;
  state[kClipCoef] = c;
  state[kClipSkip] = finite ? 0.f : 1.f;
  state[kClipNorm] = norm;
  state[kClipSteps] += 1.f;
  if (finite && c < 1.f) state[kClipClipped] += 1.f;
  if (!finite) state[kClipSkipped] += 1.f;
}

// The per-chunk reduction of seg_sumsq and lamb_moments.  chunks[c] = (segment, begin / 64, end / 64,
// counted): a run of whole 64-element blocks inside one segment (a few thousand elements; a range
// that cuts a segment only changes which chunks exist).  ONE workgroup reduces a whole chunk (the grid
// strides over the chunks): body(i, a) returns one float4 of float4 index i and hands the other back
// in a; four independent accumulator pairs per thread, wave64 shuffle, LDS; partials[2c] = sum a^2,
// partials[2c + 1] = sum of the returned squares, plain stores: no atomics, and a chunk's partial does
// not depend on the grid, so equal inputs give equal bits.  COUNTED: a chunk whose fourth field is 0
// stores 0, 0.  A chunk outside [0, n) runs no body.
template <bool COUNTED, class Body>
__device__ __forceinline__ void chunk_sumsq(const int4* chunks, int nchunks, int64_t n,
                                            float* partials, Body body) {
  static_assert(kBlock == 256, "the cross-wave sum below adds exactly four waves");
  __shared__ float red[2][kBlock / 64];
  for (int c = blockIdx.x; c < nchunks; c += gridDim.x) {
    const int4 ch = chunks[c];
    int64_t b = (int64_t)ch.y * 16, e = (int64_t)ch.z * 16;  // in float4s
    if (ch.y < 0 || ch.z < ch.y || (int64_t)ch.z * 64 > n) b = e = 0;
    const floatx4 z = {0.f, 0.f, 0.f, 0.f};
    floatx4 w0 = z, w1 = z, w2 = z, w3 = z, g0 = z, g1 = z, g2 = z, g3 = z;
    int64_t i = b + threadIdx.x;
    for (; i + 3 * kBlock < e; i += 4 * kBlock) {
      floatx4 a0, a1, a2, a3;
      const floatx4 b0 = body(i, a0), b1 = body(i + kBlock, a1), b2 = body(i + 2 * kBlock, a2),
                    b3 = body(i + 3 * kBlock, a3);
      w0 += a0 * a0;
      w1 += a1 * a1;
      w2 += a2 * a2;
      w3 += a3 * a3;
      g0 += b0 * b0;
      g1 += b1 * b1;
      g2 += b2 * b2;
      g3 += b3 * b3;
    }
    for (; i < e; i += kBlock) {
      floatx4 a;
      const floatx4 bb = body(i, a);
      w0 += a * a;
      g0 += bb * bb;
    }
    w0 = (w0 + w1) + (w2 + w3);
    g0 = (g0 + g1) + (g2 + g3);
    const float sw = wave_sum((w0[0] + w0[1]) + (w0[2] + w0[3]));
    const float sg = wave_sum((g0[0] + g0[1]) + (g0[2] + g0[3]));
    if ((threadIdx.x & 63) == 0) {
      red[0][threadIdx.x >> 6] = sw;
      red[1][threadIdx.x >> 6] = sg;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
      const float s = (red[threadIdx.x][0] + red[threadIdx.x][1]) + (red[threadIdx.x][2] + red[threadIdx.x][3]);
      partials[2 * (int64_t)c + threadIdx.x] = (!COUNTED || ch.w != 0) ? s : 0.f;
    }
    __syncthreads();
  }
}

// Per-segment sums of squares of the master AND the gradient: partials[2c] (master) and
// partials[2c + 1] (gradient) of every chunk, whatever its fourth field.  Plain loads: the update
// re-reads both buffers right after.
__global__ void seg_sumsq_kernel(const float* __restrict__ w, const float* __restrict__ g,
                                 const int4* __restrict__ chunks, int nchunks, int64_t n,
                                 float* __restrict__ partials) {
  chunk_sumsq<false>(chunks, nchunks, n, partials, [&](int64_t i, floatx4& wq) __attribute__((always_inline)) {
    wq = ld4<false>(w, i);
    return ld4<false>(g, i);
  });
}

// One wave per segment (waves stride over the segments, so any S works).  segtab[s] = (first
// chunk, end chunk, adapted, -).  Fixed summation order, in double: lane l adds the segment's
// partials l, l + 64, ... in index order, the 64 lane sums meet in an xor butterfly (every lane
// ends with the same bits).  ext: [2S] sums added on top (the sharded path's all-reduced vector).
// sums_out: write the [2S] sums alone; else the ratios (ldnn_kernels.h trust_finalize).
// LAMB: the same sums (master, Adam direction u) give ratio = wn / un: no header, and the clip state
// lends its skip flag only (the coefficient went into the moments before u was formed).
template <bool LAMB>
__global__ void lars_finalize_kernel(const float* __restrict__ partials, int nchunks, const int4* __restrict__ segtab,
                                     int S, const float* __restrict__ ext, const float* __restrict__ hdr,
                                     const float* __restrict__ clip, float grad_scale, float weight_decay,
                                     float* __restrict__ ratio, float* __restrict__ w_norm,
                                     float* __restrict__ g_norm, float* __restrict__ sums_out) {
  if (sums_out == nullptr && clip != nullptr && clip[kClipSkip] != 0.f) return;  // a skipped step
  const int lane = threadIdx.x & 63;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  for (int s = (blockIdx.x * blockDim.x + threadIdx.x) >> 6; s < S; s += nwaves) {
    const int4 t = segtab[s];
    double aw = 0.0, ag = 0.0;
    if (partials != nullptr && t.x >= 0 && t.y <= nchunks) {
      for (int c = t.x + lane; c < t.y; c += 64) {
        aw += (double)partials[2 * (int64_t)c];
        ag += (double)partials[2 * (int64_t)c + 1];
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      aw += __shfl_xor(aw, o, 64);
      ag += __shfl_xor(ag, o, 64);
    }
    if (lane != 0) continue;
    if (ext != nullptr) {
      aw += (double)ext[2 * s];
      ag += (double)ext[2 * s + 1];
    }
    if (sums_out != nullptr) {
      sums_out[2 * s] = (float)aw;
      sums_out[2 * s + 1] = (float)ag;
      continue;
    }
    const double c = (!LAMB && clip != nullptr) ? (double)clip[kClipCoef] : 1.0;
    const double wn = sqrt(aw), gn = LAMB ? sqrt(ag) : c * (double)grad_scale * sqrt(ag);
    double r = 1.0;
    if (t.z != 0 && wn > 0.0 && gn > 0.0) {
      // (a sum of squares that overflowed fp32: ratio 0, the tensor does not move)
      const bool over = (float)aw > 3.402823466e38f || (float)ag > 3.402823466e38f;
      if constexpr (LAMB) r = over ? 0.0 : wn / gn;
      else r = over ? 0.0 : (double)hdr[0] * wn / (gn + (double)weight_decay * wn + (double)hdr[1]);
    }
    ratio[s] = (float)r;
    w_norm[s] = (float)wn;
    g_norm[s] = (float)gn;
  }
}

// ---- LAMB (You et al. 2020): the Adam direction u, scaled per tensor by |w| / |u| ----
// The norm of u needs this step's moments, so the step is two passes: lamb_moments (moment update +
// per-chunk sums of w^2 and u^2), the finalize above, and lamb_apply, which recomputes u from the
// stored moments with THIS function (both passes move 42 B per element either way, and u parked
// in the gradient buffer would change what a caller sees in .grad after step()).
// rbc1 = 1 / (1 - beta1^t), rbc2 = 1 / (1 - beta2^t)
__device__ __forceinline__ float lamb_u(float w, float m, float v, float rbc1, float rbc2, const LambParams& lp) {
  return (m * rbc1) / (sqrtf(v * rbc2) + lp.eps) + lp.weight_decay * w;
}

// one float4 of the moments pass: new m, v stored; returns u (wq: the weights read).  POL, the access
// policy: 0 everything plain; 1 (what every step uses) the gradient with nontemporal loads -- it is
// dead after this pass -- and w, m, v plain, since lamb_apply re-reads all three right after; 2
// everything nontemporal.  Whole LAMB step (moments + finalize + apply) on ResNet-18's / EnhancedCNN's
// flat buffers, us, policy 0 / 1 / 2: warm 91.4 / 93.6 / 100.2 and 343.8 / 330.4 / 332.7; with 512 MiB
// streamed through the cache before every iteration 120.9 / 112.1 / 104.8 and 370.0 / 355.6 / 353.5.
// Policy 2 makes the moments pass itself faster where the buffers are cold (55 against 70 us) but
// hands part of it back in the apply pass; 1 is the best or within 1 % of it in three of the four
// (scripts/bench_lamb.py, profiles/r9/lamb_ab.jsonl).
template <int POL>
__device__ __forceinline__ floatx4 lamb_mom4(const float* __restrict__ w, const float* __restrict__ g,
                                             float* __restrict__ mm, float* __restrict__ vv, int64_t i, float gs,
                                             float rbc1, float rbc2, const LambParams& lp, floatx4& wq) {
  constexpr bool NTG = POL >= 1, NTA = POL == 2;
  wq = ld4<NTA>(w, i);
  const floatx4 gq = ld4<NTG>(g, i) * gs;
  floatx4 m = ld4<NTA>(mm, i), v = ld4<NTA>(vv, i), u;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    m[j] = lp.beta1 * m[j] + (1.f - lp.beta1) * gq[j];
    v[j] = lp.beta2 * v[j] + (1.f - lp.beta2) * gq[j] * gq[j];
    u[j] = lamb_u(wq[j], m[j], v[j], rbc1, rbc2, lp);
  }
  st4<NTA>(mm, i, m);
  st4<NTA>(vv, i, v);
  return u;
}

// chunk_sumsq over lamb_mom4: partials[2c] = sum w^2, partials[2c + 1] = sum u^2 over the chunk.  An
// uncounted chunk (another rank counts these elements) updates its moments and stores 0, 0.
template <bool CLIP, int POL>
__global__ void lamb_moments_kernel(const float* __restrict__ w, const float* __restrict__ g, float* __restrict__ mm,
                                    float* __restrict__ vv, const int4* __restrict__ chunks, int nchunks, int64_t n,
                                    const float* __restrict__ hp, float grad_scale, LambParams lp,
                                    float* __restrict__ partials, ClipArg<CLIP> clip) {
  if constexpr (CLIP) {
    if (clip.st[kClipSkip] != 0.f) return;  // a skipped step: moments and partials stay
    grad_scale *= clip.st[kClipCoef];
  }
  const float t = hp[1];
  const float rbc1 = 1.f / (1.f - powf(lp.beta1, t)), rbc2 = 1.f / (1.f - powf(lp.beta2, t));
  chunk_sumsq<true>(chunks, nchunks, n, partials, [&](int64_t i, floatx4& wq) __attribute__((always_inline)) {
    return lamb_mom4<POL>(w, g, mm, vv, i, grad_scale, rbc1, rbc2, lp, wq);
  });
}

// w -= lr * ratio * u over [0, n) (n a multiple of 64), u recomputed from the moments this step's
// lamb_moments stored; refreshes the bf16 shadow and clears the gradient zero ranges.  w, m, v: NT
// (nothing reads them again this step).  CLIP: the skip flag alone (clear the zero ranges only).
template <bool CLIP>
__global__ void lamb_apply_kernel(float* __restrict__ param, float* __restrict__ grad, const float* __restrict__ mm,
                                  const float* __restrict__ vv, bf16_t* __restrict__ shadow,
                                  const float* __restrict__ hp, LambParams lp, int64_t n,
                                  const float* __restrict__ ratio, const uint16_t* __restrict__ map,
                                  ClipArg<CLIP> clip) {
  if constexpr (CLIP) {
    if (clip.st[kClipSkip] != 0.f) {
      clear_only(lp.zero, grad, n);
      return;
    }
  }
  const float lr = hp[0], t = hp[1];
  const float rbc1 = 1.f / (1.f - powf(lp.beta1, t)), rbc2 = 1.f / (1.f - powf(lp.beta2, t));
  const bool clear = lp.zero.ze[0] > lp.zero.zb[0] || lp.zero.ze[1] > lp.zero.zb[1];
  const int64_t nv = n / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < nv; i += stride) {
    floatx4 p = ld4<true>(param, i);
    const floatx4 m = ld4<true>(mm, i), v = ld4<true>(vv, i);
    if (clear) clear4(lp.zero, grad, i);
    const float s = lr * ratio[map[i >> 4]];
#pragma unroll
    for (int j = 0; j < 4; ++j) p[j] -= s * lamb_u(p[j], m[j], v[j], rbc1, rbc2, lp);
    st4<true>(param, i, p);
    if (shadow) reinterpret_cast<u16x4*>(shadow)[i] = u16x4{f2bf(p[0]), f2bf(p[1]), f2bf(p[2]), f2bf(p[3])};
  }
}

// ---- EMA of the weights: a pass of its own behind the update kernels (12 B per element) ----
// One thread, once per step, before any range: this step's coefficient and the update count.
template <bool CLIP>
__global__ void ema_begin_kernel(float* hdr, ClipArg<CLIP> clip) {
  if constexpr (CLIP) {
    if (clip.st[kClipSkip] != 0.f) {  // a skipped step averages nothing and is not counted
      hdr[kEmaAlpha] = 0.f;
      return;
    }
  }
  const float c = hdr[kEmaUpdates];
  float a = 1.f - hdr[kEmaDecay];
  if (hdr[kEmaWarmup] != 0.f) a = fmaxf(a, 9.f / (10.f + c));
  hdr[kEmaAlpha] = a;
  hdr[kEmaUpdates] = c + 1.f;
}

// e += a_t * (w - e).  e is touched once per step: nontemporal both ways.  The master, which the
// update kernel has just written with nontemporal stores, is loaded nontemporally too -- a measured
// choice against plain loads (scripts/bench_ema.py's buffers, profiles/r12/ema_master_load_ab.jsonl).
// The pair "Adam then ema_update", us, plain / nontemporal: warm loops 88.2 / 91.4 (ResNet-18) and
// 304.9 / 324.6 (EnhancedCNN), but with 512 MiB streamed through the cache before every iteration, as
// a forward and backward leave it, 103.4 / 96.6 and 377.9 / 348.5; and the graphed training step
// decides the same way: EnhancedCNN b64 Adam 1.769 / 1.731 ms (1.635 without the EMA), ResNet-18 b64
// SGD 2.629 / 2.631 against 2.603 (profiles/r12/ema_graphed_steps.jsonl).
__global__ void ema_update_kernel(const float* __restrict__ master, float* __restrict__ ema,
                                  const float* __restrict__ hdr, int64_t n) {
  const float a = hdr[kEmaAlpha];
  if (a == 0.f) return;
  const int64_t nv = n / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t i = t0; i < nv; i += stride) {
    const floatx4 w = ld4<true>(master, i);
    floatx4 e = ld4<true>(ema, i);
    e += a * (w - e);
    st4<true>(ema, i, e);
  }
  for (int64_t i = nv * 4 + t0; i < n; i += stride) {
    const float e = ema[i];
    ema[i] = e + a * (master[i] - e);
  }
}

// master <-> ema, shadow = bf16(new master): every element is read and written by one thread, so the
// exchange is exact.
__global__ void ema_swap_kernel(float* __restrict__ master, float* __restrict__ ema, bf16_t* __restrict__ shadow,
                                int64_t n) {
  const int64_t nv = n / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t t0 = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  for (int64_t i = t0; i < nv; i += stride) {
    const floatx4 w = ld4<true>(master, i), e = ld4<true>(ema, i);
    st4<true>(master, i, e);
    st4<true>(ema, i, w);
    if (shadow) reinterpret_cast<u16x4*>(shadow)[i] = u16x4{f2bf(e[0]), f2bf(e[1]), f2bf(e[2]), f2bf(e[3])};
  }
  for (int64_t i = nv * 4 + t0; i < n; i += stride) {
    const float w = master[i], e = ema[i];
    master[i] = e;
    ema[i] = w;
    if (shadow) shadow[i] = f2bf(e);
  }
}

// ---- per-step learning-rate schedule: this step's rate into hp[0], where every update reads it ----
// One thread, once per step, behind the norms' finalize (the skip flag is known) and before any
// update.  A skipped step writes nothing: the updates return on the flag, and t counts the steps
// that changed the weights.
template <bool CLIP>
__global__ void lr_sched_kernel(float* hdr, float* hp, ClipArg<CLIP> clip) {
  if constexpr (CLIP) {
    if (clip.st[kClipSkip] != 0.f) return;
  }
  const float t = hdr[kSchedSteps], u = t + 1.f;
  const float W = hdr[kSchedWarmup], m = hdr[kSchedMin];
  const int kind = (int)hdr[kSchedKind];
  float s = 1.f;
  if (u <= W) {
    const float ws = hdr[kSchedStart];
    s = ws + (1.f - ws) * (u / W);
  } else if (kind != 0) {
    const float p = fminf(1.f, (u - W) / (hdr[kSchedTotal] - W));
    s = m + (1.f - m) * (kind == 1 ? powf(1.f - p, hdr[kSchedPower]) : 0.5f * (1.f + cospif(p)));
  }
  hp[0] = hdr[kSchedBase] * s;
  hdr[kSchedFactor] = s;
  hdr[kSchedSteps] = u;
}

int g_opt_max_blocks = 2048;  // optimizer grid cap (set_opt_max_blocks: a narrow side-stream update)

inline int grid_for(int64_t n4) {
  int64_t g = (n4 + kBlock - 1) / kBlock;
  return (int)(g < 1 ? 1 : (g > g_opt_max_blocks ? g_opt_max_blocks : g));
}
// a chunk-table kernel: one workgroup per chunk up to the cap
inline int chunk_grid(int nchunks) { return nchunks < g_opt_max_blocks ? nchunks : g_opt_max_blocks; }
// the finalize kernel: one wave per segment, at most 256 workgroups
inline int finalize_grid(int S) {
  const int g = (S + kBlock / 64 - 1) / (kBlock / 64);
  return g > 256 ? 256 : g;
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

template <bool TR, bool LARS, bool PROX = false>
void launch_sgd(int grid, float* param, float* grad, float* mom, uint16_t* shadow, const float* hp, float grad_scale,
                const SgdParams& sp, int64_t n, hipStream_t s, const ShadowT& tr, const float* clip,
                LarsArg<LARS> la, ProxArg<PROX> pa = {}) {
  with_clip(clip, [&](auto ca) {
    sgd_kernel<true, TR, ca.on, LARS, PROX><<<grid, kBlock, 0, s>>>(param, grad, mom, shadow, hp, grad_scale, sp, n, tr,
                                                                    ca, la, pa);
  });
}

}  // namespace

void set_opt_max_blocks(int n) { g_opt_max_blocks = n > 0 ? n : 2048; }

hipError_t sgd_step(float* param, float* grad, float* mom, uint16_t* shadow, const float* hp,
                    float grad_scale, SgdParams sp, int64_t n, hipStream_t s, const ShadowT* tr, const float* clip,
                    const float* lars_ratio, const uint16_t* lars_map, const float* prox_anchor,
                    const float* prox_hdr) {
  if (n <= 0) return hipSuccess;
  const bool lars = lars_ratio != nullptr;
  if (lars != (lars_map != nullptr)) return hipErrorInvalidValue;
  const bool prox = prox_anchor != nullptr;
  if (prox != (prox_hdr != nullptr)) return hipErrorInvalidValue;
  // (no agreed LARS form with a proximal term; only the static engine transposes, and it has neither)
  if (prox && (lars || (tr != nullptr && tr->out != nullptr))) return hipErrorInvalidValue;
  if (tr != nullptr && tr->out != nullptr) {
    if (lars) return hipErrorInvalidValue;  // (only the static engine transposes; it has no LARS)
    // (the tile path needs whole 64 x 64 tiles and 16-B aligned transposed rows)
    if (tr->rows <= 0 || tr->cols <= 0 || tr->rows % 64 || tr->cols % 64 || tr->begin % 4 || tr->begin < 0 ||
        tr->begin + (int64_t)tr->rows * tr->cols > n || ((uintptr_t)tr->out & 15))
      return hipErrorInvalidValue;
    const int64_t ntiles = (int64_t)(tr->rows / 64) * (tr->cols / 64);
    const int64_t rest = (n - (int64_t)tr->rows * tr->cols + 3) / 4;
    launch_sgd<true, false>((int)ntiles + grid_for(rest), param, grad, mom, shadow, hp, grad_scale, sp, n, s, *tr, clip,
                            {});
    return hipGetLastError();
  }
  const int grid = grid_for((n + 3) / 4);
  if (lars)
    launch_sgd<false, true>(grid, param, grad, mom, shadow, hp, grad_scale, sp, n, s, ShadowT{}, clip,
                            {lars_ratio, lars_map});
  else if (prox)
    launch_sgd<false, false, true>(grid, param, grad, mom, shadow, hp, grad_scale, sp, n, s, ShadowT{}, clip, {},
                                   {prox_anchor, prox_hdr});
  else
    launch_sgd<false, false>(grid, param, grad, mom, shadow, hp, grad_scale, sp, n, s, ShadowT{}, clip, {});
  return hipGetLastError();
}

hipError_t adam_step(float* param, float* grad, float* m, float* v, uint16_t* shadow, const float* hp,
                     float grad_scale, AdamParams ap, int64_t n, hipStream_t s, const float* clip,
                     const float* prox_anchor, const float* prox_hdr) {
  if (n <= 0) return hipSuccess;
  if ((prox_anchor != nullptr) != (prox_hdr != nullptr)) return hipErrorInvalidValue;
  with_clip(clip, [&](auto ca) {
    with_prox(prox_anchor, prox_hdr, [&](auto pa) {
      adam_kernel<true, decltype(ca)::on, decltype(pa)::on><<<grid_for((n + 3) / 4), kBlock, 0, s>>>(
          param, grad, m, v, shadow, hp, grad_scale, ap, n, ca, pa);
    });
  });
  return hipGetLastError();
}

hipError_t lion_step(float* param, float* grad, float* m, uint16_t* shadow, const float* hp, float grad_scale,
                     LionParams lp, int64_t n, hipStream_t s, const float* clip, const float* prox_anchor,
                     const float* prox_hdr) {
  if (n <= 0) return hipSuccess;
  if ((prox_anchor != nullptr) != (prox_hdr != nullptr)) return hipErrorInvalidValue;
  with_clip(clip, [&](auto ca) {
    with_prox(prox_anchor, prox_hdr, [&](auto pa) {
      lion_kernel<true, decltype(ca)::on, decltype(pa)::on><<<grid_for((n + 3) / 4), kBlock, 0, s>>>(
          param, grad, m, shadow, hp, grad_scale, lp, n, ca, pa);
    });
  });
  return hipGetLastError();
}

hipError_t bump_step(float* hp, hipStream_t s, const float* clip) {
  if (clip != nullptr) bump_clip_kernel<<<1, 1, 0, s>>>(hp, clip);
  else bump_kernel<<<1, 1, 0, s>>>(hp);
  return hipGetLastError();
}

int grad_sumsq_parts(int64_t n) { return n <= 0 ? 0 : grid_for((n + 3) / 4); }

hipError_t grad_sumsq(const float* grad, int64_t n, float* partials, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  sumsq_kernel<<<grad_sumsq_parts(n), kBlock, 0, s>>>(grad, n, partials);
  return hipGetLastError();
}

hipError_t sumsq_total(const float* partials, int nparts, float* out, hipStream_t s) {
  clip_finalize_kernel<<<1, kBlock, 0, s>>>(partials, nparts, nullptr, nullptr, 1.f, out);
  return hipGetLastError();
}

hipError_t clip_finalize(const float* partials, int nparts, const float* ext, float* state, float grad_scale,
                         hipStream_t s) {
  clip_finalize_kernel<<<1, kBlock, 0, s>>>(partials, nparts, ext, state, grad_scale, nullptr);
  return hipGetLastError();
}

int seg_sumsq_chunk() { return kSegChunk; }

hipError_t seg_sumsq(const float* master, const float* grad, int64_t n, const int32_t* chunks, int nchunks,
                     float* partials, hipStream_t s) {
  if (nchunks <= 0) return hipSuccess;
  seg_sumsq_kernel<<<chunk_grid(nchunks), kBlock, 0, s>>>(master, grad, reinterpret_cast<const int4*>(chunks), nchunks,
                                                          n, partials);
  return hipGetLastError();
}

hipError_t trust_finalize(bool lamb, const float* partials, int nchunks, const int32_t* segtab, int S,
                          const float* ext, const float* hdr, const float* clip, float grad_scale, float weight_decay,
                          float* ratio, float* w_norm, float* g_norm, float* sums_out, hipStream_t s) {
  if (S <= 0) return hipSuccess;
  const auto kernel = lamb ? lars_finalize_kernel<true> : lars_finalize_kernel<false>;
  kernel<<<finalize_grid(S), kBlock, 0, s>>>(partials, nchunks, reinterpret_cast<const int4*>(segtab), S, ext, hdr,
                                             clip, grad_scale, weight_decay, ratio, w_norm, g_norm, sums_out);
  return hipGetLastError();
}

hipError_t lamb_moments(const float* master, const float* grad, float* m, float* v, int64_t n, const int32_t* chunks,
                        int nchunks, const float* hp, float grad_scale, LambParams lp, float* partials,
                        hipStream_t s, const float* clip, int policy) {
  if (nchunks <= 0) return hipSuccess;
  if (policy < 0 || policy > 2) return hipErrorInvalidValue;
  with_clip(clip, [&](auto ca) {
    const auto kernel = policy == 1   ? lamb_moments_kernel<ca.on, 1>
                        : policy == 2 ? lamb_moments_kernel<ca.on, 2>
                                      : lamb_moments_kernel<ca.on, 0>;
    kernel<<<chunk_grid(nchunks), kBlock, 0, s>>>(master, grad, m, v, reinterpret_cast<const int4*>(chunks), nchunks, n,
                                                  hp, grad_scale, lp, partials, ca);
  });
  return hipGetLastError();
}

hipError_t lamb_apply(float* param, float* grad, const float* m, const float* v, uint16_t* shadow, const float* hp,
                      LambParams lp, int64_t n, const float* ratio, const uint16_t* map, hipStream_t s,
                      const float* clip) {
  if (n <= 0) return hipSuccess;
  if (n % 64 || ratio == nullptr || map == nullptr) return hipErrorInvalidValue;
  with_clip(clip, [&](auto ca) {
    lamb_apply_kernel<ca.on><<<grid_for(n / 4), kBlock, 0, s>>>(param, grad, m, v, shadow, hp, lp, n, ratio, map, ca);
  });
  return hipGetLastError();
}

hipError_t lr_sched(float* hdr, float* hp, hipStream_t s, const float* clip) {
  with_clip(clip, [&](auto ca) { lr_sched_kernel<ca.on><<<1, 1, 0, s>>>(hdr, hp, ca); });
  return hipGetLastError();
}

hipError_t ema_begin(float* hdr, hipStream_t s, const float* clip) {
  with_clip(clip, [&](auto ca) { ema_begin_kernel<ca.on><<<1, 1, 0, s>>>(hdr, ca); });
  return hipGetLastError();
}

hipError_t ema_update(const float* master, float* ema, const float* hdr, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  ema_update_kernel<<<grid_for((n + 3) / 4), kBlock, 0, s>>>(master, ema, hdr, n);
  return hipGetLastError();
}

hipError_t ema_swap(float* master, float* ema, uint16_t* shadow, int64_t n, hipStream_t s) {
  if (n <= 0) return hipSuccess;
  ema_swap_kernel<<<grid_for((n + 3) / 4), kBlock, 0, s>>>(master, ema, shadow, n);
  return hipGetLastError();
}

}  // namespace ldnn
