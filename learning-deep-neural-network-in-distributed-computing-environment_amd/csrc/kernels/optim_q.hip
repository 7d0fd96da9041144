// Adam8bit: the fused Adam update with both moments kept as block-scaled OCP fp8 (e4m3fn) codes
// (Dettmers et al. 2022, "8-bit Optimizers via Block-wise Quantization"; Peng et al. 2023, FP8-LM).
//
// A block is 64 consecutive flat elements.  Per block the state is 64 codes of the first moment m, 64
// codes of s = sqrt(v) (the root halves the second moment's dynamic range) and one fp32 scale each:
// 18.25 B move per element (w 8, g 4, bf16 shadow 2, codes 4, scales 0.25) where adam_kernel moves 30.
//
// One step of one block (optim/optimizers.py _adam8_torch is the same function in torch ops):
//   m0 = dec(cm) * sm, s0 = dec(cs) * ss, v0 = s0^2;  g as adam_elem forms it
//   m = b1 m0 + (1 - b1) g,  v = b2 v0 + (1 - b2) g^2,  v = max(v, m^2 (1 - b2) / (1 - b1)) when b1 <= b2
//   s = sqrt(v),  p -= (lr / bc1) m / (s / bc2s + eps)            (the fp32 m and s, not their codes)
//   for x in {m, s}: a = max_block |x|, scale = a / 448, y = x * min(448 / a, FLT_MAX) (0 when a == 0),
//   clamped to +-448, rounded stochastically to 3 mantissa bits in the fp32 bit pattern
//   (bits + (r << 4)) & ~0xFFFFF with 16 random bits r, then converted by v_cvt_pk_fp8_f32 -- exact on
//   the e4m3 grid; below 2^-6, the e4m3 subnormals, its round-to-nearest applies.
// The floor is a no-op for exact Adam (Cauchy-Schwarz); with quantised state it bounds the step of an
// element whose second moment rounded to 0 under a surviving first moment by sqrt((1 - b1) / (1 - b2)) lr.
// The block maximum is taken on the bit patterns of |x| as unsigned integers: it orders finite values
// as floats do and puts inf and NaN on top, so a non-finite element makes its block's scale non-finite.
//
// Random bits: key = smix(smix(seed) ^ t), t the step count hp[1] (after bump_step: a skipped step
// draws nothing, a replay advances).  The four elements at ABSOLUTE flat index 4q share
// h_m = smix(key ^ q * 0xD1B54A32D192ED03) and h_s = smix(h_m); element j takes bits [16j, 16j + 16).
// `base` is the launch's element offset in the flat buffer, so whole-buffer, range and sharded steps
// write the same bits.
//
// Work split: V float4 per lane, 16 / V lanes per block.  V = 1: sixteen lanes -- one DPP row -- own a
// block, a wave64 covers four; codes move as one 4-byte word per lane and moment, 64 B contiguous per
// block.  V = 2: eight lanes per block, 8-byte code accesses against two 16-byte loads per operand.
// The block maxima meet in an xor butterfly inside the row, all DPP: quad_perm for 1 and 2,
// row_half_mirror and row_mirror for 4 and 8 (on values already equal within quads / halves these ARE
// the xor exchanges).  No LDS, no atomics, no scratch; the loop strides over blocks, so a row's lanes
// leave it together and every DPP source lane is live.
#include <cfloat>

#include "ldnn_optim.h"

namespace ldnn {

namespace {

constexpr uint64_t kGroupMul = 0xD1B54A32D192ED03ull;

// splitmix64's finaliser (dropout.hip's smix64, data/autoaugment.smix)
__device__ __forceinline__ uint64_t smix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_max(uint32_t x) {
  const uint32_t y = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xF, 0xF, false);
  return x > y ? x : y;
}

// max over the block's LANES lanes (8 or 16, aligned in a DPP row); every lane ends with it
template <int LANES>
__device__ __forceinline__ uint32_t block_max(uint32_t x) {
  x = dpp_max<0xB1>(x);   // quad_perm [1, 0, 3, 2]: xor 1
  x = dpp_max<0x4E>(x);   // quad_perm [2, 3, 0, 1]: xor 2
  x = dpp_max<0x141>(x);  // row_half_mirror: xor 4 of quad-uniform values
  if constexpr (LANES == 16) x = dpp_max<0x140>(x);  // row_mirror: xor 8 of half-uniform values
  return x;
}

__device__ __forceinline__ uint32_t abs_bits(float x) { return __builtin_bit_cast(uint32_t, x) & 0x7FFFFFFFu; }

// four codes -> fp32 (byte j of the word is element j)
__device__ __forceinline__ floatx4 dec4(uint32_t c) {
  const auto lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)c, false);
  const auto hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)c, true);
  return floatx4{lo[0], lo[1], hi[0], hi[1]};
}

// x * inv clamped to +-448, stochastically rounded to the e4m3 grid; r: 16 random bits
__device__ __forceinline__ float sr_e4m3(float x, float inv, uint32_t r) {
  const float y = fminf(fmaxf(x * inv, -448.f), 448.f);
  return __builtin_bit_cast(float, (__builtin_bit_cast(uint32_t, y) + (r << 4)) & ~0xFFFFFu);
}

// four values of a block whose maximum magnitude is a -> their codes; h: this group's 64 random bits
__device__ __forceinline__ uint32_t enc4(floatx4 x, float a, uint64_t h) {
  const float inv = a > 0.f ? fminf(448.f / a, FLT_MAX) : 0.f;
  const uint32_t lo = (uint32_t)h, hi = (uint32_t)(h >> 32);
  int w = __builtin_amdgcn_cvt_pk_fp8_f32(sr_e4m3(x[0], inv, lo & 0xFFFFu), sr_e4m3(x[1], inv, lo >> 16), 0, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(sr_e4m3(x[2], inv, hi & 0xFFFFu), sr_e4m3(x[3], inv, hi >> 16), w, true);
  return (uint32_t)w;
}

struct Adam8Args {
  uint32_t* mq;   // codes, four to a word
  uint32_t* sq;
  float* mscale;  // one per block
  float* sscale;
  uint64_t seed;
  int64_t base;   // the range's element offset in the flat buffer (a multiple of 64)
};

template <bool NT, bool CLIP, bool PROX, int V>
__global__ void adam8_kernel(float* __restrict__ param, float* __restrict__ grad, Adam8Args q,
                             bf16_t* __restrict__ shadow, const float* __restrict__ hp, float grad_scale,
                             Adam8Params ap, int64_t n, ClipArg<CLIP> clip, ProxArg<PROX> prox) {
  static_assert(V == 1 || V == 2, "one or two float4 per lane");
  constexpr int LANES = 16 / V;
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
  const float step = lr / bc1;
  const uint64_t key = smix64(smix64(q.seed) ^ (uint64_t)(int64_t)t);
  const int64_t q0 = q.base >> 2;
  const int64_t nblk = n >> 6;
  const int64_t tid = blockIdx.x * (int64_t)blockDim.x + threadIdx.x;
  const int64_t nrows = ((int64_t)gridDim.x * blockDim.x) / LANES;
  const int r = (int)(tid % LANES);
  for (int64_t blk = tid / LANES; blk < nblk; blk += nrows) {
    const int64_t i0 = blk * 16 + r * V;  // this lane's first float4
    floatx4 p[V], g[V], m[V], s[V];
    uint32_t cm[V], cs[V];
#pragma unroll
    for (int k = 0; k < V; ++k) {
      p[k] = ld4<NT>(param, i0 + k);
      g[k] = ld4<NT>(grad, i0 + k) * grad_scale;
    }
    if constexpr (V == 1) {
      cm[0] = NT ? __builtin_nontemporal_load(q.mq + i0) : q.mq[i0];
      cs[0] = NT ? __builtin_nontemporal_load(q.sq + i0) : q.sq[i0];
    } else {
      const uint2 a = *reinterpret_cast<const uint2*>(q.mq + i0), b = *reinterpret_cast<const uint2*>(q.sq + i0);
      cm[0] = a.x, cm[1] = a.y, cs[0] = b.x, cs[1] = b.y;
    }
    const float sm = q.mscale[blk], ss = q.sscale[blk];
    uint32_t am = 0, as = 0;
#pragma unroll
    for (int k = 0; k < V; ++k) {
      clear4(ap.zero, grad, i0 + k);
      floatx4 px = {0.f, 0.f, 0.f, 0.f};
      if constexpr (PROX) px = mu * (p[k] - ld4<NT>(prox.anchor, i0 + k));
      const floatx4 m0 = dec4(cm[k]) * sm, s0 = dec4(cs[k]) * ss;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float pj = p[k][j], gj = g[k][j];
        if (ap.weight_decay != 0.f) {
          if (ap.decoupled) pj *= (1.f - lr * ap.weight_decay);
          else gj += ap.weight_decay * pj;
        }
        if constexpr (PROX) gj += px[j];
        const float mj = ap.beta1 * m0[j] + ap.omb1 * gj;
        float vj = ap.beta2 * (s0[j] * s0[j]) + ap.omb2 * gj * gj;
        vj = fmaxf(vj, mj * mj * ap.vfloor);
        const float sj = sqrtf(vj);
        p[k][j] = pj - step * mj / (sj / bc2s + ap.eps);
        m[k][j] = mj;
        s[k][j] = sj;
        const uint32_t bm = abs_bits(mj), bs = abs_bits(sj);
        am = am > bm ? am : bm;
        as = as > bs ? as : bs;
      }
    }
    const float a_m = __builtin_bit_cast(float, block_max<LANES>(am));
    const float a_s = __builtin_bit_cast(float, block_max<LANES>(as));
#pragma unroll
    for (int k = 0; k < V; ++k) {
      const uint64_t hm = smix64(key ^ ((uint64_t)(q0 + i0 + k) * kGroupMul));
      cm[k] = enc4(m[k], a_m, hm);
      cs[k] = enc4(s[k], a_s, smix64(hm));
      st4<NT>(param, i0 + k, p[k]);
      if (shadow)
        reinterpret_cast<u16x4*>(shadow)[i0 + k] = u16x4{f2bf(p[k][0]), f2bf(p[k][1]), f2bf(p[k][2]), f2bf(p[k][3])};
    }
    if constexpr (V == 1) {
      if constexpr (NT) {
        __builtin_nontemporal_store(cm[0], q.mq + i0);
        __builtin_nontemporal_store(cs[0], q.sq + i0);
      } else {
        q.mq[i0] = cm[0];
        q.sq[i0] = cs[0];
      }
    } else {
      *reinterpret_cast<uint2*>(q.mq + i0) = uint2{cm[0], cm[1]};
      *reinterpret_cast<uint2*>(q.sq + i0) = uint2{cs[0], cs[1]};
    }
    if (r == 0) {
      q.mscale[blk] = a_m / 448.f;
      q.sscale[blk] = a_s / 448.f;
    }
  }
}

}  // namespace

hipError_t adam8_step(float* param, float* grad, uint8_t* mq, uint8_t* sq, float* mscale, float* sscale,
                      uint16_t* shadow, const float* hp, float grad_scale, Adam8Params ap, int64_t n, uint64_t seed,
                      int64_t base, hipStream_t s, const float* clip, const float* prox_anchor, const float* prox_hdr,
                      bool wide) {
  if (n <= 0) return hipSuccess;
  if (n % 64 || base % 64 || base < 0) return hipErrorInvalidValue;
  if ((prox_anchor != nullptr) != (prox_hdr != nullptr)) return hipErrorInvalidValue;
  const Adam8Args q{reinterpret_cast<uint32_t*>(mq), reinterpret_cast<uint32_t*>(sq), mscale, sscale, seed, base};
  with_clip(clip, [&](auto ca) {
    with_prox(prox_anchor, prox_hdr, [&](auto pa) {
      // (the grid rule of the other updates: one float4 per thread up to the cap; wide: two)
      if (wide)
        adam8_kernel<true, decltype(ca)::on, decltype(pa)::on, 2><<<grid_for(n / 8), kBlock, 0, s>>>(
            param, grad, q, shadow, hp, grad_scale, ap, n, ca, pa);
      else
        adam8_kernel<true, decltype(ca)::on, decltype(pa)::on, 1><<<grid_for(n / 4), kBlock, 0, s>>>(
            param, grad, q, shadow, hp, grad_scale, ap, n, ca, pa);
    });
  });
  return hipGetLastError();
}

}  // namespace ldnn
