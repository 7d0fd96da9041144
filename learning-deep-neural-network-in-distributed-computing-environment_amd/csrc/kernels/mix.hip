// Batch mixing (Mixup / CutMix, one plan per batch: data/mix.py) in ONE launch:
//   mixup :  out[i] = lam x[i] + (1 - lam) x[perm[i]]      (fp32 arithmetic, rounded once)
//   cutmix:  out[i] = x[perm[i]] inside the box, x[i] outside  (bit-exact copies)
// over a contiguous [B][C][H][W] fp32 / bf16 batch, plus the dense soft targets
//   q[i][c] = lam [c == y_i] + (1 - lam) [c == y_perm[i]]   (fp32, [B][ldq], pad columns 0)
// that the soft-target softmax cross-entropy (xent.hip) reads.
//
// Grid: (blocks per image) x (B + 1).  Row i < B of the grid streams image i with 16-B
// accesses (4 fp32 / 8 bf16 per lane; a scalar instance when an image's element count
// or a base pointer does not allow them); row B writes q, one float4 per thread -- every
// element of out and q has exactly one writer, nothing is atomic.  The grid is capped
// like the other streaming kernels (2048 workgroups, grid-stride beyond).
//
// CutMix reads only what it copies: a vector wholly outside the box loads x[i] alone, one
// wholly inside loads x[perm[i]] alone, one that straddles a box edge loads both.  The
// (h, w) of a vector's first element comes from two multiply-high divisions
// (ldnn_fastdiv.h); the rest of the vector walks on from there.
//
// Stores are plain.  Nontemporal stores of the mixed batch were measured too while both
// instances existed (profiles/r13): alone the pass was 2-6 % faster with them at 256 x 3 x
// 224 x 224, but the next kernel reads the batch straight back, and inside the graphed steps
// plain stores tied (EnhancedCNN b64) or won by 0.3 % (ResNet-18 b64).
//
// A perm entry outside [0, B) is read as the identity (no out-of-bounds read); a label
// outside [0, ncls) leaves its share of the row zero.
#include <algorithm>

#include "ldnn_common.h"
#include "ldnn_fastdiv.h"
#include "ldnn_kernels.h"

namespace ldnn {

namespace {

using convlds::FastDiv;
using convlds::fdiv;
using convlds::make_fastdiv;

constexpr int kBlock = 256;
constexpr int kMaxBlocks = 2048;

struct MixArgs {
  const void* x;
  void* out;
  const int64_t* perm;
  const int64_t* labels;
  float* q;
  int B, n, H, W, ldq;
  int cutmix;
  float lam;
  int y0, y1, x0, x1;
  FastDiv dW, dHW;
};

template <typename V>
__device__ __forceinline__ V blend(const V& a, const V& b, float lam, float oml);
template <>
__device__ __forceinline__ float blend<float>(const float& a, const float& b, float lam, float oml) {
  return lam * a + oml * b;
}
template <>
__device__ __forceinline__ uint16_t blend<uint16_t>(const uint16_t& a, const uint16_t& b, float lam, float oml) {
  return f2bf(lam * bf2f(a) + oml * bf2f(b));
}
template <>
__device__ __forceinline__ floatx4 blend<floatx4>(const floatx4& a, const floatx4& b, float lam, float oml) {
  floatx4 o;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = lam * a[j] + oml * b[j];
  return o;
}
template <>
__device__ __forceinline__ u16x8 blend<u16x8>(const u16x8& a, const u16x8& b, float lam, float oml) {
  u16x8 o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = f2bf(lam * bf2f(a[j]) + oml * bf2f(b[j]));
  return o;
}

template <typename V, int VEC>
__device__ __forceinline__ V pick(const V& a, const V& b, unsigned m) {
  if constexpr (VEC == 1) {
    return m ? b : a;
  } else {
    V o;
#pragma unroll
    for (int j = 0; j < VEC; ++j) o[j] = ((m >> j) & 1u) ? b[j] : a[j];
    return o;
  }
}

// V: the access type (float / uint16_t: scalar; floatx4 / u16x8: 16 B), VEC its element count
template <typename V, int VEC>
__global__ __launch_bounds__(kBlock) void batch_mix_kernel(MixArgs p) {
  const int i = blockIdx.y;
  const int64_t stride = (int64_t)gridDim.x * kBlock;
  const int64_t t0 = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  const float lam = p.lam, oml = 1.f - p.lam;
  if (i == p.B) {
    // the soft targets: one float4 (4 classes of one row) per thread
    const int g4 = p.ldq / 4;
    const int64_t total = (int64_t)p.B * g4;
    for (int64_t t = t0; t < total; t += stride) {
      const int r = (int)(t / g4), c0 = (int)(t - (int64_t)r * g4) * 4;
      int64_t pr = p.perm[r];
      if ((uint64_t)pr >= (uint64_t)p.B) pr = r;
      const int64_t ya = p.labels[r], yb = p.labels[pr];
      floatx4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t c = c0 + j;
        v[j] = (ya == yb) ? (c == ya ? 1.f : 0.f) : (c == ya ? lam : (c == yb ? oml : 0.f));
      }
      *reinterpret_cast<floatx4*>(p.q + (size_t)r * p.ldq + c0) = v;
    }
    return;
  }
  int64_t pi = p.perm[i];
  if ((uint64_t)pi >= (uint64_t)p.B) pi = i;
  const int nv = p.n / VEC;
  const V* a = reinterpret_cast<const V*>(p.x) + (size_t)i * nv;
  const V* b = reinterpret_cast<const V*>(p.x) + (size_t)pi * nv;
  V* o = reinterpret_cast<V*>(p.out) + (size_t)i * nv;
  if (!p.cutmix) {
    for (int64_t v = t0; v < nv; v += stride) o[v] = blend<V>(a[v], b[v], lam, oml);
    return;
  }
  const int HW = p.H * p.W;
  constexpr unsigned kAll = VEC == 32 ? 0xffffffffu : ((1u << VEC) - 1u);
  for (int64_t v = t0; v < nv; v += stride) {
    const int e = (int)v * VEC;
    const int rem = e - fdiv(e, p.dHW) * HW;
    int h = fdiv(rem, p.dW);
    int w = rem - h * p.W;
    unsigned m = 0;
#pragma unroll
    for (int j = 0; j < VEC; ++j) {
      m |= (unsigned)(h >= p.y0 && h < p.y1 && w >= p.x0 && w < p.x1) << j;
      if (++w == p.W) {
        w = 0;
        if (++h == p.H) h = 0;
      }
    }
    V r;
    if (m == 0) r = a[v];
    else if (m == kAll) r = b[v];
    else r = pick<V, VEC>(a[v], b[v], m);
    o[v] = r;
  }
}

template <typename V, int VEC>
hipError_t launch(const MixArgs& p, hipStream_t s) {
  // (blocks per image) x B image rows, capped at kMaxBlocks workgroups in all
  const int64_t nv = p.n / VEC;
  int64_t bpi = (nv + kBlock - 1) / kBlock;
  bpi = std::max<int64_t>(1, std::min<int64_t>(bpi, std::max(1, kMaxBlocks / p.B)));
  const dim3 grid((unsigned)bpi, (unsigned)p.B + 1);
  batch_mix_kernel<V, VEC><<<grid, kBlock, 0, s>>>(p);
  return hipGetLastError();
}

}  // namespace

hipError_t batch_mix(const void* x, void* out, bool is_f32, const int64_t* perm, const int64_t* labels, float* q,
                     int ldq, int B, int64_t n, int H, int W, bool cutmix, float lam, int y0, int y1, int x0, int x1,
                     hipStream_t s) {
  if (B < 0 || B > 65534 || H < 1 || W < 1 || n < (int64_t)H * W || n >= (int64_t)1 << 31 || n % ((int64_t)H * W) != 0)
    return hipErrorInvalidValue;
  if (ldq < 4 || ldq % 4 || (reinterpret_cast<uintptr_t>(q) & 15)) return hipErrorInvalidValue;
  if (!(lam >= 0.f && lam <= 1.f)) return hipErrorInvalidValue;  // (NaN too)
  if (y0 < 0 || y1 > H || x0 < 0 || x1 > W) return hipErrorInvalidValue;
  if (x == out || x == nullptr || out == nullptr || perm == nullptr || labels == nullptr) return hipErrorInvalidValue;
  if (B == 0) return hipSuccess;
  MixArgs p;
  p.x = x, p.out = out, p.perm = perm, p.labels = labels, p.q = q;
  p.B = B, p.n = (int)n, p.H = H, p.W = W, p.ldq = ldq;
  // an empty box is mixup's lam = 1: either way a copy of x[i]
  p.cutmix = cutmix || lam == 1.f;
  p.lam = lam;
  if (!cutmix) y0 = y1 = x0 = x1 = 0;
  p.y0 = y0, p.y1 = y1, p.x0 = x0, p.x1 = x1;
  p.dW = make_fastdiv((uint32_t)W), p.dHW = make_fastdiv((uint32_t)(H * W));
  const int vec = is_f32 ? 4 : 8;
  const bool vec_ok = n % vec == 0 && ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
  if (is_f32) return vec_ok ? launch<floatx4, 4>(p, s) : launch<float, 1>(p, s);
  return vec_ok ? launch<u16x8, 8>(p, s) : launch<uint16_t, 1>(p, s);
}

}  // namespace ldnn
