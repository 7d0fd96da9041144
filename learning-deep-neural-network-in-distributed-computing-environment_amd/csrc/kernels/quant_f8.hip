// FP8 quantisation for the fp8 Linear (gemm_f8.hip): per-tensor current scaling with a power-of-two
// scale, OCP e4m3fn (max 448) or e5m2 (max 57344).
//
//   amax = max |t| over the logical [R, C] tensor, taken over the fp32 BIT PATTERNS of |t| as unsigned
//          integers, so NaN > inf > every finite value and a non-finite element is never lost;
//   s    = 2^e, e the largest integer with amax * 2^e <= fmt_max, capped at 126 so that s and 1 / s are
//          both normal fp32 (amax == 0: s = 1; amax not finite: s = 1 / s = NaN);
//   code = the hardware convert's round-to-nearest-even of clamp(t * s, +-fmt_max).  t is bf16 and s a
//          power of two, so t * s is exact in fp32 and so is the dequantisation by 1 / s.
//
// words (device fp32 [4]) = {amax (its bits), s, 1 / s, 0}: nothing is read back on the host, so a captured
// step replays.  f8_amax is two launches: one thread clears words[0], then a grid-stride pass with 16-byte
// loads (four in flight per lane) reduces per wave (shuffles), per workgroup (LDS) and with at most one
// atomicMax per workgroup.  s and 1 / s are written by f8_cast_transpose, whose every workgroup derives them
// from words[0] (a last-workgroup finalize in the pass, as xent.hip's, was measured first: its counter and
// fences on one word serialised the workgroups, 41 us for 4096 x 4096 at 1024 workgroups, 70 us at 2048).
//
// f8_cast_transpose reads the source once and writes the row-major codes out[Rp, Cp] and the transposed
// codes out_t[Cp, Rp] (Rp, Cp: R, C rounded up to 128; the pad is written as code 0 here, there is no
// fill launch).  A workgroup of 256 threads takes a 64 x 64 tile: a thread converts 16 consecutive
// elements of one row with the packed converts (four codes per dword), stores them row-major with one
// 16-byte store, and parks them in LDS ([64][17] dwords: the odd dword stride spreads the column gather
// over the banks).  It then gathers the bytes of one source column over 16 rows and stores them as 16
// bytes of a row of out_t.
#include <algorithm>
#include "ldnn_common.h"
#include "ldnn_f8.h"
#include "ldnn_kernels.h"

namespace ldnn {
namespace {

constexpr int kAmaxThreads = 256;
constexpr int kAmaxMaxBlocks = 1024;

__global__ void f8_words_init_kernel(float* __restrict__ words) {
  words[0] = 0.f;
  words[1] = words[2] = __uint_as_float(0x7fc00000u);  // (NaN until f8_cast_transpose writes s and 1 / s)
  words[3] = 0.f;
}

__device__ __forceinline__ void f8_scale(uint32_t bits, float fmt_max, float& s, float& inv) {
  s = inv = 1.f;
  if (bits >= 0x7f800000u) {
    s = inv = __uint_as_float(0x7fc00000u);
  } else if (bits != 0u) {
    // amax = f * 2^ex with f in [0.5, 1); fmt_max = 0.875 * 2^q for both formats
    int ex, q;
    const float f = frexpf(__uint_as_float(bits), &ex);
    (void)frexpf(fmt_max, &q);
    int e = q - ex - (f > 0.875f ? 1 : 0);
    e = min(e, 126);
    s = ldexpf(1.f, e);
    inv = ldexpf(1.f, -e);
  }
}

__global__ __launch_bounds__(kAmaxThreads) void f8_amax_kernel(const bf16_t* __restrict__ src, int R, int C8,
                                                                int64_t ld, float* __restrict__ words) {
  __shared__ uint32_t part[kAmaxThreads / kWave];
  const int64_t total = (int64_t)R * C8;
  uint32_t m = 0u;
  // four independent 16-byte loads in flight per lane; a dense matrix (ld == C) is one run, without the divide
  const int64_t step = (int64_t)gridDim.x * kAmaxThreads;
  const bool dense = ld == (int64_t)C8 * 8;
  for (int64_t i = (int64_t)blockIdx.x * kAmaxThreads + threadIdx.x; i < total; i += 4 * step) {
    u16x8 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int64_t j = i + u * step;
      v[u] = u16x8{0, 0, 0, 0, 0, 0, 0, 0};
      if (j < total) {
        const int64_t r = dense ? 0 : j / C8;
        v[u] = *reinterpret_cast<const u16x8*>(src + r * ld + (j - r * C8) * 8);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int q = 0; q < 8; ++q) m = max(m, ((uint32_t)(v[u][q] & 0x7fffu)) << 16);
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, o, 64));
  if ((threadIdx.x & (kWave - 1)) == 0) part[threadIdx.x / kWave] = m;
  __syncthreads();
  if (threadIdx.x != 0) return;
#pragma unroll
  for (int w = 1; w < kAmaxThreads / kWave; ++w) m = max(m, part[w]);
  // (one atomic per workgroup at most: 1024 workgroups' atomics on one word cost more than the pass itself, and
  // a stale read only means an atomic that was not needed)
  uint32_t* w0 = reinterpret_cast<uint32_t*>(words);
  if (m > __hip_atomic_load(w0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(w0, m);
}

constexpr int kCtTile = 64;
constexpr int kCtLds = 17;  // dwords per LDS row (16 + 1)

template <int FMT>
__global__ __launch_bounds__(256) void f8_cast_transpose_kernel(const bf16_t* __restrict__ src, int R, int C,
                                                                int64_t ld, float* __restrict__ words,
                                                                uint8_t* __restrict__ out,
                                                                uint8_t* __restrict__ out_t, int Rp, int Cp) {
  __shared__ uint32_t tile[kCtTile][kCtLds];
  constexpr float kMax = FMT == 0 ? 448.f : 57344.f;
  float s, inv;
  f8_scale(__float_as_uint(words[0]), kMax, s, inv);
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0) {
    words[1] = s;
    words[2] = inv;
  }
  const int r0 = blockIdx.y * kCtTile, c0 = blockIdx.x * kCtTile;
  const int tr = threadIdx.x >> 2, tq = threadIdx.x & 3;
  const int r = r0 + tr, c = c0 + tq * 16;
  u32x4 codes = {0u, 0u, 0u, 0u};
  if (r < R) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (c + h * 8 < C) {  // C % 8 == 0: an 8-element chunk is inside or outside as a whole
        const u16x8 v = *reinterpret_cast<const u16x8*>(src + (int64_t)r * ld + c + h * 8);
        float f[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) f[q] = clampf(bf2f(v[q]) * s, kMax);
        codes[2 * h] = cvt4<FMT>(f[0], f[1], f[2], f[3]);
        codes[2 * h + 1] = cvt4<FMT>(f[4], f[5], f[6], f[7]);
      }
    }
  }
  if (out != nullptr) *reinterpret_cast<u32x4*>(out + (int64_t)r * Cp + c) = codes;
  if (out_t == nullptr) return;
#pragma unroll
  for (int q = 0; q < 4; ++q) tile[tr][tq * 4 + q] = codes[q];
  __syncthreads();
  // out_t row (source column) c0 + tr, source rows r0 + tq * 16 .. + 15
  u32x4 t = {0u, 0u, 0u, 0u};
  const int sh = (tr & 3) * 8;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const uint32_t b = (tile[tq * 16 + j][tr >> 2] >> sh) & 0xffu;
    t[j >> 2] |= b << ((j & 3) * 8);
  }
  *reinterpret_cast<u32x4*>(out_t + (int64_t)(c0 + tr) * Rp + r0 + tq * 16) = t;
}

}  // namespace

hipError_t f8_amax(const uint16_t* src, int R, int C, int64_t ld, int fmt, float* words, hipStream_t s) {
  if (R < 1 || C < 8 || C % 8 != 0 || ld % 8 != 0 || (fmt != 0 && fmt != 1)) return hipErrorInvalidValue;
  const int64_t total = (int64_t)R * (C / 8);
  const int blocks = (int)std::min<int64_t>((total + kAmaxThreads - 1) / kAmaxThreads, kAmaxMaxBlocks);
  f8_words_init_kernel<<<1, 1, 0, s>>>(words);
  f8_amax_kernel<<<blocks, kAmaxThreads, 0, s>>>(src, R, C / 8, ld, words);
  return hipGetLastError();
}

hipError_t f8_cast_transpose(const uint16_t* src, int R, int C, int64_t ld, float* words, int fmt,
                             uint8_t* out, uint8_t* out_t, int Rp, int Cp, hipStream_t s) {
  if (R < 1 || C < 8 || C % 8 != 0 || ld % 8 != 0 || Rp % 128 != 0 || Cp % 128 != 0 || Rp < R || Cp < C ||
      (fmt != 0 && fmt != 1))
    return hipErrorInvalidValue;
  if (out == nullptr && out_t == nullptr) return hipSuccess;
  const dim3 grid(Cp / kCtTile, Rp / kCtTile);
  if (fmt == 0) f8_cast_transpose_kernel<0><<<grid, 256, 0, s>>>(src, R, C, ld, words, out, out_t, Rp, Cp);
  else f8_cast_transpose_kernel<1><<<grid, 256, 0, s>>>(src, R, C, ld, words, out, out_t, Rp, Cp);
  return hipGetLastError();
}

}  // namespace ldnn
