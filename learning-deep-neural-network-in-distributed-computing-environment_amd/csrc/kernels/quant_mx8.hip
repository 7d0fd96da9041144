// MXFP8 quantisation for the mxfp8 Linear (gemm_f8.hip with MX): OCP-MX style block scaling, OCP e4m3fn (max 448)
// or e5m2 (max 57344) codes, one E8M0 scale byte per block of 32.
//
//   block = 32 consecutive elements along the contraction dimension of the GEMM that consumes the codes:
//           the row-major copy of a [R, C] source is blocked along C, the transposed copy [C, R] along R.
//           The transposed copy is quantised from the bf16 source with scales of its own; it is NOT the
//           transpose of the row-major codes.
//   amax  = max |t| over the block's logical elements, taken over the BIT PATTERNS of |t| as unsigned
//           integers, so NaN > inf > every finite value;
//   e     = the largest integer with amax * 2^e <= fmt_max (f8_scale's rule, not the OCP floor rule: nothing
//           saturates), clamped to [-127, 127]; amax == 0: e = 0.  With amax = (1 + m / 128) 2^(E - 127) (bf16
//           fields E >= 1, m) and fmt_max = 1.75 * 2^q' that is e = q' - (E - 127) - (m > 96); a bf16 subnormal
//           amax always clamps to 127;
//   byte  = 127 - e, the E8M0 code of 2^-e, by which the matrix instruction multiplies the block's codes.  bf16
//           inputs give bytes in [0, 247];
//   code  = the hardware convert's round-to-nearest-even of t * 2^e (|t| 2^e <= fmt_max by the choice of e, so
//           the recipe's clamp to +-fmt_max never binds).  t is bf16 and 2^e a power of two: wherever the
//           product is a normal fp32 it is exact, and where it is not the code is 0 either way.
//   a block whose amax is not finite: the format's NaN code (0x7f in both formats) in every logical element
//           and byte 127 (an E8M0 byte of 255 is not relied on).
//   padding: both extents are padded to 128; pad elements are code 0, pad blocks byte 127, and a block cut by
//           the logical edge takes its amax over the logical elements only.
//
// Layout: codes uint8 [Rp][Cp], scales uint8 [Rp][Cp / 32] (the four scales of one 128-byte K step of a row
// are one aligned dword); the transposed pair [Cp][Rp] and [Cp][Rp / 32].
//
// One launch, one read of the source, no whole-tensor amax, no atomic.  A workgroup of 256 threads takes a
// 64 x 64 tile, which holds two whole blocks per row and per column.
// Row direction: thread (tr = t >> 2, tq = t & 3) holds the 16 elements [16 tq, +16) of tile row tr in
// registers; the block amax is one exchange with the neighbouring lane (tq ^ 1); convert, one 16-byte store of
// codes; the tq == 0 lane of a row fetches the second block's byte from lane + 2 and stores the row's two
// scale bytes as one 16-bit word.
// Column direction: the tile's bf16 VALUES are parked in LDS (not the row-scaled codes: those carry the wrong
// scale for this orientation), [64][33] dwords of two: the odd row stride puts the four 16-row groups a wave
// gathers at banks 0 / 16 / 32 / 48 + (column / 2), so the column gather is conflict-free.  The same thread
// then walks 16 rows of tile column tr, reduces with lane tq ^ 1 to the 32-row block amax, converts down the
// column and stores 16 bytes of an out_t row, and its scale bytes as in the row direction.
#include "ldnn_common.h"
#include "ldnn_f8.h"
#include "ldnn_kernels.h"

namespace ldnn {
namespace {

// amax16: the bf16 bit pattern of the block's amax (sign cleared).  Returns e; bad: the block is not finite.
template <int FMT>
__device__ __forceinline__ int mx_exponent(uint32_t amax16, bool& bad) {
  constexpr int kQ = FMT == 0 ? 8 : 15;  // fmt_max = 1.75 * 2^kQ
  const int E = (int)(amax16 >> 7), m = (int)(amax16 & 0x7fu);
  bad = E == 0xff;
  if (amax16 == 0u || bad) return 0;
  if (E == 0) return 127;
  return min(kQ - (E - 127) - (m > 96 ? 1 : 0), 127);  // (>= -120: the lower clamp never binds for bf16)
}

// 16 bf16 values -> 16 codes at scale 2^e; `valid` marks the logical elements (the only ones a non-finite
// block turns into the NaN code)
template <int FMT>
__device__ __forceinline__ u32x4 mx_codes16(const uint16_t (&v)[16], int e, bool bad, uint32_t valid) {
  const float s = __uint_as_float((uint32_t)(e + 127) << 23);  // e in [-126, 127]: a normal fp32
  u32x4 codes;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    codes[q] = cvt4<FMT>(bf2f(v[4 * q]) * s, bf2f(v[4 * q + 1]) * s, bf2f(v[4 * q + 2]) * s, bf2f(v[4 * q + 3]) * s);
    if (bad) {
      uint32_t w = 0u;
#pragma unroll
      for (int b = 0; b < 4; ++b) w |= ((valid >> (4 * q + b)) & 1u) ? (0x7fu << (8 * b)) : 0u;
      codes[q] = w;
    }
  }
  return codes;
}

constexpr int kMxTile = 64;
constexpr int kMxLds = 33;  // dwords per LDS row (32 + 1)

template <int FMT>
__global__ __launch_bounds__(256) void mx8_quantize_kernel(const bf16_t* __restrict__ src, int R, int C, int64_t ld,
                                                           uint8_t* __restrict__ out, uint8_t* __restrict__ out_s,
                                                           uint8_t* __restrict__ out_t, uint8_t* __restrict__ out_ts,
                                                           int Rp, int Cp) {
  __shared__ uint32_t tile[kMxTile][kMxLds];
  const int r0 = blockIdx.y * kMxTile, c0 = blockIdx.x * kMxTile;
  const int tr = threadIdx.x >> 2, tq = threadIdx.x & 3;
  const int r = r0 + tr, c = c0 + tq * 16;
  uint16_t v[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) v[q] = 0;
  uint32_t valid = 0u;
  if (r < R) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (c + h * 8 < C) {  // C % 8 == 0: an 8-element chunk is inside or outside as a whole
        const u16x8 g = *reinterpret_cast<const u16x8*>(src + (int64_t)r * ld + c + h * 8);
#pragma unroll
        for (int q = 0; q < 8; ++q) v[h * 8 + q] = g[q];
        valid |= 0xffu << (8 * h);
      }
    }
  }
  if (out != nullptr) {
    uint32_t am = 0u;
#pragma unroll
    for (int q = 0; q < 16; ++q) am = max(am, (uint32_t)(v[q] & 0x7fffu));
    am = max(am, (uint32_t)__shfl_xor((int)am, 1, 64));
    bool bad;
    const int e = mx_exponent<FMT>(am, bad);
    *reinterpret_cast<u32x4*>(out + (int64_t)r * Cp + c) = mx_codes16<FMT>(v, e, bad, valid);
    const int e2 = __shfl_down(e, 2, 64);  // the row's second block (lanes tq == 2, 3)
    if (tq == 0)
      *reinterpret_cast<uint16_t*>(out_s + (int64_t)r * (Cp / 32) + c0 / 32) =
          (uint16_t)((127 - e) | ((127 - e2) << 8));
  }
  if (out_t == nullptr) return;
#pragma unroll
  for (int q = 0; q < 8; ++q) tile[tr][tq * 8 + q] = (uint32_t)v[2 * q] | ((uint32_t)v[2 * q + 1] << 16);
  __syncthreads();
  // out_t row (source column) c0 + tr, source rows r0 + 16 tq .. + 15
  uint16_t w[16];
  uint32_t am = 0u;
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    w[j] = (uint16_t)(tile[tq * 16 + j][tr >> 1] >> ((tr & 1) * 16));
    am = max(am, (uint32_t)(w[j] & 0x7fffu));
  }
  am = max(am, (uint32_t)__shfl_xor((int)am, 1, 64));
  // logical rows of this run (pad rows and pad columns hold 0 in the tile, so only a NaN block needs the mask)
  const int nrow = (c0 + tr < C) ? min(max(R - (r0 + tq * 16), 0), 16) : 0;
  bool bad;
  const int e = mx_exponent<FMT>(am, bad);
  *reinterpret_cast<u32x4*>(out_t + (int64_t)(c0 + tr) * Rp + r0 + tq * 16) =
      mx_codes16<FMT>(w, e, bad, (1u << nrow) - 1u);
  const int e2 = __shfl_down(e, 2, 64);
  if (tq == 0)
    *reinterpret_cast<uint16_t*>(out_ts + (int64_t)(c0 + tr) * (Rp / 32) + r0 / 32) =
        (uint16_t)((127 - e) | ((127 - e2) << 8));
}

}  // namespace

hipError_t mx8_quantize(const uint16_t* src, int R, int C, int64_t ld, int fmt, uint8_t* out, uint8_t* out_s,
                        uint8_t* out_t, uint8_t* out_ts, int Rp, int Cp, hipStream_t s) {
  if (R < 1 || C < 8 || C % 8 != 0 || ld % 8 != 0 || ld < C || Rp % 128 != 0 || Cp % 128 != 0 || Rp < R || Cp < C ||
      (fmt != 0 && fmt != 1) || (out == nullptr) != (out_s == nullptr) || (out_t == nullptr) != (out_ts == nullptr))
    return hipErrorInvalidValue;
  if (out == nullptr && out_t == nullptr) return hipSuccess;
  const dim3 grid(Cp / kMxTile, Rp / kMxTile);
  if (grid.y > 65535u) return hipErrorInvalidValue;
  if (fmt == 0) mx8_quantize_kernel<0><<<grid, 256, 0, s>>>(src, R, C, ld, out, out_s, out_t, out_ts, Rp, Cp);
  else mx8_quantize_kernel<1><<<grid, 256, 0, s>>>(src, R, C, ld, out, out_s, out_t, out_ts, Rp, Cp);
  return hipGetLastError();
}

}  // namespace ldnn
