// FP8 NT GEMM on the gfx950 f8f6f4 matrix instruction: C[M, N] = epi(alpha * A[M, K] . B[N, K]^T).
//
// Both operands are K-contiguous fp8 codes as quant_f8.hip's f8_cast_transpose wrote them: rows and K
// padded to 128 with code 0, so no load is masked and the K loop has no tail; only the epilogue masks
// rows >= M and columns >= N.  A is e4m3 or e5m2 (template), B always e4m3.  alpha = (1 / s_a)(1 / s_b) is
// read from the two operands' device scale words (a power of two, or NaN when an operand was not finite).
//
// Work split: 256 threads, a 128 x 128 output tile, K steps of 128 bytes.  Each of the four waves owns
// 64 x 64 of the tile as 2 x 2 accumulators of v_mfma_scale_f32_32x32x64_f8f6f4 (scale words 1.0): 64
// accumulator registers, 8 MFMAs per wave and K step.
// Data movement: a K step's operand tiles (2 x 128 rows x 128 B) are fetched a step ahead with 16-byte
// global loads into registers (8 per thread) and written to the other half of a double-buffered LDS image
// (2 x 2 x 128 x 144 B = 72 KiB) after the current step's MFMAs were issued, so one barrier per K step
// suffices.  The LDS row stride is 128 + 16 bytes: the 32-byte fragment reads (two ds_read_b128 per lane)
// of 16 consecutive rows then cover all 64 banks.
// Fragments: lane l reads row (l & 31), bytes [32 (l >> 5), +32) of a 64-byte K sub-step for A and for B
// alike, so the two operands' K elements pair up whatever the instruction's internal K order is.  The
// B tile (the weights in the forward) is the instruction's first operand and the A tile its second: the
// accumulator register r of lane l is then C[m = l & 31][n = 8 (r >> 2) + 4 (l >> 5) + (r & 3)], four
// consecutive columns per lane, which the epilogue parks in LDS with 16-byte writes.
// Epilogue: every wave stages its fp32 64 x 64 block in LDS (row stride 68 floats, over the operand
// image, which is free by then) and re-reads it row-wise, so output stores are whole 128-B (bf16) or
// 256-B (fp32) row runs.  bf16: act(alpha * acc + bias[n]); fp32: beta * C + alpha * acc (the weight
// gradient, straight into the flat gradient buffer).
#include "ldnn_gemm_tile.h"

namespace ldnn {
namespace {

typedef int v8i32 __attribute__((ext_vector_type(8)));
typedef int v4i32 __attribute__((ext_vector_type(4)));

constexpr int kF8Tile = 128;            // output tile edge and K step (bytes)
constexpr int kF8Row = kF8Tile + 16;    // LDS row stride
constexpr int kF8Op = kF8Tile * kF8Row; // one operand tile
constexpr int kF8Stage = 2 * kF8Op;     // A + B
constexpr int kF8CRow = 68;             // staged fp32 row stride (floats)
constexpr int kF8One = 0x7f7f7f7f;      // E8M0 scale 1.0 in every byte
static_assert(4 * 64 * kF8CRow * 4 <= 2 * kF8Stage, "the epilogue staging fits the operand image");

__device__ __forceinline__ v8i32 f8_frag(const char* tile, int row, int ks, int lane) {
  const char* p = tile + row * kF8Row + ks * 64 + (lane >> 5) * 32;
  const v4i32 lo = *reinterpret_cast<const v4i32*>(p);
  const v4i32 hi = *reinterpret_cast<const v4i32*>(p + 16);
  return v8i32{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

template <int AFMT, int EPI, bool OUT_F32>
__global__ __launch_bounds__(256) void gemm_f8_kernel(GemmF8Params p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kF8Stage];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  int m0, n0;
  tile_coords(p.M, p.N, kF8Tile, kF8Tile, m0, n0);

  // staging map: thread t moves 16-byte chunk (t & 7) of rows (t >> 3) + 32 i, i = 0..3, of both tiles
  const int lrow = tid >> 3, lkc = (tid & 7) * 16;
  const uint8_t* ga = p.A + (size_t)(m0 + lrow) * p.lda + lkc;
  const uint8_t* gb = p.B + (size_t)(n0 + lrow) * p.ldb + lkc;
  u32x4 ra[4], rb[4];
  auto gload = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = *reinterpret_cast<const u32x4*>(ga + (size_t)(32 * i) * p.lda + (size_t)kt * kF8Tile);
      rb[i] = *reinterpret_cast<const u32x4*>(gb + (size_t)(32 * i) * p.ldb + (size_t)kt * kF8Tile);
    }
  };
  auto lstore = [&](char* st) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<u32x4*>(st + (lrow + 32 * i) * kF8Row + lkc) = ra[i];
      *reinterpret_cast<u32x4*>(st + kF8Op + (lrow + 32 * i) * kF8Row + lkc) = rb[i];
    }
  };

  floatx16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int nk = p.K / kF8Tile;
  gload(0);
  lstore(smem);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const char* cur = smem + (kt & 1) * kF8Stage;
    const bool more = kt + 1 < nk;
    if (more) gload(kt + 1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      v8i32 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa[i] = f8_frag(cur, wm * 64 + i * 32 + (lane & 31), ks, lane);
        fb[i] = f8_frag(cur + kF8Op, wn * 64 + i * 32 + (lane & 31), ks, lane);
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fb[j], fa[i], acc[i][j], 0, AFMT, 0, kF8One,
                                                                      0, kF8One);
    }
    // the other half was last read in step kt - 1, which every wave left through the barrier below
    if (more) lstore(smem + ((kt + 1) & 1) * kF8Stage);
    __syncthreads();
  }

  // ---- epilogue: stage the wave's 64 x 64 block, re-read it row-wise ----
  float* wbuf = reinterpret_cast<float*>(smem) + wid * 64 * kF8CRow;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int row = i * 32 + (lane & 31);
        const int col = j * 32 + 8 * g + 4 * (lane >> 5);
        *reinterpret_cast<floatx4*>(wbuf + row * kF8CRow + col) =
            floatx4{acc[i][j][4 * g], acc[i][j][4 * g + 1], acc[i][j][4 * g + 2], acc[i][j][4 * g + 3]};
      }
  __syncthreads();
  const float alpha = p.a_words[2] * p.b_words[2];
  constexpr int CPL = OUT_F32 ? 4 : 8;  // columns per lane: one 16-byte store
  constexpr int LPR = 64 / CPL;         // lanes per row
  const int col = (lane % LPR) * CPL;
  const int n = n0 + wn * 64 + col;
  if (n >= p.N) return;  // N % 8 == 0 (host): a lane's columns are inside or outside as a whole
  float bias[CPL];
#pragma unroll
  for (int q = 0; q < CPL; ++q) bias[q] = 0.f;
  if constexpr (EPI == EPI_BIAS || EPI == EPI_BIAS_RELU || EPI == EPI_BIAS_SIGMOID) {
#pragma unroll
    for (int q = 0; q < CPL; q += 4) {
      const floatx4 b = *reinterpret_cast<const floatx4*>(p.bias + n + q);
      bias[q] = b[0]; bias[q + 1] = b[1]; bias[q + 2] = b[2]; bias[q + 3] = b[3];
    }
  }
#pragma unroll 4
  for (int it = 0; it < LPR; ++it) {  // 64 / LPR rows per pass, 64 rows: LPR passes
    const int row = it * (64 / LPR) + lane / LPR;
    const int m = m0 + wm * 64 + row;
    if (m >= p.M) continue;
    float v[CPL];
#pragma unroll
    for (int q = 0; q < CPL; q += 4) {
      const floatx4 t = *reinterpret_cast<const floatx4*>(wbuf + row * kF8CRow + col + q);
      v[q] = t[0]; v[q + 1] = t[1]; v[q + 2] = t[2]; v[q + 3] = t[3];
    }
    if constexpr (OUT_F32) {
      float* c = reinterpret_cast<float*>(p.C) + (size_t)m * p.ldc + n;
      floatx4 o = floatx4{v[0], v[1], v[2], v[3]} * alpha;
      if (p.beta != 0.f) o = p.beta * *reinterpret_cast<const floatx4*>(c) + o;
      *reinterpret_cast<floatx4*>(c) = o;
    } else {
      u16x8 o;
#pragma unroll
      for (int q = 0; q < 8; ++q) o[q] = f2bf(apply_epi<EPI>(alpha * v[q], bias[q], 0.f));
      *reinterpret_cast<u16x8*>(reinterpret_cast<bf16_t*>(p.C) + (size_t)m * p.ldc + n) = o;
    }
  }
}

template <int AFMT>
hipError_t launch(const GemmF8Params& p, int epi, bool out_f32, dim3 grid, hipStream_t s) {
  if (out_f32) {
    if (epi != EPI_NONE) return hipErrorInvalidValue;
    gemm_f8_kernel<AFMT, EPI_NONE, true><<<grid, 256, 0, s>>>(p);
  } else {
    switch (epi) {
      case EPI_NONE: gemm_f8_kernel<AFMT, EPI_NONE, false><<<grid, 256, 0, s>>>(p); break;
      case EPI_BIAS: gemm_f8_kernel<AFMT, EPI_BIAS, false><<<grid, 256, 0, s>>>(p); break;
      case EPI_BIAS_RELU: gemm_f8_kernel<AFMT, EPI_BIAS_RELU, false><<<grid, 256, 0, s>>>(p); break;
      case EPI_BIAS_SIGMOID: gemm_f8_kernel<AFMT, EPI_BIAS_SIGMOID, false><<<grid, 256, 0, s>>>(p); break;
      default: return hipErrorInvalidValue;
    }
  }
  return hipGetLastError();
}

}  // namespace

hipError_t gemm_f8(const GemmF8Params& p, int a_fmt, int epi, bool out_f32, hipStream_t s) {
  if (p.M < 1 || p.N < 1 || p.N % 8 != 0 || p.K < kF8Tile || p.K % kF8Tile != 0 || p.lda < p.K || p.ldb < p.K ||
      p.lda % 16 != 0 || p.ldb % 16 != 0 || p.ldc % 8 != 0 || p.ldc < p.N)
    return hipErrorInvalidValue;
  const int tiles = ((p.M + kF8Tile - 1) / kF8Tile) * ((p.N + kF8Tile - 1) / kF8Tile);
  const dim3 grid(tiles);
  if (a_fmt == 0) return launch<0>(p, epi, out_f32, grid, s);
  if (a_fmt == 1) return launch<1>(p, epi, out_f32, grid, s);
  return hipErrorInvalidValue;
}

}  // namespace ldnn
