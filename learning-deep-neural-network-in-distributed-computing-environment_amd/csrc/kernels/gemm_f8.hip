// FP8 NT GEMMs on the gfx950 f8f6f4 matrix instruction, one kernel template for both scaling schemes:
//   per-tensor (MX = false): C[M, N] = epi(alpha * A[M, K] . B[N, K]^T), alpha = (1 / s_a)(1 / s_b) read from the two
//     operands' device scale words (a power of two, or NaN when an operand was not finite);
//   block-scaled (MX = true): C[M, N] = epi(A[M, K] . B[N, K]^T), where every 32 consecutive K elements of a row of
//     A and of B carry one E8M0 scale byte (2^(byte - 127)).  There is no alpha: the scales go into
//     v_mfma_scale_f32_32x32x64_f8f6f4's scale operands, which the per-tensor path feeds 1.0.
//
// Both operands are K-contiguous fp8 codes as quant_f8.hip's f8_cast_transpose / quant_mx8.hip's mx8_quantize
// wrote them: rows and K padded to 128 with code 0 (MX: scale arrays [rows][K / 32], pad blocks 127), so no load is
// masked and the K loop has no tail; only the epilogue masks rows >= M and columns >= N.  A is e4m3 or e5m2
// (template), B always e4m3.
//
// Work split: 256 threads, a 128 x 128 output tile, K steps of 128 bytes.  Each of the four waves owns
// 64 x 64 of the tile as 2 x 2 accumulators of v_mfma_scale_f32_32x32x64_f8f6f4: 64 accumulator registers,
// 8 MFMAs per wave and K step.
// Data movement: a K step's operand tiles (2 x 128 rows x 128 B) are fetched a step ahead with 16-byte
// global loads into registers (8 per thread) and written to the other half of a double-buffered LDS image
// (2 x 2 x 128 x 144 B = 72 KiB) after the current step's MFMAs were issued, so one barrier per K step
// suffices.  The LDS row stride is 128 + 16 bytes: the fragment reads (two ds_read_b128 per lane) of 16
// consecutive rows then cover all 64 banks.
// Fragments, per-tensor: lane l reads row (l & 31), bytes [32 (l >> 5), +32) of a 64-byte K sub-step for A and
// for B alike, so the two operands' K elements pair up whatever the instruction's internal K order is.  The
// B tile (the weights in the forward) is the instruction's first operand and the A tile its second: the
// accumulator register r of lane l is then C[m = l & 31][n = 8 (r >> 2) + 4 (l >> 5) + (r & 3)], four
// consecutive columns per lane, which the epilogue parks in LDS with 16-byte writes.
// MX scales: a K step of an operand tile needs 128 rows x one dword (four blocks).  Threads 0..127 fetch A's row
// dwords and threads 128..255 B's, a step ahead like the codes (one more register), and write them into the
// 16 spare bytes of the row's LDS stride, at byte 128: the scales ride in the operand stages and share their
// barrier, and the image stays 72 KiB.
// MX fragments and scales, as the MI355X applies them (probed with one-hot operands and a different byte per
// block, then settled by tests/test_mxfp8_gpu.py's spread / one_block cases):
//   * the byte value means 2^(byte - 127), and NaN codes make exactly the output rows (columns) they belong to
//     NaN, also against code 0 in the other operand, with byte 127;
//   * of a lane's 32 operand bytes (8 registers), the first 16 are K elements [16 g, +16) of the 64-byte
//     sub-step and the last 16 are [32 + 16 g, +16), g = l >> 5, for the row l & 31: a lane does NOT hold one
//     MX block.  Block 0 of the sub-step (K 0..31) is the first 16 bytes of lanes l and l + 32, block 1 the
//     last 16 bytes of both;
//   * block b of row l & 31 takes its scale from the scale register of lane (l & 31) + 32 b, the byte op_sel
//     names (one selection per instruction, not per lane).
// The per-tensor fragment (32 contiguous bytes per lane, the same for both operands) pairs the right products
// but would put half of each block under the other block's scale.  So with MX lane l reads bytes [16 g, +16) and
// [32 + 16 g, +16) of sub-step ks of its row (still two ds_read_b128, 16 rows x 144 B still cover all 64 banks),
// and supplies the scale of block 2 ks + g: byte 2 ks + g of its row's dword, shifted down to position 0 by the
// lane itself, op_sel 0.  Operand order and accumulator layout are the per-tensor path's.
// Epilogue: every wave stages its fp32 64 x 64 block in LDS (row stride 68 floats, over the operand
// image, which is free by then) and re-reads it row-wise, so output stores are whole 128-B (bf16) or
// 256-B (fp32) row runs.  bf16: act(alpha * acc + bias[n]); fp32: beta * C + alpha * acc (the weight
// gradient, straight into the flat gradient buffer); MX: the same without alpha.
#include "ldnn_gemm_tile.h"

namespace ldnn {
namespace {

typedef int v8i32 __attribute__((ext_vector_type(8)));
typedef int v4i32 __attribute__((ext_vector_type(4)));

constexpr int kF8Tile = 128;            // output tile edge and K step (bytes)
constexpr int kF8Row = kF8Tile + 16;    // LDS row stride: 128 code bytes, (MX) the row's scale dword, 12 spare
constexpr int kF8Op = kF8Tile * kF8Row; // one operand tile
constexpr int kF8Stage = 2 * kF8Op;     // A + B
constexpr int kF8CRow = 68;             // staged fp32 row stride (floats)
constexpr int kF8One = 0x7f7f7f7f;      // E8M0 scale 1.0 in every byte
static_assert(4 * 64 * kF8CRow * 4 <= 2 * kF8Stage, "the epilogue staging fits the operand image");

template <bool MX>
__device__ __forceinline__ v8i32 f8_frag(const char* tile, int row, int ks, int lane) {
  const char* p = tile + row * kF8Row + ks * 64 + (lane >> 5) * (MX ? 16 : 32);
  const v4i32 lo = *reinterpret_cast<const v4i32*>(p);                   // MX: block 2 ks
  const v4i32 hi = *reinterpret_cast<const v4i32*>(p + (MX ? 32 : 16));  // MX: block 2 ks + 1
  return v8i32{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}

// apply_epi; with MX a ReLU that keeps a NaN (fmaxf drops it): a row that covered a non-finite block must stay
// non-finite through the fused activation, or the non-finite-step guard never sees it.
// (whether the per-tensor ReLU should keep a NaN too is a question of behaviour, left as it is here)
template <bool MX, int EPI>
__device__ __forceinline__ float f8_epi(float v, float bias) {
  if constexpr (MX && EPI == EPI_BIAS_RELU) {
    const float t = v + bias;
    return t < 0.f ? 0.f : t;
  }
  return apply_epi<EPI>(v, bias, 0.f);
}

template <bool MX, int AFMT, int EPI, bool OUT_F32>
__global__ __launch_bounds__(256) void gemm_f8_kernel(GemmF8Params p) {
  __shared__ __attribute__((aligned(16))) char smem[2 * kF8Stage];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid >> 1, wn = wid & 1;
  int m0, n0;
  tile_coords(p.M, p.N, kF8Tile, kF8Tile, m0, n0);

  // staging map: thread t moves 16-byte chunk (t & 7) of rows (t >> 3) + 32 i, i = 0..3, of both tiles, and (MX)
  // the scale dword of row (t & 127) of A (t < 128) or of B
  const int lrow = tid >> 3, lkc = (tid & 7) * 16;
  const uint8_t* ga = p.A + (size_t)(m0 + lrow) * p.lda + lkc;
  const uint8_t* gb = p.B + (size_t)(n0 + lrow) * p.ldb + lkc;
  const uint32_t* gs = nullptr;
  int soff = 0;
  if constexpr (MX) {
    const int srow = tid & 127;
    const int kblocks = p.K / 32;
    gs = reinterpret_cast<const uint32_t*>(
        tid < 128 ? p.a_scales + (size_t)(m0 + srow) * kblocks : p.b_scales + (size_t)(n0 + srow) * kblocks);
    soff = (tid < 128 ? 0 : kF8Op) + srow * kF8Row + kF8Tile;
  }
  u32x4 ra[4], rb[4];
  uint32_t rs;
  auto gload = [&](int kt) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      ra[i] = *reinterpret_cast<const u32x4*>(ga + (size_t)(32 * i) * p.lda + (size_t)kt * kF8Tile);
      rb[i] = *reinterpret_cast<const u32x4*>(gb + (size_t)(32 * i) * p.ldb + (size_t)kt * kF8Tile);
    }
    if constexpr (MX) rs = gs[kt];
  };
  auto lstore = [&](char* st) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      *reinterpret_cast<u32x4*>(st + (lrow + 32 * i) * kF8Row + lkc) = ra[i];
      *reinterpret_cast<u32x4*>(st + kF8Op + (lrow + 32 * i) * kF8Row + lkc) = rb[i];
    }
    if constexpr (MX) *reinterpret_cast<uint32_t*>(st + soff) = rs;
  };

  floatx16 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  const int sh = (lane >> 5) * 8;  // (MX) the block of a sub-step's pair whose scale byte this lane supplies
  const int nk = p.K / kF8Tile;
  gload(0);
  lstore(smem);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const char* cur = smem + (kt & 1) * kF8Stage;
    const bool more = kt + 1 < nk;
    if (more) gload(kt + 1);
    uint32_t sa[2] = {kF8One, kF8One}, sb[2] = {kF8One, kF8One};
    if constexpr (MX) {
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        sa[i] = *reinterpret_cast<const uint32_t*>(cur + (wm * 64 + i * 32 + (lane & 31)) * kF8Row + kF8Tile) >> sh;
        sb[i] = *reinterpret_cast<const uint32_t*>(cur + kF8Op + (wn * 64 + i * 32 + (lane & 31)) * kF8Row + kF8Tile) >>
                sh;
      }
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      v8i32 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        fa[i] = f8_frag<MX>(cur, wm * 64 + i * 32 + (lane & 31), ks, lane);
        fb[i] = f8_frag<MX>(cur + kF8Op, wn * 64 + i * 32 + (lane & 31), ks, lane);
      }
      const int ssh = MX ? 16 * ks : 0;  // (per-tensor: the constant 1.0 as it is)
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fb[j], fa[i], acc[i][j], 0, AFMT, 0,
                                                                      (int)(sb[j] >> ssh), 0, (int)(sa[i] >> ssh));
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
  float alpha = 1.f;
  if constexpr (!MX) alpha = p.a_words[2] * p.b_words[2];
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
    if constexpr (!MX) {
#pragma unroll
      for (int q = 0; q < CPL; ++q) v[q] = alpha * v[q];
    }
    if constexpr (OUT_F32) {
      float* c = reinterpret_cast<float*>(p.C) + (size_t)m * p.ldc + n;
      floatx4 o = floatx4{v[0], v[1], v[2], v[3]};
      if (p.beta != 0.f) o = p.beta * *reinterpret_cast<const floatx4*>(c) + o;
      *reinterpret_cast<floatx4*>(c) = o;
    } else {
      u16x8 o;
#pragma unroll
      for (int q = 0; q < 8; ++q) o[q] = f2bf(f8_epi<MX, EPI>(v[q], bias[q]));
      *reinterpret_cast<u16x8*>(reinterpret_cast<bf16_t*>(p.C) + (size_t)m * p.ldc + n) = o;
    }
  }
}

template <bool MX, int AFMT>
hipError_t launch(const GemmF8Params& p, int epi, bool out_f32, dim3 grid, hipStream_t s) {
  if (out_f32) {
    if (epi != EPI_NONE) return hipErrorInvalidValue;
    gemm_f8_kernel<MX, AFMT, EPI_NONE, true><<<grid, 256, 0, s>>>(p);
  } else {
    switch (epi) {
      case EPI_NONE: gemm_f8_kernel<MX, AFMT, EPI_NONE, false><<<grid, 256, 0, s>>>(p); break;
      case EPI_BIAS: gemm_f8_kernel<MX, AFMT, EPI_BIAS, false><<<grid, 256, 0, s>>>(p); break;
      case EPI_BIAS_RELU: gemm_f8_kernel<MX, AFMT, EPI_BIAS_RELU, false><<<grid, 256, 0, s>>>(p); break;
      case EPI_BIAS_SIGMOID: gemm_f8_kernel<MX, AFMT, EPI_BIAS_SIGMOID, false><<<grid, 256, 0, s>>>(p); break;
      default: return hipErrorInvalidValue;
    }
  }
  return hipGetLastError();
}

}  // namespace

hipError_t gemm_f8(const GemmF8Params& p, bool mx, int a_fmt, int epi, bool out_f32, hipStream_t s) {
  if (p.M < 1 || p.N < 1 || p.N % 8 != 0 || p.K < kF8Tile || p.K % kF8Tile != 0 || p.lda < p.K || p.ldb < p.K ||
      p.lda % 16 != 0 || p.ldb % 16 != 0 || p.ldc % 8 != 0 || p.ldc < p.N ||
      (mx ? p.a_scales == nullptr || p.b_scales == nullptr : p.a_words == nullptr || p.b_words == nullptr) ||
      (a_fmt != 0 && a_fmt != 1))
    return hipErrorInvalidValue;
  const int tiles = ((p.M + kF8Tile - 1) / kF8Tile) * ((p.N + kF8Tile - 1) / kF8Tile);
  const dim3 grid(tiles);
  if (mx) return a_fmt == 0 ? launch<true, 0>(p, epi, out_f32, grid, s) : launch<true, 1>(p, epi, out_f32, grid, s);
  return a_fmt == 0 ? launch<false, 0>(p, epi, out_f32, grid, s) : launch<false, 1>(p, epi, out_f32, grid, s);
}

}  // namespace ldnn
