// Squeeze-and-Excitation (Hu et al. 2018) over dense NHWC bf16 activations [N][P][C] (P = H * W
// pixels, C % 8 == 0), with the block's residual add and ReLU fused into the scaling pass, forward
// and backward.  Arithmetic is fp32; the four parameters are read from the fp32 master storage
// (W1 [Chp][C], b1 [Chp], W2 [C][Chp], b2 [C], Chp = Ch rounded up to 8: a few hundred KB at most,
// they stay in L2, no bf16 copy is involved) and their gradients go into the fp32 gradient storage.
//
//     z[n][c] = mean_p u[n][p][c]
//     h[n][:] = relu(W1 z[n][:] + b1)                     Ch hidden units
//     s[n][:] = sigmoid(W2 h[n][:] + b2)
//     y       = relu?(s[n][c] * u (+ r))
//     g       = dy * relu'(y)
//     ds[n][c] = sum_p g * u,  da2 = ds * s * (1 - s),  dh[j] = (sum_c W2[c][j] da2[c]) * (h[j] > 0),
//     dz[c]   = (sum_j W1[j][c] dh[j]) / P
//     du      = g * s[n][c] + dz[n][c],  dres = g
//     dW2[c][j] = sum_n da2[n][c] h[n][j],  db2 = sum_n da2,  dW1[j][c] = sum_n dh[n][j] z[n][c],
//     db1 = sum_n dh
//
// Five launches per block and step, no atomics and no hand-off between workgroups, so every output
// and gradient is the same bits on every run:
//   se_gate / se_bwd_gate   one 256-thread workgroup per sample.  A lane owns one 8-channel vector
//                           column (16-B loads); C/8 lanes cover a pixel, 256 / (C/8) pixels are in
//                           flight per sweep, C/8 > 256 loops over column chunks.  Per-channel sums
//                           stay in fp32 registers and the pixel lanes of a column are summed
//                           through LDS (8 x 256 floats) in a fixed order into an LDS vector of C
//                           floats (z, or ds turned into da2).  The two tiny FCs then run out of
//                           LDS: FC1 one wave per hidden unit with float4 loads of the W1 row and a
//                           wave reduction, FC2 one thread per channel over its contiguous W2 row;
//                           the backward's W2^T product splits c over the four waves (lanes = hidden
//                           units, coalesced) and sums the four parts through LDS, its W1^T product
//                           is one thread per channel (coalesced over c).  LDS: 2 x 16 KiB vectors +
//                           8 KiB of reduction scratch.
//   se_apply / se_bwd_apply streaming passes over all N * P * C/8 vectors, 16-B loads and stores,
//                           four vectors per thread; grid (blocks per sample, N), so a thread's
//                           sample is its blockIdx.y and the gate vectors are 2 float4 loads.
//   se_wgrad                one launch for the four parameter gradients: a thread owns 4 neighbouring
//                           elements of one gradient and contracts the batch in order (one scalar and
//                           one float4 load per sample); each parameter is stored or added as asked,
//                           pad rows / columns of the padded storage get exactly 0 on a store.
// No matrix instruction: the per-sample FCs are matrix-vector products of at most 1024 x 64 and the
// batch contraction of the weight gradients is 64 to 256 long; the cost is the two sweeps over the
// activation.  One workgroup per sample is kept for every shape: splitting a sample over several
// workgroups (for N far below the CU count with large images) has not been measured, so it is not
// done.
//
// Buffers of one call, fp32, nothing to zero:  gate  = z [N][C] | s [N][C] | h [N][Chp]  (forward
// -> backward),  ws = da2 [N][C] | dz [N][C] | dh [N][Chp]  (within the backward).  The ReLU bit
// mask has bn_fwd's layout: byte (element offset / 8), bit j = channel c0 + j is > 0.
#include "ldnn_common.h"
#include "ldnn_kernels.h"

namespace ldnn {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / kWave;
constexpr int kMaxC = 4096;          // the LDS vectors of the gate kernels
constexpr int kApplyVecs = 4;        // vectors per thread of the streaming passes

struct SeGeo {
  int64_t N, P;
  int C, Ch, Chp;
  int V;        // vector columns, C / 8
  int lanes;    // vector columns per sweep, min(V, 256)
  int rl;       // pixel lanes, 256 / lanes
  int CB;       // column chunks, ceil(V / 256)
  int PV;       // vectors per sample, P * V
};

SeGeo se_geometry(const SeArgs& a) {
  SeGeo g;
  g.N = a.N, g.P = a.P, g.C = a.C, g.Ch = a.Ch, g.Chp = (a.Ch + 7) / 8 * 8;
  g.V = a.C / 8;
  g.lanes = g.V < kBlock ? g.V : kBlock;
  g.rl = kBlock / g.lanes;
  g.CB = (g.V + kBlock - 1) / kBlock;
  g.PV = (int)(a.P * g.V);
  return g;
}

__device__ __forceinline__ void ld8f(const float* __restrict__ p, float (&v)[8]) {
  const floatx4 a = *reinterpret_cast<const floatx4*>(p), b = *reinterpret_cast<const floatx4*>(p + 4);
  v[0] = a[0], v[1] = a[1], v[2] = a[2], v[3] = a[3];
  v[4] = b[0], v[5] = b[1], v[6] = b[2], v[7] = b[3];
}

// Per-channel sums over the pixels of sample n into out[C] (LDS):  FWD: sum u;  !FWD: sum g * u,
// g = dy masked by the forward's ReLU bits when MASK.  red: 8 * kBlock floats of LDS.  Ends with a
// barrier: out is complete for every thread.
template <bool FWD, bool MASK>
__device__ __forceinline__ void se_sweep(const bf16_t* __restrict__ u, const bf16_t* __restrict__ dy,
                                         const uint8_t* __restrict__ mask, int64_t n, const SeGeo& g,
                                         float* __restrict__ red, float* __restrict__ out) {
  const int tid = threadIdx.x, lane = tid % g.lanes, rlane = tid / g.lanes;
  const int64_t sample = n * g.P * g.C;
  for (int cb = 0; cb < g.CB; ++cb) {
    const int v = cb * kBlock + lane;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    if (rlane < g.rl && v < g.V) {
      const int64_t base = sample + (int64_t)v * 8;
#pragma unroll 4
      for (int64_t p = rlane; p < g.P; p += g.rl) {
        const int64_t o = base + p * g.C;
        const u16x8 uv = *reinterpret_cast<const u16x8*>(u + o);
        if constexpr (FWD) {
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] += bf2f(uv[j]);
        } else {
          const u16x8 gv = *reinterpret_cast<const u16x8*>(dy + o);
          uint32_t mb = 0xffu;
          if constexpr (MASK) mb = mask[o >> 3];
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[j] += ((mb >> j) & 1u) ? bf2f(gv[j]) * bf2f(uv[j]) : 0.f;
        }
      }
    }
    __syncthreads();   // (red of the previous chunk has been read)
#pragma unroll
    for (int j = 0; j < 8; ++j) red[j * kBlock + tid] = acc[j];
    __syncthreads();
    // red[k][rlane][lane]: the pixel lanes of a column are summed in the order of rlane
    const int cols = min(g.lanes, g.V - cb * kBlock);
    for (int i = tid; i < 8 * cols; i += kBlock) {
      const int k = i / cols, l = i - k * cols;
      float t = 0.f;
      for (int r = 0; r < g.rl; ++r) t += red[k * kBlock + r * g.lanes + l];
      out[(cb * kBlock + l) * 8 + k] = t;
    }
  }
  __syncthreads();
}

// One workgroup per sample: z, h, s of the sample into gate.
__global__ __launch_bounds__(kBlock) void se_gate_kernel(const bf16_t* __restrict__ u, const float* __restrict__ w1,
                                                         const float* __restrict__ b1, const float* __restrict__ w2,
                                                         const float* __restrict__ b2, float* __restrict__ gate,
                                                         SeGeo g) {
  __shared__ __attribute__((aligned(16))) float zs[kMaxC];
  __shared__ __attribute__((aligned(16))) float hs[kMaxC];
  __shared__ float red[8 * kBlock];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t n = blockIdx.x;
  float* zo = gate + n * g.C;
  float* so = gate + (g.N + n) * g.C;
  float* ho = gate + 2 * g.N * g.C + n * g.Chp;
  se_sweep<true, false>(u, nullptr, nullptr, n, g, red, zs);
  const float inv = 1.f / (float)g.P;
  for (int c = tid; c < g.C; c += kBlock) {
    const float z = zs[c] * inv;
    zs[c] = z;
    zo[c] = z;
  }
  __syncthreads();
  // FC1: a wave per hidden unit, lanes stride over c with float4 loads of the W1 row
  for (int j = wave; j < g.Chp; j += kWaves) {
    float acc = 0.f;
    if (j < g.Ch) {
      const float* row = w1 + (int64_t)j * g.C;
#pragma unroll 4
      for (int c = lane * 4; c < g.C; c += kWave * 4) {
        const floatx4 w = *reinterpret_cast<const floatx4*>(row + c);
        const floatx4 z = *reinterpret_cast<const floatx4*>(zs + c);
        acc += w[0] * z[0] + w[1] * z[1] + w[2] * z[2] + w[3] * z[3];
      }
      acc = fmaxf(wave_sum(acc) + b1[j], 0.f);
    }
    if (lane == 0) {   // (the pad units j >= Ch are written as zeros)
      hs[j] = acc;
      ho[j] = acc;
    }
  }
  __syncthreads();
  // FC2: a thread per channel over its contiguous W2 row
  for (int c = tid; c < g.C; c += kBlock) {
    const float* row = w2 + (int64_t)c * g.Chp;
    float acc = b2[c];
    int j = 0;
#pragma unroll 4
    for (; j + 4 <= g.Ch; j += 4) {
      const floatx4 w = *reinterpret_cast<const floatx4*>(row + j);
      const floatx4 h = *reinterpret_cast<const floatx4*>(hs + j);
      acc += w[0] * h[0] + w[1] * h[1] + w[2] * h[2] + w[3] * h[3];
    }
    for (; j < g.Ch; ++j) acc += row[j] * hs[j];
    so[c] = 1.f / (1.f + __expf(-acc));
  }
}

// y = relu?(s[n][c] * u (+ res)), and the ReLU bits when MASK.  grid (ceil(PV / (256 * 4)), N).
template <bool RES, bool RELU, bool MASK>
__global__ __launch_bounds__(kBlock) void se_apply_kernel(const bf16_t* __restrict__ u, const bf16_t* __restrict__ res,
                                                          const float* __restrict__ gate, bf16_t* __restrict__ y,
                                                          uint8_t* __restrict__ mask, SeGeo g) {
  const int64_t n = blockIdx.y;
  const float* sn = gate + (g.N + n) * g.C;
  const int64_t sample = n * (int64_t)g.PV;   // in vectors
  const int first = blockIdx.x * (kBlock * kApplyVecs) + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kApplyVecs; ++k) {
    const int i = first + k * kBlock;
    if (i >= g.PV) break;
    const int64_t o = (sample + i) * 8;
    float s[8];
    ld8f(sn + (i % g.V) * 8, s);
    const u16x8 uv = *reinterpret_cast<const u16x8*>(u + o);
    u16x8 rv;
    if constexpr (RES) rv = *reinterpret_cast<const u16x8*>(res + o);
    u16x8 out;
    uint32_t mb = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = bf2f(uv[j]) * s[j];
      if constexpr (RES) f += bf2f(rv[j]);
      if constexpr (RELU) f = fmaxf(f, 0.f);
      out[j] = f2bf(f);
      if constexpr (MASK) mb |= (bf2f(out[j]) > 0.f ? 1u : 0u) << j;
    }
    *reinterpret_cast<u16x8*>(y + o) = out;
    if constexpr (MASK) mask[o >> 3] = (uint8_t)mb;
  }
}

// One workgroup per sample: da2, dh, dz of the sample into ws.
template <bool MASK>
__global__ __launch_bounds__(kBlock) void se_bwd_gate_kernel(const bf16_t* __restrict__ u, const bf16_t* __restrict__ dy,
                                                             const uint8_t* __restrict__ mask,
                                                             const float* __restrict__ w1, const float* __restrict__ w2,
                                                             const float* __restrict__ gate, float* __restrict__ ws,
                                                             SeGeo g) {
  __shared__ float da[kMaxC];
  __shared__ float dhs[kMaxC];
  __shared__ float red[8 * kBlock];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
  const int64_t n = blockIdx.x;
  const float* sn = gate + (g.N + n) * g.C;
  const float* hn = gate + 2 * g.N * g.C + n * g.Chp;
  float* da_o = ws + n * g.C;
  float* dz_o = ws + (g.N + n) * g.C;
  float* dh_o = ws + 2 * g.N * g.C + n * g.Chp;
  se_sweep<false, MASK>(u, dy, mask, n, g, red, da);
  for (int c = tid; c < g.C; c += kBlock) {
    const float s = sn[c], d = da[c] * s * (1.f - s);
    da[c] = d;
    da_o[c] = d;
  }
  __syncthreads();
  // dh = (W2^T da2) * (h > 0): lanes are hidden units (coalesced over a W2 row), the four waves
  // take c = wave, wave + 4, ...; the four parts are added in the order of the waves
  for (int jb = 0; jb < g.Chp; jb += kWave) {
    const int j = jb + lane;
    float acc = 0.f;
    if (j < g.Ch) {
#pragma unroll 8
      for (int c = wave; c < g.C; c += kWaves) acc += w2[(int64_t)c * g.Chp + j] * da[c];
    }
    red[tid] = acc;
    __syncthreads();
    if (wave == 0 && j < g.Chp) {
      float t = 0.f;
      if (j < g.Ch && hn[j] > 0.f) t = red[lane] + red[kWave + lane] + red[2 * kWave + lane] + red[3 * kWave + lane];
      dhs[j] = t;
      dh_o[j] = t;   // (the pad units j >= Ch are written as zeros)
    }
    __syncthreads();
  }
  // dz = (W1^T dh) / P: a thread per channel, coalesced over c
  const float inv = 1.f / (float)g.P;
  for (int c = tid; c < g.C; c += kBlock) {
    float acc = 0.f;
#pragma unroll 8
    for (int j = 0; j < g.Ch; ++j) acc += w1[(int64_t)j * g.C + c] * dhs[j];
    dz_o[c] = acc * inv;
  }
}

// du = g * s[n][c] + dz[n][c], dres = g (g = dy masked by the ReLU bits when MASK).  Grid as se_apply.
template <bool MASK>
__global__ __launch_bounds__(kBlock) void se_bwd_apply_kernel(const bf16_t* __restrict__ dy,
                                                              const uint8_t* __restrict__ mask,
                                                              const float* __restrict__ gate,
                                                              const float* __restrict__ ws, bf16_t* __restrict__ du,
                                                              bf16_t* __restrict__ dres, SeGeo g) {
  const int64_t n = blockIdx.y;
  const float* sn = gate + (g.N + n) * g.C;
  const float* dzn = ws + (g.N + n) * g.C;
  const int64_t sample = n * (int64_t)g.PV;
  const int first = blockIdx.x * (kBlock * kApplyVecs) + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kApplyVecs; ++k) {
    const int i = first + k * kBlock;
    if (i >= g.PV) break;
    const int64_t o = (sample + i) * 8;
    float s[8], dz[8];
    ld8f(sn + (i % g.V) * 8, s);
    ld8f(dzn + (i % g.V) * 8, dz);
    const u16x8 gv = *reinterpret_cast<const u16x8*>(dy + o);
    uint32_t mb = 0xffu;
    if constexpr (MASK) mb = mask[o >> 3];
    u16x8 out, og;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float f = ((mb >> j) & 1u) ? bf2f(gv[j]) : 0.f;
      out[j] = f2bf(f * s[j] + dz[j]);
      og[j] = f2bf(f);
    }
    *reinterpret_cast<u16x8*>(du + o) = out;
    if (dres) *reinterpret_cast<u16x8*>(dres + o) = og;
  }
}

__device__ __forceinline__ void se_put4(float* __restrict__ dst, floatx4 v, bool store) {
  floatx4* d = reinterpret_cast<floatx4*>(dst);
  *d = store ? v : *d + v;
}

// The four parameter gradients.  A thread owns 4 neighbouring elements of one of them (unit ranges
// in the order dW2, dW1, db2, db1) and sums the samples in order.  Pad rows / columns (hidden units
// >= Ch) are zeros on a store and left alone on an add.
__global__ __launch_bounds__(kBlock) void se_wgrad_kernel(const float* __restrict__ gate, const float* __restrict__ ws,
                                                          float* __restrict__ dw1, float* __restrict__ db1,
                                                          float* __restrict__ dw2, float* __restrict__ db2,
                                                          int store, SeGeo g) {
  const float* z = gate;
  const float* h = gate + 2 * g.N * g.C;
  const float* da2 = ws;
  const float* dh = ws + 2 * g.N * g.C;
  const int C = g.C, Chp = g.Chp, N = (int)g.N;
  const int uw = C * (Chp / 4), ub2 = C / 4, ub1 = Chp / 4;
  int t = blockIdx.x * kBlock + threadIdx.x;
  floatx4 acc = {0.f, 0.f, 0.f, 0.f};
  if (t < uw) {   // dW2[c][j .. j+3] = sum_n da2[n][c] * h[n][j .. j+3]
    const int c = t / (Chp / 4), j = (t - c * (Chp / 4)) * 4;
#pragma unroll 8
    for (int n = 0; n < N; ++n)
      acc += da2[(int64_t)n * C + c] * *reinterpret_cast<const floatx4*>(h + (int64_t)n * Chp + j);
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (j + q >= g.Ch) acc[q] = 0.f;
    if ((store & SE_STORE_W2) || j + 4 <= g.Ch) se_put4(dw2 + (int64_t)c * Chp + j, acc, store & SE_STORE_W2);
    else
      for (int q = 0; j + q < g.Ch; ++q) dw2[(int64_t)c * Chp + j + q] += acc[q];
    return;
  }
  t -= uw;
  if (t < uw) {   // dW1[j][c .. c+3] = sum_n dh[n][j] * z[n][c .. c+3]
    const int j = t / (C / 4), c = (t - j * (C / 4)) * 4;
    if (j < g.Ch) {
#pragma unroll 8
      for (int n = 0; n < N; ++n)
        acc += dh[(int64_t)n * Chp + j] * *reinterpret_cast<const floatx4*>(z + (int64_t)n * C + c);
      se_put4(dw1 + (int64_t)j * C + c, acc, store & SE_STORE_W1);
    } else if (store & SE_STORE_W1) {
      se_put4(dw1 + (int64_t)j * C + c, acc, true);
    }
    return;
  }
  t -= uw;
  if (t < ub2) {   // db2[c .. c+3] = sum_n da2[n][c .. c+3]
#pragma unroll 8
    for (int n = 0; n < N; ++n) acc += *reinterpret_cast<const floatx4*>(da2 + (int64_t)n * C + t * 4);
    se_put4(db2 + t * 4, acc, store & SE_STORE_B2);
    return;
  }
  t -= ub2;
  if (t < ub1) {   // db1[j .. j+3] = sum_n dh[n][j .. j+3] (dh's pad units are zeros)
#pragma unroll 8
    for (int n = 0; n < N; ++n) acc += *reinterpret_cast<const floatx4*>(dh + (int64_t)n * Chp + t * 4);
    if (store & SE_STORE_B1) {
      se_put4(db1 + t * 4, acc, true);
    } else {
      for (int q = 0; q < 4 && t * 4 + q < g.Ch; ++q) db1[t * 4 + q] += acc[q];
    }
  }
}

bool se_args_ok(const SeArgs& a) {
  if (a.u == nullptr || a.w1 == nullptr || a.w2 == nullptr || a.gate == nullptr) return false;
  if (a.N < 1 || a.N > 65535 || a.P < 1 || a.C < 8 || a.C % 8 != 0 || a.C > kMaxC) return false;
  if (a.Ch < 1 || a.Ch > a.C) return false;
  if (a.P > (INT32_MAX - kBlock * kApplyVecs) / (a.C / 8)) return false;   // (a sample's vector index is an int)
  return ((reinterpret_cast<uintptr_t>(a.u) | reinterpret_cast<uintptr_t>(a.y) |
           reinterpret_cast<uintptr_t>(a.residual) | reinterpret_cast<uintptr_t>(a.w1) |
           reinterpret_cast<uintptr_t>(a.w2) | reinterpret_cast<uintptr_t>(a.gate) |
           reinterpret_cast<uintptr_t>(a.ws)) & 15) == 0;
}

dim3 se_apply_grid(const SeGeo& g) {
  return dim3((unsigned)((g.PV + kBlock * kApplyVecs - 1) / (kBlock * kApplyVecs)), (unsigned)g.N);
}

}  // namespace

int se_max_channels() { return kMaxC; }

int64_t se_workspace_floats(int64_t N, int C, int Ch) { return N * (2 * (int64_t)C + (Ch + 7) / 8 * 8); }

hipError_t se_forward(const SeArgs& a, hipStream_t s) {
  if (!se_args_ok(a) || a.y == nullptr || a.b1 == nullptr || a.b2 == nullptr || (a.mask && !a.relu))
    return hipErrorInvalidValue;
  const SeGeo g = se_geometry(a);
  se_gate_kernel<<<(unsigned)a.N, kBlock, 0, s>>>(a.u, a.w1, a.b1, a.w2, a.b2, a.gate, g);
  const dim3 grid = se_apply_grid(g);
  if (a.residual) {
    if (a.mask) se_apply_kernel<true, true, true><<<grid, kBlock, 0, s>>>(a.u, a.residual, a.gate, a.y, a.mask, g);
    else if (a.relu) se_apply_kernel<true, true, false><<<grid, kBlock, 0, s>>>(a.u, a.residual, a.gate, a.y, nullptr, g);
    else se_apply_kernel<true, false, false><<<grid, kBlock, 0, s>>>(a.u, a.residual, a.gate, a.y, nullptr, g);
  } else {
    if (a.mask) se_apply_kernel<false, true, true><<<grid, kBlock, 0, s>>>(a.u, nullptr, a.gate, a.y, a.mask, g);
    else if (a.relu) se_apply_kernel<false, true, false><<<grid, kBlock, 0, s>>>(a.u, nullptr, a.gate, a.y, nullptr, g);
    else se_apply_kernel<false, false, false><<<grid, kBlock, 0, s>>>(a.u, nullptr, a.gate, a.y, nullptr, g);
  }
  return hipGetLastError();
}

hipError_t se_backward(const SeArgs& a, const uint16_t* dy, uint16_t* du, uint16_t* dres, float* dw1, float* db1,
                       float* dw2, float* db2, int store, hipStream_t s) {
  if (!se_args_ok(a) || a.ws == nullptr || dy == nullptr || du == nullptr || (a.relu != 0) != (a.mask != nullptr))
    return hipErrorInvalidValue;
  if (dw1 == nullptr || db1 == nullptr || dw2 == nullptr || db2 == nullptr) return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(du) | reinterpret_cast<uintptr_t>(dres) |
       reinterpret_cast<uintptr_t>(dw1) | reinterpret_cast<uintptr_t>(db1) | reinterpret_cast<uintptr_t>(dw2) |
       reinterpret_cast<uintptr_t>(db2)) & 15)
    return hipErrorInvalidValue;
  const SeGeo g = se_geometry(a);
  const dim3 grid = se_apply_grid(g);
  if (a.mask) {
    se_bwd_gate_kernel<true><<<(unsigned)a.N, kBlock, 0, s>>>(a.u, dy, a.mask, a.w1, a.w2, a.gate, a.ws, g);
    se_bwd_apply_kernel<true><<<grid, kBlock, 0, s>>>(dy, a.mask, a.gate, a.ws, du, dres, g);
  } else {
    se_bwd_gate_kernel<false><<<(unsigned)a.N, kBlock, 0, s>>>(a.u, dy, nullptr, a.w1, a.w2, a.gate, a.ws, g);
    se_bwd_apply_kernel<false><<<grid, kBlock, 0, s>>>(dy, nullptr, a.gate, a.ws, du, dres, g);
  }
  const int64_t units = 2 * (int64_t)g.C * (g.Chp / 4) + g.C / 4 + g.Chp / 4;
  se_wgrad_kernel<<<(unsigned)((units + kBlock - 1) / kBlock), kBlock, 0, s>>>(a.gate, a.ws, dw1, db1, dw2, db2, store,
                                                                                g);
  return hipGetLastError();
}

}  // namespace ldnn
