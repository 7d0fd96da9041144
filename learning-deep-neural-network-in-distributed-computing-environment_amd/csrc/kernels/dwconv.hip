// Depthwise 3x3 convolution (groups == channels, multiplier 1, padding 1, stride 1 or 2) on dense
// NHWC bf16 activations [N][H][W][Cp], fp32 accumulation: forward, input gradient, weight gradient.
//
//   y[n,p,q,c] = sum_{r,s} x[n, p*st + r - 1, q*st + s - 1, c] * w[c,r,s]
//
// There is no reduction across channels, so these are bandwidth kernels without matrix instructions:
// every activation byte should cross HBM once per pass.
//
// Weights: a [C,1,3,3] parameter lives in the KRSC storage as [Cp][3][3][8] with the tap in element
// 0 of the inner 8 (the other seven are padding and stay zero).  The kernels read the bf16 shadow
// with that stride and the weight gradient goes to the same positions of the fp32 gradient storage.
//
// Work split (all three kernels): 256 threads = 8 channel lanes (one 16-byte vector of 8 channels
// each: 64 channels, 128 contiguous bytes per pixel) x 32 pixel lanes.  Output rows are flattened
// over (n, p), so a tile of TR rows takes rows of several images at the small stages.  A pixel lane
// owns one flattened row and a run of RUN neighbouring output columns; the tile is TR x TC outputs
// with TC = RUN * (column groups).  The input halo tile is staged once into LDS with 16-byte loads;
// positions outside the image or beyond Cp are staged as zeros, so the inner loops have no bounds
// tests.  Input rows carry one zero row above and below each image in the tile's row numbering
// ("padded flat rows", IHp = IH + 2 per image), which makes the halo of a tile that crosses an image
// boundary one contiguous row range.  The host picks TR so that the tile fits kDwMaxPx pixels.
//
// Along its run a thread reads each input column's three rows once and feeds them to every output
// of the run they belong to (fp32 accumulators), so an LDS element is read once per tap row.
//
// The stride-2 input gradient gathers: a dx pixel of row parity a and column parity b receives
// 1, 2 or 4 taps (even/even: w[1][1]; odd rows: w[2][.] from dy row h>>1 and w[0][.] from the next),
// chosen per thread (rows) and at compile time along the run (columns).  Nothing is scattered.
//
// The weight gradient keeps 8 channels x 9 taps of fp32 sums per thread over a slice of the row
// tiles, reduces the 32 pixel lanes in a fixed order (butterfly inside a wave, then the four waves
// through LDS) and stores one partial [9][Cp] per slice with plain stores; a second small launch
// sums the slices in a fixed order (four interleaved groups, then the groups in order) and stores
// into or adds onto the gradient storage.  dy has no reuse and is read straight from HBM.  No
// floating-point atomics: a shape has one summation order.
#include "ldnn_common.h"
#include "ldnn_fastdiv.h"
#include "ldnn_kernels.h"

namespace ldnn {
namespace {

using convlds::FastDiv;
using convlds::fdiv;
using convlds::make_fastdiv;

constexpr int kDwBlock = 256;
constexpr int kDwCB = 64;        // channels per workgroup
constexpr int kDwMaxPx = 320;    // LDS tile: pixels of 128 bytes (40 KiB; three workgroups per CU)
constexpr int kDwSliceTarget = 512;   // wgrad: workgroups aimed at

struct DwGeo {
  int N, OH, OW, IH, IW, IHp, Cp;   // out [N][OH][OW][Cp], in [N][IH][IW][Cp], IHp = IH + 2
  int NR;                           // N * OH flattened output rows
  int TR, TC, cg_log2, LC;          // tile rows / columns, log2(column groups), LDS tile columns
  int ntr, ntc, ncb;                // row tiles, column tiles, channel blocks
  FastDiv d_oh, d_ihp, d_lc, d_ntc;
};

template <int STRIDE, bool DGRAD>
struct DwCfg {
  static constexpr bool kDg2 = DGRAD && STRIDE == 2;
  static constexpr int kSt = DGRAD ? 1 : STRIDE;           // input columns per output column of the gather
  static constexpr int kRun = (STRIDE == 2 && !DGRAD) ? 2 : 4;
  static constexpr int kTapRows = kDg2 ? 2 : 3;
  static constexpr int kMaxCg = 4;
};

// Padded flat input row of the first tap row of flattened output row R.
template <int STRIDE, bool DGRAD>
__host__ __device__ __forceinline__ int dw_in_row(int R, const DwGeo& g) {
  const int n = fdiv(R, g.d_oh), o = R - n * g.OH;
  if constexpr (DwCfg<STRIDE, DGRAD>::kDg2) return n * g.IHp + (o >> 1) + 1;
  else return n * g.IHp + o * DwCfg<STRIDE, DGRAD>::kSt;
}

template <int STRIDE, bool DGRAD>
DwGeo dw_geometry(int N, int OH, int OW, int IH, int IW, int Cp) {
  using K = DwCfg<STRIDE, DGRAD>;
  DwGeo g{};
  g.N = N, g.OH = OH, g.OW = OW, g.IH = IH, g.IW = IW, g.IHp = IH + 2, g.Cp = Cp;
  g.NR = N * OH;
  g.d_oh = make_fastdiv(OH);
  g.d_ihp = make_fastdiv(g.IHp);
  const int runs = (OW + K::kRun - 1) / K::kRun;
  int cg = 1;
  while (cg < runs && cg < K::kMaxCg) cg *= 2, ++g.cg_log2;
  g.TC = K::kRun * cg;
  g.LC = K::kDg2 ? g.TC / 2 + 1 : (g.TC - 1) * K::kSt + 3;
  g.d_lc = make_fastdiv(g.LC);
  // the most rows whose halo fits the LDS tile at every tile start (the phases repeat every OH tiles)
  for (g.TR = 32 / cg; g.TR > 1; --g.TR) {
    const int nt = (g.NR + g.TR - 1) / g.TR;
    bool ok = true;
    for (int k = 0; k < nt && k < OH && ok; ++k) {
      const int R0 = k * g.TR, Rl = (R0 + g.TR < g.NR ? R0 + g.TR : g.NR) - 1;
      ok = (dw_in_row<STRIDE, DGRAD>(Rl, g) + K::kTapRows - dw_in_row<STRIDE, DGRAD>(R0, g)) * g.LC <= kDwMaxPx;
    }
    if (ok) break;
  }
  g.ntr = (g.NR + g.TR - 1) / g.TR;
  g.ntc = (OW + g.TC - 1) / g.TC;
  g.ncb = (Cp + kDwCB - 1) / kDwCB;
  g.d_ntc = make_fastdiv(g.ntc);
  return g;
}

__device__ __forceinline__ void dw_unpack(const u32x4& raw, float (&f)[8]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f[2 * i] = __uint_as_float(raw[i] << 16);
    f[2 * i + 1] = __uint_as_float(raw[i] & 0xffff0000u);
  }
}

__device__ __forceinline__ u32x4 dw_pack(const float (&f)[8]) {
  u32x4 o;
#pragma unroll
  for (int i = 0; i < 4; ++i) o[i] = (uint32_t)f2bf(f[2 * i]) | ((uint32_t)f2bf(f[2 * i + 1]) << 16);
  return o;
}

// Stage the input halo tile: `span` padded flat rows from G0, g.LC columns from input column col0,
// this workgroup's 64 channels.  tile[(row * LC + col) * 8 + channel lane]; zeros outside.
__device__ __forceinline__ void dw_stage(const bf16_t* __restrict__ in, u32x4* tile, const DwGeo& g, int G0, int span,
                                         int col0, int ch, int tid) {
  const int v = tid & 7;
  const bool chok = ch < g.Cp;
  int npx = span * g.LC;
  npx = npx < kDwMaxPx ? npx : kDwMaxPx;   // (the host sized TR for this: never clipped)
  for (int px = tid >> 3; px < npx; px += kDwBlock / 8) {
    const int lr = fdiv(px, g.d_lc), lc = px - lr * g.LC;
    const int gr = G0 + lr;
    const int n = fdiv(gr, g.d_ihp), ih = gr - n * g.IHp - 1, ic = col0 + lc;
    u32x4 val = {0u, 0u, 0u, 0u};
    if (chok && n < g.N && (unsigned)ih < (unsigned)g.IH && (unsigned)ic < (unsigned)g.IW)
      val = *reinterpret_cast<const u32x4*>(in + (((int64_t)n * g.IH + ih) * g.IW + ic) * g.Cp + ch);
    tile[px * 8 + v] = val;
  }
}

// The channel block's 9 x 64 taps as fp32, tap-major; FLIP: rotated by 180 degrees (stride-1 dgrad).
template <bool FLIP>
__device__ __forceinline__ void dw_stage_w(const bf16_t* __restrict__ w, float* wl, int cb, int Cp, int tid) {
  for (int i = tid; i < 9 * kDwCB; i += kDwBlock) {
    const int t = i / kDwCB, c = cb * kDwCB + i % kDwCB;
    wl[i] = c < Cp ? bf2f(w[(int64_t)c * 72 + (FLIP ? 8 - t : t) * 8]) : 0.f;
  }
}

// Forward (DGRAD = false: in = x, out = y) and input gradient (DGRAD = true: in = dy, out = dx).
// grid (row tiles * column tiles, channel blocks).
template <int STRIDE, bool DGRAD>
__global__ __launch_bounds__(kDwBlock) void dwconv3x3_kernel(const bf16_t* __restrict__ in,
                                                            const bf16_t* __restrict__ w,
                                                            const float* __restrict__ bias, int relu,
                                                            bf16_t* __restrict__ out, DwGeo g) {
  using K = DwCfg<STRIDE, DGRAD>;
  constexpr int RUN = K::kRun, ST = K::kSt;
  __shared__ u32x4 tile[kDwMaxPx * 8];
  __shared__ float wl[9 * kDwCB];
  const int tid = threadIdx.x, v = tid & 7, pl = tid >> 3;
  const int rt = fdiv((int)blockIdx.x, g.d_ntc), ct = (int)blockIdx.x - rt * g.ntc;
  const int cb = blockIdx.y, ch = cb * kDwCB + v * 8;
  const int R0 = rt * g.TR, c0 = ct * g.TC;
  const int Rl = (R0 + g.TR < g.NR ? R0 + g.TR : g.NR) - 1;
  const int G0 = dw_in_row<STRIDE, DGRAD>(R0, g);
  const int span = dw_in_row<STRIDE, DGRAD>(Rl, g) + K::kTapRows - G0;
  dw_stage_w<DGRAD && STRIDE == 1>(w, wl, cb, g.Cp, tid);
  dw_stage(in, tile, g, G0, span, K::kDg2 ? c0 >> 1 : c0 * ST - 1, ch, tid);
  __syncthreads();

  const int cgi = pl & ((1 << g.cg_log2) - 1), ri = pl >> g.cg_log2;
  const int R = R0 + ri, oc0 = c0 + cgi * RUN;
  if (ri >= g.TR || R > Rl || oc0 >= g.OW || ch >= g.Cp) return;   // (no barrier below)

  float wr[9][8];
#pragma unroll
  for (int t = 0; t < 9; ++t) {
    const floatx4 a = *reinterpret_cast<const floatx4*>(wl + t * kDwCB + v * 8);
    const floatx4 b = *reinterpret_cast<const floatx4*>(wl + t * kDwCB + v * 8 + 4);
#pragma unroll
    for (int j = 0; j < 4; ++j) wr[t][j] = a[j], wr[t][4 + j] = b[j];
  }
  float acc[RUN][8];
#pragma unroll
  for (int k = 0; k < RUN; ++k)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[k][j] = (!DGRAD && bias) ? bias[ch + j] : 0.f;

  const int lr = dw_in_row<STRIDE, DGRAD>(R, g) - G0;
  if constexpr (!K::kDg2) {
    constexpr int NCOL = (RUN - 1) * ST + 3;
    const u32x4* src = tile + ((int64_t)lr * g.LC + cgi * RUN * ST) * 8 + v;
#pragma unroll
    for (int cc = 0; cc < NCOL; ++cc) {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        float xv[8];
        dw_unpack(src[(r * g.LC + cc) * 8], xv);
#pragma unroll
        for (int k = 0; k < RUN; ++k) {
          const int s = cc - k * ST;
          if (s >= 0 && s <= 2) {
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[k][j] = fmaf(xv[j], wr[r * 3 + s][j], acc[k][j]);
          }
        }
      }
    }
  } else {
    // dx row h: dy row h >> 1 with w[2 or 1][.], and for odd h the next dy row with w[0][.]
    const int n = fdiv(R, g.d_oh), hodd = (R - n * g.OH) & 1;
    float w0[3][8], w1[3][8];
#pragma unroll
    for (int s = 0; s < 3; ++s)
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        w0[s][j] = hodd ? wr[6 + s][j] : wr[3 + s][j];
        w1[s][j] = hodd ? wr[s][j] : 0.f;
      }
    const u32x4* s0 = tile + ((int64_t)lr * g.LC + ((cgi * RUN) >> 1)) * 8 + v;
    const u32x4* s1 = s0 + hodd * g.LC * 8;
    // dx columns w0 + {0, 1, 2, 3} (w0 even) from dy columns j0 + {0, 1, 2}: even columns take
    // tap column 1 of their dy column, odd ones tap column 2 of the left and 0 of the right one
#pragma unroll
    for (int jj = 0; jj < RUN / 2 + 1; ++jj) {
      float d0[8], d1[8];
      dw_unpack(s0[jj * 8], d0);
      dw_unpack(s1[jj * 8], d1);
#pragma unroll
      for (int k = 0; k < RUN; ++k) {
        const int s = (k & 1) ? (2 * jj == k - 1 ? 2 : (2 * jj == k + 1 ? 0 : -1)) : (2 * jj == k ? 1 : -1);
        if (s >= 0) {
#pragma unroll
          for (int j = 0; j < 8; ++j) acc[k][j] = fmaf(d1[j], w1[s][j], fmaf(d0[j], w0[s][j], acc[k][j]));
        }
      }
    }
  }

  bf16_t* dst = out + ((int64_t)R * g.OW + oc0) * g.Cp + ch;
#pragma unroll
  for (int k = 0; k < RUN; ++k) {
    if (oc0 + k < g.OW) {
      if (!DGRAD && relu) {
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[k][j] = fmaxf(acc[k][j], 0.f);
      }
      *reinterpret_cast<u32x4*>(dst + (int64_t)k * g.Cp) = dw_pack(acc[k]);
    }
  }
}

// Weight gradient partials: part[slice][9][Cp].  grid (slices, channel blocks); a slice takes
// `tps` row tiles (forward geometry: out = dy, in = x) and every column tile.
template <int STRIDE>
__global__ __launch_bounds__(kDwBlock) void dwconv3x3_wgrad_kernel(const bf16_t* __restrict__ x,
                                                                  const bf16_t* __restrict__ dy,
                                                                  float* __restrict__ part, DwGeo g, int tps) {
  using K = DwCfg<STRIDE, false>;
  constexpr int RUN = K::kRun, ST = K::kSt, NCOL = (RUN - 1) * ST + 3;
  __shared__ u32x4 tile[kDwMaxPx * 8];
  __shared__ float red[4 * 9 * kDwCB];
  const int tid = threadIdx.x, v = tid & 7, pl = tid >> 3;
  const int cb = blockIdx.y, ch = cb * kDwCB + v * 8;
  const int cgi = pl & ((1 << g.cg_log2) - 1), ri = pl >> g.cg_log2;
  float acc[9][8];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[t][j] = 0.f;

  const int rt_end = ((int)blockIdx.x + 1) * tps < g.ntr ? ((int)blockIdx.x + 1) * tps : g.ntr;
  for (int rt = (int)blockIdx.x * tps; rt < rt_end; ++rt) {
    const int R0 = rt * g.TR;
    const int Rl = (R0 + g.TR < g.NR ? R0 + g.TR : g.NR) - 1;
    const int G0 = dw_in_row<STRIDE, false>(R0, g);
    const int span = dw_in_row<STRIDE, false>(Rl, g) + 3 - G0;
    const int R = R0 + ri;
    const int lr = dw_in_row<STRIDE, false>(R <= Rl ? R : Rl, g) - G0;
    for (int ct = 0; ct < g.ntc; ++ct) {
      const int c0 = ct * g.TC, oc0 = c0 + cgi * RUN;
      __syncthreads();   // (the previous tile's readers are done)
      dw_stage(x, tile, g, G0, span, c0 * ST - 1, ch, tid);
      __syncthreads();
      if (ri < g.TR && R <= Rl && oc0 < g.OW && ch < g.Cp) {
        float gv[RUN][8];
        const bf16_t* gp = dy + ((int64_t)R * g.OW + oc0) * g.Cp + ch;
#pragma unroll
        for (int k = 0; k < RUN; ++k) {
          u32x4 raw = {0u, 0u, 0u, 0u};
          if (oc0 + k < g.OW) raw = *reinterpret_cast<const u32x4*>(gp + (int64_t)k * g.Cp);
          dw_unpack(raw, gv[k]);
        }
        const u32x4* src = tile + ((int64_t)lr * g.LC + cgi * RUN * ST) * 8 + v;
#pragma unroll
        for (int cc = 0; cc < NCOL; ++cc) {
#pragma unroll
          for (int r = 0; r < 3; ++r) {
            float xv[8];
            dw_unpack(src[(r * g.LC + cc) * 8], xv);
#pragma unroll
            for (int k = 0; k < RUN; ++k) {
              const int s = cc - k * ST;
              if (s >= 0 && s <= 2) {
#pragma unroll
                for (int j = 0; j < 8; ++j) acc[r * 3 + s][j] = fmaf(gv[k][j], xv[j], acc[r * 3 + s][j]);
              }
            }
          }
        }
      }
    }
  }

  // the 8 pixel lanes of a wave (lane bits 3..5), then the four waves in order
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float a = acc[t][j];
      a += __shfl_xor(a, 8, 64);
      a += __shfl_xor(a, 16, 64);
      a += __shfl_xor(a, 32, 64);
      acc[t][j] = a;
    }
  if ((tid & 63) < 8) {
    float* dst = red + (tid >> 6) * 9 * kDwCB + v * 8;
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int j = 0; j < 8; ++j) dst[t * kDwCB + j] = acc[t][j];
  }
  __syncthreads();
  for (int i = tid; i < 9 * kDwCB; i += kDwBlock) {
    const int t = i / kDwCB, c = cb * kDwCB + i % kDwCB;
    if (c < g.Cp)
      part[((int64_t)blockIdx.x * 9 + t) * g.Cp + c] =
          ((red[i] + red[9 * kDwCB + i]) + red[2 * 9 * kDwCB + i]) + red[3 * 9 * kDwCB + i];
  }
}

// dw storage [Cp][9][8] (tap in element 0) = or += the slices' sum, in slice order.  A storing pass
// writes the whole 8-wide position (zeros beside the tap, and for the pad channels C .. Cp-1).
__global__ __launch_bounds__(kDwBlock) void dwconv_wgrad_finalize_kernel(const float* __restrict__ part,
                                                                        float* __restrict__ dw, int slices, int Cp,
                                                                        int C, int accumulate) {
  // 64 (tap, channel) elements per workgroup; four wave-sized groups take every fourth slice each
  // (independent loads in flight), then their sums are added in group order
  __shared__ float red[4][64];
  const int e = threadIdx.x & 63, sg = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + e;
  const bool ok = i < 9 * Cp;
  float sum = 0.f;
  if (ok) {
#pragma unroll 4
    for (int s = sg; s < slices; s += 4) sum += part[(int64_t)s * 9 * Cp + i];
  }
  red[sg][e] = sum;
  __syncthreads();
  if (sg != 0 || !ok) return;
  sum = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
  const int t = i / Cp, c = i - t * Cp;
  if (c >= C) sum = 0.f;
  float* dst = dw + (int64_t)c * 72 + t * 8;
  if (accumulate) {
    dst[0] += sum;
  } else {
    *reinterpret_cast<floatx4*>(dst) = floatx4{sum, 0.f, 0.f, 0.f};
    *reinterpret_cast<floatx4*>(dst + 4) = floatx4{0.f, 0.f, 0.f, 0.f};
  }
}

bool dw_shape_ok(int64_t N, int64_t H, int64_t W, int64_t Cp, int stride) {
  if (N < 1 || H < 1 || W < 1 || Cp < 8 || Cp % 8 != 0 || (stride != 1 && stride != 2)) return false;
  // flattened (padded) rows, tile counts and the tap storage index stay in int32; channel blocks in grid.y
  return N * (H + 2) < INT32_MAX && N * (H + 2) * ((W + 3) / 4) < INT32_MAX && Cp <= 65535 * kDwCB;
}

bool dw_aligned(const void* a, const void* b, const void* c) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c)) & 15) == 0;
}

int dw_slices(const DwGeo& g, int* tps) {
  const int want = kDwSliceTarget / g.ncb > 0 ? kDwSliceTarget / g.ncb : 1;
  *tps = (g.ntr + want - 1) / want;
  return (g.ntr + *tps - 1) / *tps;
}

DwGeo dw_fwd_geometry(int N, int H, int W, int Cp, int stride) {
  const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1;
  return stride == 1 ? dw_geometry<1, false>(N, P, Q, H, W, Cp) : dw_geometry<2, false>(N, P, Q, H, W, Cp);
}

}  // namespace

int64_t dwconv_workspace_floats(int64_t N, int64_t H, int64_t W, int64_t Cp, int stride) {
  if (!dw_shape_ok(N, H, W, Cp, stride)) return -1;
  int tps;
  return (int64_t)dw_slices(dw_fwd_geometry((int)N, (int)H, (int)W, (int)Cp, stride), &tps) * 9 * Cp;
}

hipError_t dwconv_forward(const uint16_t* x, const uint16_t* w, const float* bias, bool relu, uint16_t* y, int64_t N,
                          int64_t H, int64_t W, int64_t Cp, int stride, hipStream_t s) {
  if (!dw_shape_ok(N, H, W, Cp, stride) || !x || !w || !y || !dw_aligned(x, y, nullptr)) return hipErrorInvalidValue;
  const DwGeo g = dw_fwd_geometry((int)N, (int)H, (int)W, (int)Cp, stride);
  const dim3 grid((unsigned)(g.ntr * g.ntc), (unsigned)g.ncb);
  if (stride == 1) dwconv3x3_kernel<1, false><<<grid, kDwBlock, 0, s>>>(x, w, bias, relu ? 1 : 0, y, g);
  else dwconv3x3_kernel<2, false><<<grid, kDwBlock, 0, s>>>(x, w, bias, relu ? 1 : 0, y, g);
  return hipGetLastError();
}

hipError_t dwconv_dgrad(const uint16_t* dy, const uint16_t* w, uint16_t* dx, int64_t N, int64_t H, int64_t W,
                        int64_t Cp, int stride, hipStream_t s) {
  if (!dw_shape_ok(N, H, W, Cp, stride) || !dy || !w || !dx || !dw_aligned(dy, dx, nullptr))
    return hipErrorInvalidValue;
  const int P = (int)((H - 1) / stride + 1), Q = (int)((W - 1) / stride + 1);
  const DwGeo g = stride == 1 ? dw_geometry<1, true>((int)N, (int)H, (int)W, P, Q, (int)Cp)
                              : dw_geometry<2, true>((int)N, (int)H, (int)W, P, Q, (int)Cp);
  const dim3 grid((unsigned)(g.ntr * g.ntc), (unsigned)g.ncb);
  if (stride == 1) dwconv3x3_kernel<1, true><<<grid, kDwBlock, 0, s>>>(dy, w, nullptr, 0, dx, g);
  else dwconv3x3_kernel<2, true><<<grid, kDwBlock, 0, s>>>(dy, w, nullptr, 0, dx, g);
  return hipGetLastError();
}

hipError_t dwconv_wgrad(const uint16_t* x, const uint16_t* dy, float* ws, float* dw, int64_t C, bool accumulate,
                        int64_t N, int64_t H, int64_t W, int64_t Cp, int stride, hipStream_t s) {
  if (!dw_shape_ok(N, H, W, Cp, stride) || !x || !dy || !ws || !dw || C < 1 || C > Cp || !dw_aligned(x, dy, dw))
    return hipErrorInvalidValue;
  const DwGeo g = dw_fwd_geometry((int)N, (int)H, (int)W, (int)Cp, stride);
  int tps;
  const int slices = dw_slices(g, &tps);
  const dim3 grid((unsigned)slices, (unsigned)g.ncb);
  if (stride == 1) dwconv3x3_wgrad_kernel<1><<<grid, kDwBlock, 0, s>>>(x, dy, ws, g, tps);
  else dwconv3x3_wgrad_kernel<2><<<grid, kDwBlock, 0, s>>>(x, dy, ws, g, tps);
  dwconv_wgrad_finalize_kernel<<<(unsigned)((9 * Cp + 63) / 64), kDwBlock, 0, s>>>(
      ws, dw, slices, (int)Cp, (int)C, accumulate ? 1 : 0);
  return hipGetLastError();
}

}  // namespace ldnn
