// Grouped 3x3 convolution on the matrix pipe: padding 1, stride 1 or 2, in_channels == out_channels == C,
// group width gw = C / groups in {8, 16, 32}; dense NHWC bf16 activations [N][H][W][C] (C % 8 == 0: no pad
// channels), fp32 accumulation: forward, input gradient, weight gradient.
//
//   y[n,p,q,k] = sum_{r,s} sum_{c in group(k)} x[n, p*st + r - 1, q*st + s - 1, c] * w[k][r][s][c - c0(k)]
//
// Weights: the KRSC storage [C][3][3][gw] of a [C, gw, 3, 3] parameter (bf16 shadow; the weight gradient
// goes to the fp32 gradient storage of the same layout).  For these widths the storage has no padding.
//
// Work split (forward and input gradient): a workgroup of 256 threads owns a slab of 64 channels (128
// contiguous bytes per pixel, whole groups only) x a tile of TR flattened output rows (n, p) x SW columns.
// Rows are dwconv.hip's padded flat rows (one zero row above and below each image), so a tile that crosses
// an image boundary is one row range and the 4x4 / 2x2 stages fill a tile from several images.  The input
// halo tile is staged once into LDS with 16-byte loads (zeros outside the image and beyond C; the 16-byte
// chunks of a pixel XOR-swizzled by the pixel index, so 8 neighbouring pixels' reads of one chunk spread
// over all banks); the inner loop has no bounds tests.
//
// MFMA roles (v_mfma_f32_16x16x32_bf16, D[4g + v][l16] in lane (g, l16) as in conv.hip's small-channel
// kernels): A = weights, 16 rows = 16 neighbouring channels of the slab, held in registers for the whole
// tile (all four 16-blocks x all taps: 144 VGPRs at gw 32, 80 below); B = 16 output pixels (a "set": SW
// columns x 16 / SW rows, SW a power of two <= 16, so narrow images still fill a set), one 16-byte LDS
// vector per lane = 8 consecutive channels of one tap of one pixel.  Contraction packing:
//   gw 32: one tap per MFMA, k-block g = channels 8g.. of the group; 9 MFMAs per 16x16 block, and one B
//          fragment feeds the group's two 16-blocks.
//   gw 16: two taps per MFMA (k-blocks 0,1 the first, 2,3 the second), 5 MFMAs, the last half zero.
//   gw 8:  runs as gw 16 with the two groups of a 16-block on a block diagonal (the off-diagonal weight
//          elements are zeros built while the fragments are made): 5 MFMAs, not the 3 a waste-free packing
//          would take.  Both MFMA operands are shared by the whole 16x16 block, and a 16-channel block
//          spans two groups with different input channels, so one instruction cannot serve four taps of
//          both.  These passes are bandwidth-bound at every width, and 5 is what gw 16 pays anyway.
// Each wave takes every fourth set and computes all 64 channels for it, so its epilogue is private: the
// accumulators (+ bias, ReLU) go as bf16 through a 2 KiB per-wave LDS stage and leave as 16-byte stores,
// 128 contiguous bytes per pixel.
//
// The slab's weights (64 x 9 x gw bf16, <= 36 KiB) are loaded once per workgroup with 16-byte loads into the
// LDS of the tile (before the tile), from which the A fragments are read as 16-byte vectors; the input
// gradient transposes each group's gw x gw block on its way into LDS -- no transposed shadow exists.
// Stride-1 dgrad is then the forward over dy with the taps rotated by 180 degrees.  The stride-2 dgrad gathers by parity class: a set is 16 dx pixels of one row and one column parity, and takes
// 1, 2 or 4 taps (gw 32) or 1, 1 or 2 MFMAs of tap pairs (gw <= 16), chosen per set at compile time.
//
// Weight gradient: dw[k][r][s][c] = sum_pix dy[pix][k] x[pix + tap][c]; pixels are the contraction.  x (halo
// tile) and dy (the tile's pixels, zeros outside) are staged in LDS pixel-major rows of 128 bytes and both
// read with ds_read_b64_tr_b16 as in conv_lds.hip's ring wgrad.  Wave w owns the out-channels 16w.. of the
// slab and their group's in-channels (two 16-blocks at gw 32), 9 taps: at most 72 accumulator registers.
// grid = (slices of the row tiles) x (slabs); a workgroup leaves one plain-store fp32 partial [64][9][gw]
// per slice in the workspace and a second launch sums the slices in a fixed order and stores or adds.
// No floating-point atomics: a shape has one summation order.
#include "ldnn_common.h"
#include "ldnn_fastdiv.h"
#include "ldnn_kernels.h"

namespace ldnn {
namespace {

using convlds::FastDiv;
using convlds::fdiv;
using convlds::make_fastdiv;

constexpr int kGcBlock = 256;
constexpr int kGcCB = 64;          // channels per workgroup
constexpr int kGcMaxPx = 320;      // LDS halo tile: pixels of 128 bytes (40 KiB)
constexpr int kGcMaxSlots = 256;   // wgrad: dy pixels per tile (32 KiB)
constexpr int kGcSliceTarget = 512;   // wgrad: workgroups aimed at

typedef __attribute__((address_space(3))) bf16x4 lds_b4;

struct GcGeo {
  int N, OH, OW, IH, IW, IHp, C;   // out [N][OH][OW][C], in [N][IH][IW][C], IHp = IH + 2
  int NR;                          // N * OH flattened output rows
  int TR, TC, swl, LC;             // tile rows / columns, log2(set width), LDS tile columns
  int ntr, ntc, ncb;               // row tiles, column tiles, channel slabs
  FastDiv d_oh, d_ihp, d_lc, d_ntc;
};

template <int STRIDE, bool DGRAD>
struct GcCfg {
  static constexpr bool kDg2 = DGRAD && STRIDE == 2;
  static constexpr int kSt = DGRAD ? 1 : STRIDE;   // input columns per output column of the gather
  static constexpr int kTapRows = kDg2 ? 2 : 3;
};

// Padded flat input row of the first tap row of flattened output row R.
template <int STRIDE, bool DGRAD>
__host__ __device__ __forceinline__ int gc_in_row(int R, const GcGeo& g) {
  const int n = fdiv(R, g.d_oh), o = R - n * g.OH;
  if constexpr (GcCfg<STRIDE, DGRAD>::kDg2) return n * g.IHp + (o >> 1) + 1;
  else return n * g.IHp + o * GcCfg<STRIDE, DGRAD>::kSt;
}

template <int STRIDE, bool DGRAD>
GcGeo gc_geometry(int N, int OH, int OW, int IH, int IW, int C) {
  using K = GcCfg<STRIDE, DGRAD>;
  GcGeo g{};
  g.N = N, g.OH = OH, g.OW = OW, g.IH = IH, g.IW = IW, g.IHp = IH + 2, g.C = C;
  g.NR = N * OH;
  g.d_oh = make_fastdiv(OH);
  g.d_ihp = make_fastdiv(g.IHp);
  g.swl = 4;
  if (!K::kDg2)
    while (g.swl > 0 && (1 << (g.swl - 1)) >= OW) --g.swl;
  const int SW = 1 << g.swl;
  g.TC = K::kDg2 ? 2 * SW : SW;   // a stride-2 dgrad set takes every second column
  g.LC = K::kDg2 ? SW + 1 : (SW - 1) * K::kSt + 3;
  g.d_lc = make_fastdiv(g.LC);
  // the most rows whose halo fits the LDS tile at every tile start (the phases repeat every OH tiles)
  const int trmax = (K::kDg2 || kGcMaxSlots / SW > 32) ? 32 : kGcMaxSlots / SW;
  for (g.TR = trmax; g.TR > 1; --g.TR) {
    const int nt = (g.NR + g.TR - 1) / g.TR;
    bool ok = true;
    for (int k = 0; k < nt && k < OH && ok; ++k) {
      const int R0 = k * g.TR, Rl = (R0 + g.TR < g.NR ? R0 + g.TR : g.NR) - 1;
      ok = (gc_in_row<STRIDE, DGRAD>(Rl, g) + K::kTapRows - gc_in_row<STRIDE, DGRAD>(R0, g)) * g.LC <= kGcMaxPx;
    }
    if (ok) break;
  }
  g.ntr = (g.NR + g.TR - 1) / g.TR;
  g.ntc = (OW + g.TC - 1) / g.TC;
  g.ncb = (C + kGcCB - 1) / kGcCB;
  g.d_ntc = make_fastdiv(g.ntc);
  return g;
}

// Stage the input halo tile: `span` padded flat rows from G0, g.LC columns from input column col0, this
// workgroup's 64 channels.  tile[(row * LC + col) * 8 + (chunk ^ (pixel & 7))]; zeros outside.
__device__ __forceinline__ void gc_stage(const bf16_t* __restrict__ in, u32x4* tile, const GcGeo& g, int G0, int span,
                                         int col0, int cb, int tid) {
  const int v = tid & 7, ch = cb * kGcCB + v * 8;
  const bool chok = ch < g.C;
  int npx = span * g.LC;
  npx = npx < kGcMaxPx ? npx : kGcMaxPx;   // (the host sized TR for this: never clipped)
  for (int px = tid >> 3; px < npx; px += kGcBlock / 8) {
    const int lr = fdiv(px, g.d_lc), lc = px - lr * g.LC;
    const int gr = G0 + lr;
    const int n = fdiv(gr, g.d_ihp), ih = gr - n * g.IHp - 1, ic = col0 + lc;
    u32x4 val = {0u, 0u, 0u, 0u};
    if (chok && n < g.N && (unsigned)ih < (unsigned)g.IH && (unsigned)ic < (unsigned)g.IW)
      val = *reinterpret_cast<const u32x4*>(in + (((int64_t)n * g.IH + ih) * g.IW + ic) * g.C + ch);
    tile[px * 8 + (v ^ (px & 7))] = val;
  }
}

// The weight tap (r * 3 + s) of half h of A fragment f; -1: a zero half.  KW 32: one tap per fragment.
// KW 16: two; the stride-2 dgrad pairs the taps that one parity class uses together (see gc_dg2_class).
template <int STRIDE, bool DGRAD, int KW>
__device__ constexpr int gc_frag_tap(int f, int h) {
  if (KW == 32) return (DGRAD && STRIDE == 1) ? 8 - f : f;
  if (DGRAD && STRIDE == 2) {
    constexpr int t[5][2] = {{4, -1}, {5, 3}, {7, 1}, {8, 6}, {2, 0}};
    return t[f][h];
  }
  const int t = 2 * f + h;
  return t > 8 ? -1 : (DGRAD ? 8 - t : t);
}

// One k-step of a set: B fragments of the pixel at tile position px, every 16-block's accumulator.
template <int KW>
__device__ __forceinline__ void gc_step(floatx4 (&acc)[4], const bf16x8 (&wj)[4], const u32x4* tile, int px, int gq) {
  const int sw = px & 7;
  if constexpr (KW == 32) {
#pragma unroll
    for (int G = 0; G < 2; ++G) {
      const bf16x8 b = __builtin_bit_cast(bf16x8, tile[px * 8 + ((4 * G + gq) ^ sw)]);
      acc[2 * G] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wj[2 * G], b, acc[2 * G], 0, 0, 0);
      acc[2 * G + 1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wj[2 * G + 1], b, acc[2 * G + 1], 0, 0, 0);
    }
  } else {
#pragma unroll
    for (int kb = 0; kb < 4; ++kb) {
      const bf16x8 b = __builtin_bit_cast(bf16x8, tile[px * 8 + ((2 * kb + (gq & 1)) ^ sw)]);
      acc[kb] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wj[kb], b, acc[kb], 0, 0, 0);
    }
  }
}

// A set's epilogue, private to the wave: lane (g, l16) holds channels 16 kb + 4 g + v of pixel l16; through
// the wave's 2 KiB stage (16 pixels x 128 bytes, chunks swizzled by pixel) to 16-byte stores, 8 lanes per
// pixel.  pix(p, R, col): flattened output row and column of the set's pixel p; false: not an output.
template <class F>
__device__ __forceinline__ void gc_store(const floatx4 (&acc)[4], int relu, u32x4* ostw, bf16_t* __restrict__ out,
                                         const GcGeo& g, int cb, int lane, F&& pix) {
  const int gq = lane >> 4, l16 = lane & 15;
  uint2* o8 = reinterpret_cast<uint2*>(ostw);
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    floatx4 v = acc[kb];
    if (relu) v = floatx4{fmaxf(v[0], 0.f), fmaxf(v[1], 0.f), fmaxf(v[2], 0.f), fmaxf(v[3], 0.f)};
    uint2 pk;
    pk.x = (uint32_t)f2bf(v[0]) | ((uint32_t)f2bf(v[1]) << 16);
    pk.y = (uint32_t)f2bf(v[2]) | ((uint32_t)f2bf(v[3]) << 16);
    o8[l16 * 16 + (((2 * kb + (gq >> 1)) ^ (l16 & 7)) << 1) + (gq & 1)] = pk;
  }
  // the wave's own LDS accesses execute in order; the fences keep the compiler from reordering them
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int idx = h * 64 + lane, p = idx >> 3, ch = idx & 7;
    const u32x4 val = ostw[p * 8 + (ch ^ (p & 7))];
    int R, col;
    if (pix(p, R, col) && cb * kGcCB + ch * 8 < g.C)
      *reinterpret_cast<u32x4*>(out + ((int64_t)R * g.OW + col) * g.C + cb * kGcCB + ch * 8) = val;
  }
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// Stride-2 dgrad, one set of row parity A and column parity B: the tile positions (dr, dc) it gathers and
// their weight taps.  dx row h takes dy row h >> 1 with tap row 1 (h even) or 2 (h odd), and for odd h the
// next dy row with tap row 0; columns alike.
template <int KW, int A, int B>
__device__ __forceinline__ void gc_dg2_class(floatx4 (&acc)[4], const bf16x8 (&wf)[KW == 32 ? 9 : 5][4],
                                             const u32x4* tile, int base, int LC, int gq) {
  if constexpr (KW == 32) {
#pragma unroll
    for (int ir = 0; ir <= A; ++ir)
#pragma unroll
      for (int ic = 0; ic <= B; ++ic) {
        const int r = A ? (ir ? 0 : 2) : 1, s = B ? (ic ? 0 : 2) : 1;
        gc_step<32>(acc, wf[r * 3 + s], tile, base + ir * LC + ic, gq);
      }
  } else {
    const int h = gq >> 1;   // which tap of the fragment's pair this lane's k-block belongs to
    if constexpr (A == 0 && B == 0) gc_step<16>(acc, wf[0], tile, base, gq);
    else if constexpr (A == 0) gc_step<16>(acc, wf[1], tile, base + h, gq);
    else if constexpr (B == 0) gc_step<16>(acc, wf[2], tile, base + h * LC, gq);
    else {
      gc_step<16>(acc, wf[3], tile, base + h, gq);
      gc_step<16>(acc, wf[4], tile, base + LC + h, gq);
    }
  }
}

// Forward (DGRAD = false: in = x, out = y) and input gradient (DGRAD = true: in = dy, out = dx).
// grid (row tiles * column tiles, channel slabs).  glog = log2(gw).
template <int STRIDE, bool DGRAD, int KW>
__global__ __launch_bounds__(kGcBlock, 2) void gconv3x3_kernel(const bf16_t* __restrict__ in,
                                                               const bf16_t* __restrict__ w,
                                                               const float* __restrict__ bias, int relu,
                                                               bf16_t* __restrict__ out, GcGeo g, int glog) {
  using K = GcCfg<STRIDE, DGRAD>;
  constexpr int NF = KW == 32 ? 9 : 5, ST = K::kSt;
  __shared__ u32x4 tile[kGcMaxPx * 8];
  __shared__ u32x4 ost[4 * 128];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, gq = lane >> 4, l16 = lane & 15;
  const int rt = fdiv((int)blockIdx.x, g.d_ntc), ct = (int)blockIdx.x - rt * g.ntc;
  const int cb = blockIdx.y;
  const int R0 = rt * g.TR, c0 = ct * g.TC;
  const int Rl = (R0 + g.TR < g.NR ? R0 + g.TR : g.NR) - 1;
  const int G0 = gc_in_row<STRIDE, DGRAD>(R0, g);
  const int span = gc_in_row<STRIDE, DGRAD>(Rl, g) + K::kTapRows - G0;
  const int gw = 1 << glog;

  // the slab's weights [64][9][gw] through the tile's LDS into A fragments.  The input gradient stages each
  // group's gw x gw block transposed ([c][tap][k] from [k][tap][c]), so both passes read vectors below
  {
    const int per = 9 * gw / 8, nv = kGcCB * per;   // 16-byte vectors per channel, per slab
    for (int i = tid; i < nv; i += kGcBlock) {
      const int kl = i / per, rem = i - kl * per;
      u32x4 val = {0u, 0u, 0u, 0u};
      if (cb * kGcCB + kl < g.C) val = reinterpret_cast<const u32x4*>(w)[(int64_t)cb * nv + i];
      if constexpr (!DGRAD) {
        tile[i] = val;
      } else {
        const int tap = rem >> (glog - 3), c0g = (kl & ~(gw - 1)) + ((rem & ((gw >> 3) - 1)) << 3);
        const u16x8 v = __builtin_bit_cast(u16x8, val);
        uint16_t* wt = reinterpret_cast<uint16_t*>(tile);
#pragma unroll
        for (int e = 0; e < 8; ++e) wt[(((c0g + e) * 9 + tap) << glog) + (kl & (gw - 1))] = v[e];
      }
    }
  }
  __syncthreads();
  bf16x8 wf[NF][4];
  {
    const uint16_t* wl = reinterpret_cast<const uint16_t*>(tile);
#pragma unroll
    for (int f = 0; f < NF; ++f)
#pragma unroll
      for (int kb = 0; kb < 4; ++kb) {
        const int tap = (gq >> 1) ? gc_frag_tap<STRIDE, DGRAD, KW>(f, 1) : gc_frag_tap<STRIDE, DGRAD, KW>(f, 0);
        const int tp = tap < 0 ? 0 : tap;
        const int p = 16 * kb + l16;                                            // this row's channel
        const int q0 = KW == 32 ? 32 * (kb >> 1) + 8 * gq : 16 * kb + 8 * (gq & 1);   // the k-block's first channel
        u16x8 v = *reinterpret_cast<const u16x8*>(wl + ((p * 9 + tp) << glog) + (q0 & (gw - 1)));
        if (tap < 0 || (p >> glog) != (q0 >> glog)) v = u16x8{0, 0, 0, 0, 0, 0, 0, 0};   // (gw 8: off the diagonal)
        wf[f][kb] = __builtin_bit_cast(bf16x8, v);
      }
  }
  __syncthreads();
  gc_stage(in, tile, g, G0, span, K::kDg2 ? c0 >> 1 : c0 * ST - 1, cb, tid);
  __syncthreads();

  floatx4 bv[4];
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    const int c = cb * kGcCB + 16 * kb + 4 * gq;
    const bool ok = !DGRAD && bias != nullptr && c < g.C;
#pragma unroll
    for (int v = 0; v < 4; ++v) bv[kb][v] = ok ? bias[c + v] : 0.f;
  }
  u32x4* ostw = ost + wv * 128;
  const int nrows = Rl - R0 + 1;

  if constexpr (!K::kDg2) {
    const int swl = g.swl, swm = (1 << swl) - 1, rps = 16 >> swl;
    const int nsets = (nrows + rps - 1) >> (4 - swl);
    for (int s = wv; s < nsets; s += 4) {
      const int Rs = R0 + s * rps;
      const int R = Rs + (l16 >> swl);
      const int base = (gc_in_row<STRIDE, DGRAD>(R <= Rl ? R : Rl, g) - G0) * g.LC + (l16 & swm) * ST;
      floatx4 acc[4] = {bv[0], bv[1], bv[2], bv[3]};
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        int off;
        if constexpr (KW == 32) {
          off = (j / 3) * g.LC + j % 3;
        } else {
          // the zero half of the fifth fragment reads the ninth tap's pixel again (finite times zero)
          const int t0 = 2 * j, t1 = 2 * j + 1 > 8 ? 8 : 2 * j + 1;
          off = (gq >> 1) ? (t1 / 3) * g.LC + t1 % 3 : (t0 / 3) * g.LC + t0 % 3;
        }
        gc_step<KW>(acc, wf[j], tile, base + off, gq);
      }
      gc_store(acc, !DGRAD && relu, ostw, out, g, cb, lane, [&](int p, int& Ro, int& co) {
        Ro = Rs + (p >> swl);
        co = c0 + (p & swm);
        return Ro <= Rl && co < g.OW;
      });
    }
  } else {
    for (int s = wv; s < nrows; s += 4) {
      const int R = R0 + s;
      const int hodd = (R - fdiv(R, g.d_oh) * g.OH) & 1;
      const int base = (gc_in_row<STRIDE, DGRAD>(R, g) - G0) * g.LC + l16;
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        floatx4 acc[4] = {bv[0], bv[1], bv[2], bv[3]};
        if (hodd) {
          if (b) gc_dg2_class<KW, 1, 1>(acc, wf, tile, base, g.LC, gq);
          else gc_dg2_class<KW, 1, 0>(acc, wf, tile, base, g.LC, gq);
        } else {
          if (b) gc_dg2_class<KW, 0, 1>(acc, wf, tile, base, g.LC, gq);
          else gc_dg2_class<KW, 0, 0>(acc, wf, tile, base, g.LC, gq);
        }
        gc_store(acc, 0, ostw, out, g, cb, lane, [&](int p, int& Ro, int& co) {
          Ro = R;
          co = c0 + 2 * p + b;
          return co < g.OW;
        });
      }
    }
  }
}

// Weight gradient partials: part[slice][slab * 64 + k][9][gw].  grid (slices, channel slabs); a slice takes
// `tps` row tiles (forward geometry: out = dy, in = x) and every column tile.
template <int STRIDE, int KW>
__global__ __launch_bounds__(kGcBlock, 2) void gconv3x3_wgrad_kernel(const bf16_t* __restrict__ x,
                                                                     const bf16_t* __restrict__ dy,
                                                                     float* __restrict__ part, GcGeo g, int glog,
                                                                     int tps) {
  constexpr int NB = KW == 32 ? 2 : 1;
  __shared__ u32x4 xt[kGcMaxPx * 8];
  __shared__ u32x4 dyt[kGcMaxSlots * 8];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, gq = lane >> 4, l16 = lane & 15;
  const int qq = l16 >> 2, pp = l16 & 3;
  const int cb = blockIdx.y;
  const int swl = g.swl, swm = (1 << swl) - 1;
  const char* const xb = reinterpret_cast<const char*>(xt);
  const char* const db = reinterpret_cast<const char*>(dyt);
  floatx4 acc[9][NB];
#pragma unroll
  for (int t = 0; t < 9; ++t)
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[t][b] = floatx4{0.f, 0.f, 0.f, 0.f};

  // a transposing read: lane (g, l16) gets channel 16 * (chunk / 2) + l16 of 4 consecutive pixel rows
  auto frag = [&](const char* buf, int r0, int r1, int chunk) {
    const bf16x4 lo =
        __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b4*)(buf + r0 * 128 + ((chunk ^ (r0 & 7)) << 4) + 8 * (pp & 1)));
    const bf16x4 hi =
        __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_b4*)(buf + r1 * 128 + ((chunk ^ (r1 & 7)) << 4) + 8 * (pp & 1)));
    return bf16x8{lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  };

  const int rt_end = ((int)blockIdx.x + 1) * tps < g.ntr ? ((int)blockIdx.x + 1) * tps : g.ntr;
  for (int rt = (int)blockIdx.x * tps; rt < rt_end; ++rt) {
    const int R0 = rt * g.TR;
    const int Rl = (R0 + g.TR < g.NR ? R0 + g.TR : g.NR) - 1;
    const int G0 = gc_in_row<STRIDE, false>(R0, g);
    const int span = gc_in_row<STRIDE, false>(Rl, g) + 3 - G0;
    const int nrows = Rl - R0 + 1;
    const int nk = ((nrows << swl) + 31) >> 5;   // k-steps of 32 pixel slots (<= kGcMaxSlots / 32)
    for (int ct = 0; ct < g.ntc; ++ct) {
      const int c0 = ct * g.TC;
      __syncthreads();   // (the previous tile's readers are done)
      gc_stage(x, xt, g, G0, span, c0 * STRIDE - 1, cb, tid);
      {
        // dy slot i = the tile's pixel (row i >> swl, column i & swm); zeros past the tile, the image or C
        const int v = tid & 7, ch = cb * kGcCB + v * 8;
        for (int i = tid >> 3; i < nk * 32; i += kGcBlock / 8) {
          const int R = R0 + (i >> swl), col = c0 + (i & swm);
          u32x4 val = {0u, 0u, 0u, 0u};
          if (R <= Rl && col < g.OW && ch < g.C)
            val = *reinterpret_cast<const u32x4*>(dy + ((int64_t)R * g.OW + col) * g.C + ch);
          dyt[i * 8 + (v ^ (i & 7))] = val;
        }
      }
      __syncthreads();
      for (int kk = 0; kk < nk; ++kk) {
        const int i0 = 32 * kk + 8 * gq + qq, i1 = i0 + 4;
        const bf16x8 fdy = frag(db, i0, i1, 2 * wv + (pp >> 1));
        // x positions of the two slots at tap (0, 0); a slot past the tile's rows has dy = 0 and reads
        // the last row's (staged, finite) pixels
        int pb[2];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
          const int i = u ? i1 : i0;
          const int row = (i >> swl) < nrows ? (i >> swl) : nrows - 1;
          pb[u] = (gc_in_row<STRIDE, false>(R0 + row, g) - G0) * g.LC + (i & swm) * STRIDE;
        }
#pragma unroll
        for (int t = 0; t < 9; ++t) {
          const int off = (t / 3) * g.LC + t % 3;
#pragma unroll
          for (int b = 0; b < NB; ++b) {
            const int chunk = (KW == 32 ? 4 * (wv >> 1) + 2 * b : 2 * wv) + (pp >> 1);
            const bf16x8 fx = frag(xb, pb[0] + off, pb[1] + off, chunk);
            acc[t][b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fx, fdy, acc[t][b], 0, 0, 0);
          }
        }
      }
    }
  }

  // lane holds dw[k = 16 wv + l16][tap][in-channels 4 gq + 0..3 of the wave's 16-block b]
  const int gw = 1 << glog;
  const bool own = glog > 3 || (gq >> 1) == (l16 >> 3);   // gw 8: only the diagonal 8 x 8 blocks exist
  const int ci0 = (4 * gq) & (gw - 1);
  float* dst = part + (((int64_t)blockIdx.x * g.ncb + cb) * kGcCB + 16 * wv + l16) * 9 * gw;
  if (own) {
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
      for (int b = 0; b < NB; ++b) *reinterpret_cast<floatx4*>(dst + t * gw + 16 * b + ci0) = acc[t][b];
  }
}

// dw storage [C][9][gw] = or += the slices' sum in a fixed order: four wave-sized groups take every fourth
// slice each (independent loads in flight), then their sums are added in group order.  n4 = C * 9 * gw / 4.
__global__ __launch_bounds__(kGcBlock) void gconv_wgrad_finalize_kernel(const float* __restrict__ part,
                                                                       float* __restrict__ dw, int slices,
                                                                       int64_t stride4, int n4, int accumulate) {
  __shared__ floatx4 red[4][64];
  const int e = threadIdx.x & 63, sg = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + e;
  const bool ok = i < n4;
  floatx4 sum = {0.f, 0.f, 0.f, 0.f};
  if (ok) {
#pragma unroll 4
    for (int s = sg; s < slices; s += 4) sum += reinterpret_cast<const floatx4*>(part)[(int64_t)s * stride4 + i];
  }
  red[sg][e] = sum;
  __syncthreads();
  if (sg != 0 || !ok) return;
  sum = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
  floatx4* dst = reinterpret_cast<floatx4*>(dw) + i;
  *dst = accumulate ? *dst + sum : sum;
}

int gc_glog(int gw) { return gw == 8 ? 3 : gw == 16 ? 4 : gw == 32 ? 5 : -1; }

bool gc_shape_ok(int64_t N, int64_t H, int64_t W, int64_t C, int gw, int stride) {
  if (N < 1 || H < 1 || W < 1 || gc_glog(gw) < 0 || C < gw || C % gw != 0 || (stride != 1 && stride != 2)) return false;
  // flattened (padded) rows, tile counts and the weight index stay in int32; channel slabs in grid.y
  return N * (H + 2) < INT32_MAX && N * (H + 2) * ((W + 1) / 2) < INT32_MAX && C <= 65535 * kGcCB;
}

bool gc_aligned(const void* a, const void* b, const void* c, const void* d = nullptr) {
  return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
           reinterpret_cast<uintptr_t>(d)) & 15) == 0;
}

int gc_slices(const GcGeo& g, int* tps) {
  const int want = kGcSliceTarget / g.ncb > 0 ? kGcSliceTarget / g.ncb : 1;
  *tps = (g.ntr + want - 1) / want;
  return (g.ntr + *tps - 1) / *tps;
}

GcGeo gc_fwd_geometry(int N, int H, int W, int C, int stride) {
  const int P = (H - 1) / stride + 1, Q = (W - 1) / stride + 1;
  return stride == 1 ? gc_geometry<1, false>(N, P, Q, H, W, C) : gc_geometry<2, false>(N, P, Q, H, W, C);
}

template <bool DGRAD>
void gc_launch(const bf16_t* in, const bf16_t* w, const float* bias, int relu, bf16_t* out, const GcGeo& g, int gw,
               int stride, hipStream_t s) {
  const dim3 grid((unsigned)(g.ntr * g.ntc), (unsigned)g.ncb);
  const int glog = gc_glog(gw);
  if (stride == 1) {
    if (gw == 32) gconv3x3_kernel<1, DGRAD, 32><<<grid, kGcBlock, 0, s>>>(in, w, bias, relu, out, g, glog);
    else gconv3x3_kernel<1, DGRAD, 16><<<grid, kGcBlock, 0, s>>>(in, w, bias, relu, out, g, glog);
  } else {
    if (gw == 32) gconv3x3_kernel<2, DGRAD, 32><<<grid, kGcBlock, 0, s>>>(in, w, bias, relu, out, g, glog);
    else gconv3x3_kernel<2, DGRAD, 16><<<grid, kGcBlock, 0, s>>>(in, w, bias, relu, out, g, glog);
  }
}

}  // namespace

int64_t gconv_workspace_floats(int64_t N, int64_t H, int64_t W, int64_t C, int gw, int stride) {
  if (!gc_shape_ok(N, H, W, C, gw, stride)) return -1;
  int tps;
  const GcGeo g = gc_fwd_geometry((int)N, (int)H, (int)W, (int)C, stride);
  return (int64_t)gc_slices(g, &tps) * g.ncb * kGcCB * 9 * gw;
}

hipError_t gconv_forward(const uint16_t* x, const uint16_t* w, const float* bias, bool relu, uint16_t* y, int64_t N,
                         int64_t H, int64_t W, int64_t C, int gw, int stride, hipStream_t s) {
  if (!gc_shape_ok(N, H, W, C, gw, stride) || !x || !w || !y || !gc_aligned(x, y, w)) return hipErrorInvalidValue;
  const GcGeo g = gc_fwd_geometry((int)N, (int)H, (int)W, (int)C, stride);
  gc_launch<false>(x, w, bias, relu ? 1 : 0, y, g, gw, stride, s);
  return hipGetLastError();
}

hipError_t gconv_dgrad(const uint16_t* dy, const uint16_t* w, uint16_t* dx, int64_t N, int64_t H, int64_t W, int64_t C,
                       int gw, int stride, hipStream_t s) {
  if (!gc_shape_ok(N, H, W, C, gw, stride) || !dy || !w || !dx || !gc_aligned(dy, dx, w)) return hipErrorInvalidValue;
  const int P = (int)((H - 1) / stride + 1), Q = (int)((W - 1) / stride + 1);
  const GcGeo g = stride == 1 ? gc_geometry<1, true>((int)N, (int)H, (int)W, P, Q, (int)C)
                              : gc_geometry<2, true>((int)N, (int)H, (int)W, P, Q, (int)C);
  gc_launch<true>(dy, w, nullptr, 0, dx, g, gw, stride, s);
  return hipGetLastError();
}

hipError_t gconv_wgrad(const uint16_t* x, const uint16_t* dy, float* ws, float* dw, bool accumulate, int64_t N,
                       int64_t H, int64_t W, int64_t C, int gw, int stride, hipStream_t s) {
  if (!gc_shape_ok(N, H, W, C, gw, stride) || !x || !dy || !ws || !dw || !gc_aligned(x, dy, dw, ws))
    return hipErrorInvalidValue;
  const GcGeo g = gc_fwd_geometry((int)N, (int)H, (int)W, (int)C, stride);
  int tps;
  const int slices = gc_slices(g, &tps);
  const int glog = gc_glog(gw);
  const dim3 grid((unsigned)slices, (unsigned)g.ncb);
  if (stride == 1) {
    if (gw == 32) gconv3x3_wgrad_kernel<1, 32><<<grid, kGcBlock, 0, s>>>(x, dy, ws, g, glog, tps);
    else gconv3x3_wgrad_kernel<1, 16><<<grid, kGcBlock, 0, s>>>(x, dy, ws, g, glog, tps);
  } else {
    if (gw == 32) gconv3x3_wgrad_kernel<2, 32><<<grid, kGcBlock, 0, s>>>(x, dy, ws, g, glog, tps);
    else gconv3x3_wgrad_kernel<2, 16><<<grid, kGcBlock, 0, s>>>(x, dy, ws, g, glog, tps);
  }
  const int64_t n4 = C * 9 * gw / 4;
  gconv_wgrad_finalize_kernel<<<(unsigned)((n4 + 63) / 64), kGcBlock, 0, s>>>(
      ws, dw, slices, (int64_t)g.ncb * kGcCB * 9 * gw / 4, (int)n4, accumulate ? 1 : 0);
  return hipGetLastError();
}

}  // namespace ldnn
