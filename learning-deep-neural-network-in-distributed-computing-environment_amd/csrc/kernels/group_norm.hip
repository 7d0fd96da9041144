// GroupNorm over dense NHWC bf16 activations [N][P][C] (P = H * W pixels, C % 8 == 0), with the
// residual add and the ReLU fused into the apply pass, forward and backward.
//
//   G groups of cg = C / G neighbouring channels; statistics per (sample, group) over m = P * cg
//   elements, biased variance:
//     y  = relu?( (x - mean) * rstd * gamma[c] + beta[c] (+ residual) ),  rstd = rsqrt(var + eps)
//     dx = rstd * (gamma * g - (s1 + xhat * s2) / m),  g = dy * relu'(y),  xhat = (x - mean) * rstd,
//          s1 = sum_group gamma * g,  s2 = sum_group gamma * g * xhat
//     dgamma[c] = sum_{n,p} g * xhat,  dbeta[c] = sum_{n,p} g,  dres = g
//
// Three launches each way, no atomics and no inter-workgroup hand-off, so every output and both
// parameter gradients are the same bits on every run:
//   gn_stats / gn_bwd_stats   a thread owns one 8-channel vector column (16-B loads) and strides
//                             over the pixels of one (sample, pixel slab); per-channel sums stay in
//                             registers, the threads of a column are summed through LDS in a fixed
//                             order, and per-(sample, slab, channel) partials leave by plain stores.
//                             Working per channel makes every cg one code path: a group is a channel
//                             range, narrower or wider than a vector.
//   gn_finalize / gn_bwd_finalize   one small workgroup per (sample, group) sums slabs and the
//                             group's channels in double in a fixed order and writes per-(sample,
//                             channel) coefficients; the backward's further workgroups (one per 16
//                             channels) sum dgamma / dbeta over the samples in a fixed order.
//   gn_apply / gn_bwd_apply   streaming pass, 16-B loads and stores:  y = a*x + b (+ r),
//                             dx = c1*g + c2*x + c3.
// The slab split (gn_geometry) is a function of the shape alone, never of the device or a knob:
// a shape has one summation order.  Element offsets are 64-bit (N * P * C may pass 2^31).
//
// Workspace of one module, fp32, nothing in it has to survive a call or be zeroed:
//   part [N][S][2][C]   slab partials (fwd: sum x, sum x^2;  bwd: sum g, sum g * x)
//   coef [3][N][C]      fwd: a | b | -        bwd: c1 | c2 | c3
// The ReLU bit mask has bn_fwd's layout: byte (element offset / 8), bit j = channel c0 + j is > 0.
#include "ldnn_common.h"
#include "ldnn_kernels.h"

namespace ldnn {
namespace {

constexpr int kBlock = 256;
constexpr int kMaxSlabs = 64;
constexpr int kGradCh = 16, kGradLanes = kBlock / kGradCh;   // gn_bwd_finalize's dgamma / dbeta workgroups

struct GnGeo {
  int64_t N, P;   // samples, pixels per sample
  int C, G, cg;
  int V;          // vector columns, C / 8
  int lanes;      // vector columns per workgroup, min(V, 256)
  int rl;         // pixel lanes per workgroup, 256 / lanes (>= 1)
  int CB;         // column blocks, ceil(V / 256)
  int S;          // pixel slabs per sample (1 <= S <= min(P, kMaxSlabs))
  int64_t pps;    // pixels per slab, ceil(P / S); no slab is empty
};

// About four workgroups per CU of a 256-CU device for the large early layers; never more slabs
// than pixels (or than whole rounds of the workgroup's pixel lanes) for the 2x2 and 1x1 tails.
GnGeo gn_geometry(int64_t N, int64_t P, int C, int G) {
  GnGeo g;
  g.N = N, g.P = P, g.C = C, g.G = G, g.cg = C / G;
  g.V = C / 8;
  g.lanes = g.V < kBlock ? g.V : kBlock;
  g.rl = kBlock / g.lanes;
  g.CB = (g.V + kBlock - 1) / kBlock;
  const int64_t wgs = N * g.CB;
  int64_t want = (1024 + wgs - 1) / wgs;
  int64_t cap = P / g.rl;
  if (cap < 1) cap = 1;
  if (want > cap) want = cap;
  if (want > kMaxSlabs) want = kMaxSlabs;
  g.pps = (P + want - 1) / want;
  g.S = (int)((P + g.pps - 1) / g.pps);
  return g;
}

__device__ __forceinline__ void ld8f(const float* __restrict__ p, float (&v)[8]) {
  const floatx4 a = *reinterpret_cast<const floatx4*>(p), b = *reinterpret_cast<const floatx4*>(p + 4);
  v[0] = a[0], v[1] = a[1], v[2] = a[2], v[3] = a[3];
  v[4] = b[0], v[5] = b[1], v[6] = b[2], v[7] = b[3];
}

// Slab partials.  FWD: s0 = sum x, s1 = sum x^2.  !FWD: s0 = sum g, s1 = sum g * x, g = dy masked
// by the forward's ReLU bits when MASK.  grid (CB, S, N).
template <bool FWD, bool MASK>
__global__ __launch_bounds__(kBlock) void gn_stats_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                          const uint8_t* __restrict__ mask,
                                                          float* __restrict__ part, GnGeo g) {
  __shared__ float sm[16 * kBlock];
  const int tid = threadIdx.x, lane = tid % g.lanes, rlane = tid / g.lanes;
  const int v = blockIdx.x * kBlock + lane;
  const int64_t n = blockIdx.z, s = blockIdx.y;
  const bool active = rlane < g.rl && v < g.V;
  float s0[8], s1[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s0[j] = 0.f, s1[j] = 0.f;
  if (active) {
    const int64_t p_end = (s + 1) * g.pps < g.P ? (s + 1) * g.pps : g.P;
    const int64_t base = n * g.P * g.C + (int64_t)v * 8;
#pragma unroll 4
    for (int64_t p = s * g.pps + rlane; p < p_end; p += g.rl) {
      const int64_t o = base + p * g.C;
      const u16x8 xv = *reinterpret_cast<const u16x8*>(x + o);
      if constexpr (FWD) {
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float f = bf2f(xv[j]);
          s0[j] += f;
          s1[j] += f * f;
        }
      } else {
        const u16x8 gv = *reinterpret_cast<const u16x8*>(dy + o);
        uint32_t mb = 0xffu;
        if constexpr (MASK) mb = mask[o >> 3];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float f = ((mb >> j) & 1u) ? bf2f(gv[j]) : 0.f;
          s0[j] += f;
          s1[j] += f * bf2f(xv[j]);
        }
      }
    }
  }
  // sm[k][rlane][lane]: the pixel lanes of a column are summed in the order of rlane
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    sm[j * kBlock + tid] = s0[j];
    sm[(8 + j) * kBlock + tid] = s1[j];
  }
  __syncthreads();
  const int cols = min(g.lanes, g.V - (int)blockIdx.x * kBlock);   // this block's vector columns
  for (int i = tid; i < 16 * cols; i += kBlock) {
    const int k = i / cols, l = i - k * cols;   // k = which * 8 + channel of the vector
    float acc = 0.f;
    for (int r = 0; r < g.rl; ++r) acc += sm[k * kBlock + r * g.lanes + l];
    const int c = (blockIdx.x * kBlock + l) * 8 + (k & 7);
    part[((n * g.S + s) * 2 + (k >> 3)) * g.C + c] = acc;
  }
}

// Sum of (a, b) over the workgroup in a fixed tree; every thread calls it, the result is thread 0's
// and is broadcast through sm (which must hold 2 * kBlock doubles).
__device__ __forceinline__ void block_sum2(double& a, double& b, double* sm) {
  const int tid = threadIdx.x;
  __syncthreads();
  sm[tid] = a;
  sm[kBlock + tid] = b;
  __syncthreads();
  for (int o = kBlock / 2; o > 0; o >>= 1) {
    if (tid < o) {
      sm[tid] += sm[tid + o];
      sm[kBlock + tid] += sm[kBlock + tid + o];
    }
    __syncthreads();
  }
  a = sm[0];
  b = sm[kBlock];
}

// One workgroup per (n, group): mean, rstd and the apply coefficients a = rstd * gamma,
// b = beta - mean * a of the group's channels.
__global__ __launch_bounds__(kBlock) void gn_finalize_kernel(const float* __restrict__ part,
                                                             const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, float* __restrict__ mean,
                                                             float* __restrict__ rstd, float* __restrict__ coef,
                                                             float eps, GnGeo g) {
  __shared__ double sm[2 * kBlock];
  const int64_t ng = blockIdx.x, n = ng / g.G;
  const int grp = (int)(ng - n * g.G), c_lo = grp * g.cg;
  double t0 = 0.0, t1 = 0.0;
  for (int c = c_lo + threadIdx.x; c < c_lo + g.cg; c += kBlock) {
    for (int s = 0; s < g.S; ++s) {
      const float* p = part + ((n * g.S + s) * 2) * g.C + c;
      t0 += (double)p[0];
      t1 += (double)p[g.C];
    }
  }
  block_sum2(t0, t1, sm);
  const double m = (double)g.P * (double)g.cg;
  const double mu = t0 / m;
  double var = t1 / m - mu * mu;
  if (var < 0.0) var = 0.0;
  const float fmu = (float)mu, frs = (float)(1.0 / sqrt(var + (double)eps));
  if (threadIdx.x == 0) {
    mean[ng] = fmu;
    rstd[ng] = frs;
  }
  float* ca = coef + n * g.C;
  float* cb = coef + (g.N + n) * g.C;
  for (int c = c_lo + threadIdx.x; c < c_lo + g.cg; c += kBlock) {
    const float a = frs * (gamma ? gamma[c] : 1.f);
    ca[c] = a;
    cb[c] = (beta ? beta[c] : 0.f) - fmu * a;
  }
}

// y = relu?( a[n][c] * x + b[n][c] (+ res) ), and the ReLU bits when MASK.  grid (CB, S, N).
template <bool RES, bool RELU, bool MASK>
__global__ __launch_bounds__(kBlock) void gn_apply_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ res,
                                                          const float* __restrict__ coef, bf16_t* __restrict__ y,
                                                          uint8_t* __restrict__ mask, GnGeo g) {
  const int tid = threadIdx.x, lane = tid % g.lanes, rlane = tid / g.lanes;
  const int v = blockIdx.x * kBlock + lane;
  if (rlane >= g.rl || v >= g.V) return;
  const int64_t n = blockIdx.z, s = blockIdx.y;
  float a[8], b[8];
  ld8f(coef + n * g.C + v * 8, a);
  ld8f(coef + (g.N + n) * g.C + v * 8, b);
  const int64_t p_end = (s + 1) * g.pps < g.P ? (s + 1) * g.pps : g.P;
  const int64_t base = n * g.P * g.C + (int64_t)v * 8;
#pragma unroll 4
  for (int64_t p = s * g.pps + rlane; p < p_end; p += g.rl) {
    const int64_t o = base + p * g.C;
    const u16x8 xv = *reinterpret_cast<const u16x8*>(x + o);
    u16x8 rv;
    if constexpr (RES) rv = *reinterpret_cast<const u16x8*>(res + o);
    u16x8 out;
    uint32_t mb = 0;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = bf2f(xv[j]) * a[j] + b[j];
      if constexpr (RES) f += bf2f(rv[j]);
      if constexpr (RELU) f = fmaxf(f, 0.f);
      out[j] = f2bf(f);
      if constexpr (MASK) mb |= (bf2f(out[j]) > 0.f ? 1u : 0u) << j;
    }
    *reinterpret_cast<u16x8*>(y + o) = out;
    if constexpr (MASK) mask[o >> 3] = (uint8_t)mb;
  }
}

// Workgroups [0, N*G): one per (n, group) -- s1, s2 and the dx coefficients of its channels:
//   c1 = rstd * gamma,  c2 = -rstd^2 * s2 / m,  c3 = (rstd^2 * s2 * mean - rstd * s1) / m.
// Workgroups [N*G, N*G + ceil(C/16)) (only with dgamma / dbeta): 16 channels x 16 sample lanes;
// lane q sums samples q, q+16, ... in order, the sixteen are added in order, the total is stored
// (assign) or added to the flat gradient.
__global__ __launch_bounds__(kBlock) void gn_bwd_finalize_kernel(const float* __restrict__ part,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ mean,
                                                                 const float* __restrict__ rstd,
                                                                 float* __restrict__ coef, float* __restrict__ dgamma,
                                                                 float* __restrict__ dbeta, int assign, GnGeo g) {
  __shared__ double sm[2 * kBlock];
  const int64_t groups = g.N * g.G;
  if ((int64_t)blockIdx.x < groups) {
    const int64_t ng = blockIdx.x, n = ng / g.G;
    const int grp = (int)(ng - n * g.G), c_lo = grp * g.cg;
    const double mu = (double)mean[ng], rs = (double)rstd[ng];
    double s1 = 0.0, s2 = 0.0;
    for (int c = c_lo + threadIdx.x; c < c_lo + g.cg; c += kBlock) {
      double A = 0.0, B = 0.0;
      for (int s = 0; s < g.S; ++s) {
        const float* p = part + ((n * g.S + s) * 2) * g.C + c;
        A += (double)p[0];
        B += (double)p[g.C];
      }
      const double gm = gamma ? (double)gamma[c] : 1.0;
      s1 += gm * A;
      s2 += gm * rs * (B - mu * A);
    }
    block_sum2(s1, s2, sm);
    const double m = (double)g.P * (double)g.cg;
    const float c2 = (float)(-rs * rs * s2 / m), c3 = (float)((rs * rs * s2 * mu - rs * s1) / m);
    float* k1 = coef + n * g.C;
    float* k2 = coef + (g.N + n) * g.C;
    float* k3 = coef + (2 * g.N + n) * g.C;
    for (int c = c_lo + threadIdx.x; c < c_lo + g.cg; c += kBlock) {
      k1[c] = (float)rs * (gamma ? gamma[c] : 1.f);
      k2[c] = c2;
      k3[c] = c3;
    }
    return;
  }
  const int cl = threadIdx.x & (kGradCh - 1), q = threadIdx.x / kGradCh;
  const int c = (int)((int64_t)blockIdx.x - groups) * kGradCh + cl;
  double dg = 0.0, db = 0.0;
  if (c < g.C) {
    const int grp = c / g.cg;
    for (int64_t n = q; n < g.N; n += kGradLanes) {
      double A = 0.0, B = 0.0;
      for (int s = 0; s < g.S; ++s) {
        const float* p = part + ((n * g.S + s) * 2) * g.C + c;
        A += (double)p[0];
        B += (double)p[g.C];
      }
      const double mu = (double)mean[n * g.G + grp], rs = (double)rstd[n * g.G + grp];
      dg += rs * (B - mu * A);
      db += A;
    }
  }
  sm[threadIdx.x] = dg;
  sm[kBlock + threadIdx.x] = db;
  __syncthreads();
  if (q == 0 && c < g.C) {
    double tg = 0.0, tb = 0.0;
    for (int l = 0; l < kGradLanes; ++l) {   // the sample lanes in order
      tg += sm[l * kGradCh + cl];
      tb += sm[kBlock + l * kGradCh + cl];
    }
    if (dgamma) dgamma[c] = assign ? (float)tg : dgamma[c] + (float)tg;
    if (dbeta) dbeta[c] = assign ? (float)tb : dbeta[c] + (float)tb;
  }
}

// dx = c1 * g + c2 * x + c3, dres = g (g = dy masked by the ReLU bits when MASK).  grid (CB, S, N).
template <bool MASK>
__global__ __launch_bounds__(kBlock) void gn_bwd_apply_kernel(const bf16_t* __restrict__ x,
                                                              const bf16_t* __restrict__ dy,
                                                              const uint8_t* __restrict__ mask,
                                                              const float* __restrict__ coef, bf16_t* __restrict__ dx,
                                                              bf16_t* __restrict__ dres, GnGeo g) {
  const int tid = threadIdx.x, lane = tid % g.lanes, rlane = tid / g.lanes;
  const int v = blockIdx.x * kBlock + lane;
  if (rlane >= g.rl || v >= g.V) return;
  const int64_t n = blockIdx.z, s = blockIdx.y;
  float c1[8], c2[8], c3[8];
  ld8f(coef + n * g.C + v * 8, c1);
  ld8f(coef + (g.N + n) * g.C + v * 8, c2);
  ld8f(coef + (2 * g.N + n) * g.C + v * 8, c3);
  const int64_t p_end = (s + 1) * g.pps < g.P ? (s + 1) * g.pps : g.P;
  const int64_t base = n * g.P * g.C + (int64_t)v * 8;
#pragma unroll 4
  for (int64_t p = s * g.pps + rlane; p < p_end; p += g.rl) {
    const int64_t o = base + p * g.C;
    const u16x8 xv = *reinterpret_cast<const u16x8*>(x + o);
    const u16x8 gv = *reinterpret_cast<const u16x8*>(dy + o);
    uint32_t mb = 0xffu;
    if constexpr (MASK) mb = mask[o >> 3];
    u16x8 out, og;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float f = ((mb >> j) & 1u) ? bf2f(gv[j]) : 0.f;
      out[j] = f2bf(c1[j] * f + c2[j] * bf2f(xv[j]) + c3[j]);
      og[j] = f2bf(f);
    }
    *reinterpret_cast<u16x8*>(dx + o) = out;
    if (dres) *reinterpret_cast<u16x8*>(dres + o) = og;
  }
}

bool gn_args_ok(const GnArgs& a) {
  if (a.x == nullptr || a.mean == nullptr || a.rstd == nullptr || a.ws == nullptr) return false;
  if (a.N < 1 || a.N > 65535 || a.P < 1 || a.C < 8 || a.C % 8 != 0 || a.G < 1 || a.C % a.G != 0) return false;
  if (a.P > INT64_MAX / a.C / a.N / 4) return false;   // (element and byte offsets stay in int64)
  if (a.N * a.G + a.C / kGradCh + 1 > INT32_MAX) return false;   // (the finalize grids)
  return ((reinterpret_cast<uintptr_t>(a.x) | reinterpret_cast<uintptr_t>(a.y) |
           reinterpret_cast<uintptr_t>(a.residual) | reinterpret_cast<uintptr_t>(a.ws)) & 15) == 0;
}

}  // namespace

int64_t gn_workspace_floats(int64_t N, int64_t P, int C, int G) {
  const GnGeo g = gn_geometry(N, P, C, G);
  return N * g.S * 2 * C + 3 * N * C;
}

int gn_slabs(int64_t N, int64_t P, int C, int G) { return gn_geometry(N, P, C, G).S; }

hipError_t gn_forward(const GnArgs& a, hipStream_t s) {
  if (!gn_args_ok(a) || a.y == nullptr || (a.mask && !a.relu)) return hipErrorInvalidValue;
  const GnGeo g = gn_geometry(a.N, a.P, a.C, a.G);
  float* part = a.ws;
  float* coef = a.ws + a.N * g.S * 2 * a.C;
  const dim3 grid(g.CB, g.S, (unsigned)a.N);
  if (!a.apply_only) {
    gn_stats_kernel<true, false><<<grid, kBlock, 0, s>>>(a.x, nullptr, nullptr, part, g);
    gn_finalize_kernel<<<(unsigned)(a.N * a.G), kBlock, 0, s>>>(part, a.gamma, a.beta, a.mean, a.rstd, coef, a.eps, g);
  }
  if (a.residual) {
    if (a.mask) gn_apply_kernel<true, true, true><<<grid, kBlock, 0, s>>>(a.x, a.residual, coef, a.y, a.mask, g);
    else if (a.relu) gn_apply_kernel<true, true, false><<<grid, kBlock, 0, s>>>(a.x, a.residual, coef, a.y, nullptr, g);
    else gn_apply_kernel<true, false, false><<<grid, kBlock, 0, s>>>(a.x, a.residual, coef, a.y, nullptr, g);
  } else {
    if (a.mask) gn_apply_kernel<false, true, true><<<grid, kBlock, 0, s>>>(a.x, nullptr, coef, a.y, a.mask, g);
    else if (a.relu) gn_apply_kernel<false, true, false><<<grid, kBlock, 0, s>>>(a.x, nullptr, coef, a.y, nullptr, g);
    else gn_apply_kernel<false, false, false><<<grid, kBlock, 0, s>>>(a.x, nullptr, coef, a.y, nullptr, g);
  }
  return hipGetLastError();
}

hipError_t gn_backward(const GnArgs& a, const uint16_t* dy, uint16_t* dx, uint16_t* dres, float* dgamma, float* dbeta,
                       bool grad_assign, hipStream_t s) {
  if (!gn_args_ok(a) || dy == nullptr || dx == nullptr || (a.relu != 0) != (a.mask != nullptr))
    return hipErrorInvalidValue;
  if ((reinterpret_cast<uintptr_t>(dy) | reinterpret_cast<uintptr_t>(dx) | reinterpret_cast<uintptr_t>(dres)) & 15)
    return hipErrorInvalidValue;
  const GnGeo g = gn_geometry(a.N, a.P, a.C, a.G);
  float* part = a.ws;
  float* coef = a.ws + a.N * g.S * 2 * a.C;
  const dim3 grid(g.CB, g.S, (unsigned)a.N);
  if (!a.apply_only) {
    if (a.mask) gn_stats_kernel<false, true><<<grid, kBlock, 0, s>>>(a.x, dy, a.mask, part, g);
    else gn_stats_kernel<false, false><<<grid, kBlock, 0, s>>>(a.x, dy, nullptr, part, g);
    const int64_t fin = a.N * a.G + ((dgamma || dbeta) ? (a.C + kGradCh - 1) / kGradCh : 0);
    gn_bwd_finalize_kernel<<<(unsigned)fin, kBlock, 0, s>>>(part, a.gamma, a.mean, a.rstd, coef, dgamma, dbeta,
                                                          grad_assign ? 1 : 0, g);
  }
  if (a.mask) gn_bwd_apply_kernel<true><<<grid, kBlock, 0, s>>>(a.x, dy, a.mask, coef, dx, dres, g);
  else gn_bwd_apply_kernel<false><<<grid, kBlock, 0, s>>>(a.x, dy, nullptr, coef, dx, dres, g);
  return hipGetLastError();
}

}  // namespace ldnn
