// LayerNorm over the last dimension of a logical [B][N] bf16 matrix, with the layer's activation
// fused, forward and backward.
//
//   y  = act(z),  z = gamma * xhat + beta,  xhat = (x - mean) * rstd,  rstd = rsqrt(var + eps),
//        mean and biased variance per row;  act in none | relu | sigmoid
//   dx = rstd * (a - s1 / N - xhat * s2 / N),  a = dz * gamma,  dz = dy * act'(z),
//        s1 = sum_row a,  s2 = sum_row a * xhat
//   dgamma[j] = sum_rows dz * xhat,  dbeta[j] = sum_rows dz
//
// Operands: row stride ld >= N in elements, ld % 8 == 0, 16-byte aligned bases, 64-bit row offsets.
// N need not be a multiple of 8: the last 16-byte vector of a row lies inside the row's stride and
// is loaded whole; its lanes beyond N are removed by select (never by a product with 0: padding may
// hold NaN) and count neither in the sums nor in N.  The outputs' pad columns N <= c < ld are written
// as zeros under every activation, so a padded consumer skips its re-zeroing.
//
// One wave owns a row at a time; a lane holds the row's vectors lane, lane + 64, ... as packed bf16
// in registers (VPL vectors per lane, instances 1, 2, 4, 8, 16: rows up to 8192 wide), so a row is
// read once.  The mean is a wave reduction, the variance the sum of (x - mean)^2 over the registers
// (two passes at no memory cost, clamped at 0).  Only mean[B] and rstd[B] are saved (fp32).
// gamma / beta are streamed from the cache one vector ahead of their use (ln_coef and the compiler
// barrier behind it): loading a whole row's worth up front costs 16 registers per vector.
//
// The backward recomputes z with the forward's expression (ln_z), so the ReLU decision is the
// forward's bit for bit and no mask is stored.  Up to 4096 columns (PSUM instances) a lane
// accumulates the dgamma / dbeta partials of its columns in registers across its rows; after the
// last row the workgroup's four waves are added through LDS in the order of the wave index and the
// workgroup's partial row leaves by plain stores: x and dy are read once, 6 B per element.  The
// 16-vector instance has no registers for 256 partials beside two packed rows, so its parameter
// sums are a kernel of their own (ln_param_partials: a lane owns a vector column and walks the rows
// of a slab; x and dy are read a second time, 10 B per element).  Either way ln_bwd_finalize sums
// the partial rows per column in double in a fixed order and stores or adds into the flat gradient.
// No atomics; the grids are functions of (B, N) alone: every output is the same bits on every run.
//
// Workspace, fp32, nothing in it has to survive a call or be zeroed:  part [partial rows][2][up8(N)].
#include <type_traits>

#include "ldnn_common.h"
#include "ldnn_kernels.h"

namespace ldnn {
namespace {

constexpr int kBlock = 256, kWaves = kBlock / kWave;
constexpr int kPsumVpl = 8;                                  // widest instance with register partials
constexpr int kMaxVpl = 16;                                  // vectors per lane of the widest instance
constexpr int kMaxWidth = kMaxVpl * kWave * 8;               // 8192
constexpr int kMaxSlabs = 128;                               // ln_param_partials: row slabs
constexpr int kFinCols = 16, kFinLanes = kBlock / kFinCols;  // ln_bwd_finalize: columns x partial-row lanes

struct LnGeo {
  int64_t B;
  int64_t ld_x, ld_y, ld_dy, ld_dx;
  int N, Np;     // columns, and rounded up to 8
  int last_c0;   // first column of the row's last vector
  float inv_n, eps;
};

// Workgroups of the row passes: four rows each, at most four per CU of a 256-CU device in the
// forward and two in the backward, whose every workgroup leaves a partial row for the finalize to
// read.  Never a device query or a knob.
int ln_grid(int64_t B, bool fwd) {
  const int64_t cap = fwd ? 1024 : 512;
  const int64_t want = (B + kWaves - 1) / kWaves;
  return (int)(want < cap ? want : cap);
}

bool ln_psum(int64_t N) { return N <= kPsumVpl * kWave * 8; }

// Row slabs of ln_param_partials (rows beyond 4096 columns).
int ln_slabs(int64_t B) {
  const int64_t want = (B + kWaves - 1) / kWaves;
  return (int)(want < kMaxSlabs ? want : kMaxSlabs);
}

int ln_partial_rows(int64_t B, int64_t N) { return ln_psum(N) ? ln_grid(B, false) : ln_slabs(B); }

__device__ __forceinline__ void ld8f(const float* __restrict__ p, float (&v)[8]) {
  const floatx4 a = *reinterpret_cast<const floatx4*>(p), b = *reinterpret_cast<const floatx4*>(p + 4);
  v[0] = a[0], v[1] = a[1], v[2] = a[2], v[3] = a[3];
  v[4] = b[0], v[5] = b[1], v[6] = b[2], v[7] = b[3];
}

// gamma / beta of the vector at column c0 (a lane past the row's end takes the last vector's).
__device__ __forceinline__ void ln_coef(const float* __restrict__ gamma, const float* __restrict__ beta, int c0,
                                        int last_c0, float (&gm)[8], float (&bt)[8]) {
  uint32_t cc = c0 < last_c0 ? c0 : last_c0;
  // (an offset the compiler knows nothing about: the loads stay where they are written, one vector
  // ahead of their use, instead of being merged across passes and rows into registers held throughout)
  asm volatile("" : "+v"(cc));
  ld8f(gamma + cc, gm);
  ld8f(beta + cc, bt);
}

// Between two vectors of an unrolled pass: memory accesses (the coefficient loads of the vector after
// next) and the instruction scheduler stay on their side, which bounds the registers live at once.
__device__ __forceinline__ void ln_fence() {
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

// Between two passes over a row held in registers: the packed vectors come back as values the
// compiler knows nothing about, so each pass unpacks them again instead of keeping the previous
// pass's fp32 copies (8 registers per vector and pass) alive beside them.
template <int VPL>
__device__ __forceinline__ void ln_repack(u16x8 (&v)[VPL]) {
#pragma unroll
  for (int k = 0; k < VPL; ++k) asm volatile("" : "+v"(v[k]));
}

// Columns of the vector at c0 that lie inside the row (<= 0: none), as a value the compiler knows
// nothing about: the eight compares against it are made where they are used, not once per kernel
// and kept (a mask pair per element of the row otherwise outgrows the scalar registers).
__device__ __forceinline__ int ln_nv(int N, int c0) {
  int nv = N - c0;
  asm volatile("" : "+v"(nv));
  return nv;
}

// The pre-activation, one expression for the forward and the backward's recomputation.
template <bool AFFINE>
__device__ __forceinline__ float ln_z(float xhat, float gamma, float beta) {
  if constexpr (AFFINE) return fmaf(gamma, xhat, beta);
  return xhat;
}

// (v_rcp_f32 is good to 1 ulp: the value is rounded to bf16, or scales a bf16 gradient, next)
__device__ __forceinline__ float ln_sigmoid(float z) { return __builtin_amdgcn_rcpf(1.f + __expf(-z)); }

template <int ACT>
__device__ __forceinline__ float ln_act(float z) {
  if constexpr (ACT == LN_ACT_RELU) return fmaxf(z, 0.f);
  if constexpr (ACT == LN_ACT_SIGMOID) return ln_sigmoid(z);
  return z;
}

template <int ACT>
__device__ __forceinline__ float ln_act_grad(float z) {
  if constexpr (ACT == LN_ACT_RELU) return z > 0.f ? 1.f : 0.f;
  if constexpr (ACT == LN_ACT_SIGMOID) {
    const float s = ln_sigmoid(z);
    return s * (1.f - s);
  }
  return 1.f;
}

// One element of the backward: xhat, dz = dy * act'(z) and a = dz * gamma; all 0 or finite outside the
// row (in == false: x, dy, gamma and beta are replaced by select before they are used).
template <int ACT, bool AFFINE>
__device__ __forceinline__ void ln_bwd_elem(bool in, uint16_t xb, uint16_t gb, float mu, float rs, float gmj,
                                            float btj, float& xhat, float& dz, float& a) {
  // every product here is rounded on its own (the flag travels with the inlined instructions): were
  // dz * gamma contracted into the sum of pass 1 or the difference of pass 2, `a - s1` would be the
  // product's rounding error instead of 0 in a one-element row
#pragma clang fp contract(off)
  const float xf = in ? bf2f(xb) : 0.f, gf = in ? bf2f(gb) : 0.f;
  const float gj = AFFINE && in ? gmj : 1.f;
  xhat = (xf - mu) * rs;
  const float z = ln_z<AFFINE>(xhat, gj, AFFINE && in ? btj : 0.f);
  // (every input was selected above, so z is finite and the product with gf = 0 is 0; a select
  // around the activation's derivative instead becomes a branch per element)
  dz = gf * ln_act_grad<ACT>(z);
  a = dz * gj;
}

// Zeros into the pad columns of an output row that lie beyond the instance's register vectors.
template <int VPL>
__device__ __forceinline__ void ln_zero_tail(bf16_t* __restrict__ row, int64_t ld, int lane) {
  const u16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t c0 = (int64_t)(VPL * kWave + lane) * 8; c0 < ld; c0 += kWave * 8)
    *reinterpret_cast<u16x8*>(row + c0) = zero;
}

// The four waves' column partials (ag: sum dz * xhat, ab: sum dz of a lane's vector) added through
// sm[wave][lane][16] in the order of the wave index; row `prow` of part gets the columns of the
// vectors vbase .. vbase + 63.  Every thread of the workgroup calls it.
__device__ __forceinline__ void ln_store_partials(const float (&ag)[8], const float (&ab)[8], float* sm,
                                                  float* __restrict__ part, int64_t prow, int vbase, int N, int Np) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  float* mine = sm + (wave * kWave + lane) * 16;
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    mine[j] = ag[j];
    mine[8 + j] = ab[j];
  }
  __syncthreads();
#pragma unroll
  for (int i = 0; i < kWave * 16 / kBlock; ++i) {
    const int o = i * kBlock + threadIdx.x, l = o >> 4, j = o & 15;
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < kWaves; ++w) t += sm[(w * kWave + l) * 16 + j];
    const int c = (vbase + l) * 8 + (j & 7);
    if (c < N) part[(prow * 2 + (j >> 3)) * Np + c] = t;
  }
}

template <int VPL, int ACT, bool AFFINE>
__global__ __launch_bounds__(kBlock) void ln_fwd_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ beta, float* __restrict__ mean,
                                                        float* __restrict__ rstd, LnGeo g) {
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  for (int64_t r = (int64_t)blockIdx.x * kWaves + wave; r < g.B; r += (int64_t)gridDim.x * kWaves) {
    const bf16_t* xr = x + r * g.ld_x;
    // every lane loads: a lane past the row's end takes the last vector again and discards it
    u16x8 xv[VPL];
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int c0 = (k * kWave + lane) * 8;
      xv[k] = *reinterpret_cast<const u16x8*>(xr + (uint32_t)(c0 < g.last_c0 ? c0 : g.last_c0));
    }
    float s = 0.f;
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int nv = ln_nv(g.N, (k * kWave + lane) * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) s += j < nv ? bf2f(xv[k][j]) : 0.f;
    }
    const float mu = wave_sum(s) * g.inv_n;
    ln_repack(xv);
    float q = 0.f;
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int nv = ln_nv(g.N, (k * kWave + lane) * 8);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float d = j < nv ? bf2f(xv[k][j]) - mu : 0.f;
        q += d * d;
      }
    }
    const float rs = rsqrtf(fmaxf(wave_sum(q) * g.inv_n, 0.f) + g.eps);
    if (lane == 0) {
      mean[r] = mu;
      rstd[r] = rs;
    }
    ln_repack(xv);
    bf16_t* yr = y + r * g.ld_y;
    float gm[2][8] = {}, bt[2][8] = {};
    if constexpr (AFFINE) ln_coef(gamma, beta, lane * 8, g.last_c0, gm[0], bt[0]);
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int c0 = (k * kWave + lane) * 8, nv = ln_nv(g.N, c0);
      if constexpr (AFFINE) {
        if (k + 1 < VPL) ln_coef(gamma, beta, c0 + kWave * 8, g.last_c0, gm[(k + 1) & 1], bt[(k + 1) & 1]);
      }
      ln_fence();
      u16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bool in = j < nv;
        const float xhat = ((in ? bf2f(xv[k][j]) : 0.f) - mu) * rs;
        const float z = ln_z<AFFINE>(xhat, AFFINE && in ? gm[k & 1][j] : 1.f, AFFINE && in ? bt[k & 1][j] : 0.f);
        o[j] = f2bf(ln_act<ACT>(z)) & (in ? (uint16_t)0xFFFFu : (uint16_t)0);   // (a select of bits: no branch)
      }
      if (c0 < g.ld_y) *reinterpret_cast<u16x8*>(yr + c0) = o;
    }
    ln_zero_tail<VPL>(yr, g.ld_y, lane);
  }
}

// PSUM: the lane's dgamma / dbeta column partials in registers (needs AFFINE).
template <int VPL, int ACT, bool AFFINE, bool PSUM>
__global__ __launch_bounds__(kBlock) void ln_bwd_kernel(const bf16_t* __restrict__ x, const bf16_t* __restrict__ dy,
                                                        const float* __restrict__ gamma,
                                                        const float* __restrict__ beta,
                                                        const float* __restrict__ mean,
                                                        const float* __restrict__ rstd, bf16_t* __restrict__ dx,
                                                        float* __restrict__ part, LnGeo g) {
  static_assert(AFFINE || !PSUM, "parameter sums belong to an affine layer");
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  float ag[PSUM ? VPL : 1][8], ab[PSUM ? VPL : 1][8];
#pragma unroll
  for (int k = 0; k < (PSUM ? VPL : 1); ++k) {
#pragma unroll
    for (int j = 0; j < 8; ++j) ag[k][j] = 0.f, ab[k][j] = 0.f;
  }
  for (int64_t r = (int64_t)blockIdx.x * kWaves + wave; r < g.B; r += (int64_t)gridDim.x * kWaves) {
    const bf16_t* xr = x + r * g.ld_x;
    const bf16_t* gr = dy + r * g.ld_dy;
    u16x8 xv[VPL], gv[VPL];
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int c0 = (k * kWave + lane) * 8;
      const uint32_t cc = c0 < g.last_c0 ? c0 : g.last_c0;
      xv[k] = *reinterpret_cast<const u16x8*>(xr + cc);
      gv[k] = *reinterpret_cast<const u16x8*>(gr + cc);
    }
    const float mu = mean[r], rs = rstd[r];
    float s1 = 0.f, s2 = 0.f;
    float gm[2][8] = {}, bt[2][8] = {};
    if constexpr (AFFINE) ln_coef(gamma, beta, lane * 8, g.last_c0, gm[0], bt[0]);
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int c0 = (k * kWave + lane) * 8, nv = ln_nv(g.N, c0);
      if constexpr (AFFINE) {
        if (k + 1 < VPL) ln_coef(gamma, beta, c0 + kWave * 8, g.last_c0, gm[(k + 1) & 1], bt[(k + 1) & 1]);
      }
      ln_fence();
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float xhat, dz, a;
        ln_bwd_elem<ACT, AFFINE>(j < nv, xv[k][j], gv[k][j], mu, rs, gm[k & 1][j], bt[k & 1][j], xhat, dz, a);
        s1 += a;
        s2 += a * xhat;
        if constexpr (PSUM) {
          ag[k][j] += dz * xhat;
          ab[k][j] += dz;
        }
      }
    }
    s1 = wave_sum(s1) * g.inv_n;
    s2 = wave_sum(s2) * g.inv_n;
    ln_repack(xv);
    ln_repack(gv);
    bf16_t* dr = dx + r * g.ld_dx;
    if constexpr (AFFINE) ln_coef(gamma, beta, lane * 8, g.last_c0, gm[0], bt[0]);
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const int c0 = (k * kWave + lane) * 8, nv = ln_nv(g.N, c0);
      if constexpr (AFFINE) {
        if (k + 1 < VPL) ln_coef(gamma, beta, c0 + kWave * 8, g.last_c0, gm[(k + 1) & 1], bt[(k + 1) & 1]);
      }
      ln_fence();
      u16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float xhat, dz, a;
        ln_bwd_elem<ACT, AFFINE>(j < nv, xv[k][j], gv[k][j], mu, rs, gm[k & 1][j], bt[k & 1][j], xhat, dz, a);
        o[j] = f2bf(rs * (a - s1 - xhat * s2)) & (j < nv ? (uint16_t)0xFFFFu : (uint16_t)0);
      }
      if (c0 < g.ld_dx) *reinterpret_cast<u16x8*>(dr + c0) = o;
    }
    ln_zero_tail<VPL>(dr, g.ld_dx, lane);
  }
  if constexpr (PSUM) {
    __shared__ float sm[kWaves * kWave * 16];
#pragma unroll
    for (int k = 0; k < VPL; ++k) ln_store_partials(ag[k], ab[k], sm, part, blockIdx.x, k * kWave, g.N, g.Np);
  }
}

// The parameter sums of rows too wide for register partials.  grid (ceil(Np / 8 / 64), slabs): a
// lane owns the vector column blockIdx.x * 64 + lane, wave w the rows w, w + 4, ... of slab blockIdx.y.
template <int ACT>
__global__ __launch_bounds__(kBlock) void ln_param_partials_kernel(const bf16_t* __restrict__ x,
                                                                   const bf16_t* __restrict__ dy,
                                                                   const float* __restrict__ gamma,
                                                                   const float* __restrict__ beta,
                                                                   const float* __restrict__ mean,
                                                                   const float* __restrict__ rstd,
                                                                   float* __restrict__ part, int64_t rows_per_slab,
                                                                   LnGeo g) {
  __shared__ float sm[kWaves * kWave * 16];
  const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  const int c0 = (blockIdx.x * kWave + lane) * 8, nv = g.N - c0;
  float ag[8], ab[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) ag[j] = 0.f, ab[j] = 0.f;
  if (nv > 0) {
    float gm[8], bt[8];
    ln_coef(gamma, beta, c0, g.last_c0, gm, bt);
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_slab;
    const int64_t r1 = r0 + rows_per_slab < g.B ? r0 + rows_per_slab : g.B;
#pragma unroll 2
    for (int64_t r = r0 + wave; r < r1; r += kWaves) {
      const u16x8 xv = *reinterpret_cast<const u16x8*>(x + r * g.ld_x + c0);
      const u16x8 gv = *reinterpret_cast<const u16x8*>(dy + r * g.ld_dy + c0);
      const float mu = mean[r], rs = rstd[r];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float xhat, dz, a;
        ln_bwd_elem<ACT, true>(j < nv, xv[j], gv[j], mu, rs, gm[j], bt[j], xhat, dz, a);
        ag[j] += dz * xhat;
        ab[j] += dz;
      }
    }
  }
  ln_store_partials(ag, ab, sm, part, blockIdx.y, blockIdx.x * kWave, g.N, g.Np);
}

// One workgroup per 16 columns: lane q of 16 sums the partial rows q, q + 16, ... in order in double
// (unrolled: the loads of eight rows are in flight together, the additions keep their order), the
// sixteen are added in order, the total is stored (assign) or added to the gradient.
__global__ __launch_bounds__(kBlock) void ln_bwd_finalize_kernel(const float* __restrict__ part, int prows, int N,
                                                                 int Np, float* __restrict__ dgamma,
                                                                 float* __restrict__ dbeta, int assign) {
  __shared__ double sm[2 * kBlock];
  const int cl = threadIdx.x & (kFinCols - 1), q = threadIdx.x / kFinCols;
  const int c = blockIdx.x * kFinCols + cl;
  double dg = 0.0, db = 0.0;
  if (c < N) {
#pragma unroll 8
    for (int w = q; w < prows; w += kFinLanes) {
      const float* p = part + (int64_t)w * 2 * Np + c;
      dg += (double)p[0];
      db += (double)p[Np];
    }
  }
  sm[threadIdx.x] = dg;
  sm[kBlock + threadIdx.x] = db;
  __syncthreads();
  if (q == 0 && c < N) {
    double tg = 0.0, tb = 0.0;
    for (int l = 0; l < kFinLanes; ++l) {
      tg += sm[l * kFinCols + cl];
      tb += sm[kBlock + l * kFinCols + cl];
    }
    dgamma[c] = assign ? (float)tg : dgamma[c] + (float)tg;
    dbeta[c] = assign ? (float)tb : dbeta[c] + (float)tb;
  }
}

bool ln_args_ok(const LnArgs& a) {
  if (a.x == nullptr || a.mean == nullptr || a.rstd == nullptr) return false;
  if (a.B < 1 || a.N < 1 || a.N > kMaxWidth) return false;
  if ((a.gamma == nullptr) != (a.beta == nullptr)) return false;
  if (a.act != LN_ACT_NONE && a.act != LN_ACT_RELU && a.act != LN_ACT_SIGMOID) return false;
  return ((reinterpret_cast<uintptr_t>(a.gamma) | reinterpret_cast<uintptr_t>(a.beta)) & 15) == 0;
}

bool ln_ld_ok(const void* p, int64_t ld, const LnArgs& a) {
  return p != nullptr && ld >= a.N && ld % 8 == 0 && (reinterpret_cast<uintptr_t>(p) & 15) == 0 &&
         a.B <= INT64_MAX / 4 / ld;   // (element and byte offsets stay in int64)
}

LnGeo ln_geometry(const LnArgs& a) {
  LnGeo g{};
  g.B = a.B, g.N = (int)a.N, g.Np = (int)((a.N + 7) / 8 * 8);
  g.ld_x = a.ld_x;
  g.last_c0 = (int)((a.N - 1) / 8 * 8);
  g.inv_n = 1.f / (float)a.N;
  g.eps = a.eps;
  return g;
}

template <typename F>
void ln_with_act(int act, F&& f) {
  if (act == LN_ACT_RELU) f(std::integral_constant<int, LN_ACT_RELU>{});
  else if (act == LN_ACT_SIGMOID) f(std::integral_constant<int, LN_ACT_SIGMOID>{});
  else f(std::integral_constant<int, LN_ACT_NONE>{});
}

// f(VPL, ACT, AFFINE tags) for the instance of a call: the narrowest that holds the row.
template <typename F>
void ln_dispatch(int64_t N, int act, bool affine, F&& f) {
  auto with_vpl = [&](auto vpl) {
    ln_with_act(act, [&](auto a) {
      if (affine) f(vpl, a, std::true_type{});
      else f(vpl, a, std::false_type{});
    });
  };
  if (N <= 512) with_vpl(std::integral_constant<int, 1>{});
  else if (N <= 1024) with_vpl(std::integral_constant<int, 2>{});
  else if (N <= 2048) with_vpl(std::integral_constant<int, 4>{});
  else if (N <= 4096) with_vpl(std::integral_constant<int, 8>{});
  else with_vpl(std::integral_constant<int, 16>{});
}

}  // namespace

int ln_max_width() { return kMaxWidth; }

int64_t ln_workspace_floats(int64_t B, int64_t N) {
  if (B < 1 || N < 1) return 0;
  return (int64_t)ln_partial_rows(B, N) * 2 * ((N + 7) / 8 * 8);
}

hipError_t ln_forward(const LnArgs& a, uint16_t* y, int64_t ld_y, hipStream_t s) {
  if (!ln_args_ok(a) || !ln_ld_ok(a.x, a.ld_x, a) || !ln_ld_ok(y, ld_y, a) || y == a.x) return hipErrorInvalidValue;
  LnGeo g = ln_geometry(a);
  g.ld_y = ld_y;
  const int grid = ln_grid(a.B, true);
  ln_dispatch(a.N, a.act, a.gamma != nullptr, [&](auto vpl, auto act, auto affine) {
    ln_fwd_kernel<decltype(vpl)::value, decltype(act)::value, decltype(affine)::value>
        <<<grid, kBlock, 0, s>>>(a.x, y, a.gamma, a.beta, a.mean, a.rstd, g);
  });
  return hipGetLastError();
}

hipError_t ln_backward(const LnArgs& a, const uint16_t* dy, int64_t ld_dy, uint16_t* dx, int64_t ld_dx, float* ws,
                       float* dgamma, float* dbeta, bool grad_assign, hipStream_t s) {
  if (!ln_args_ok(a) || !ln_ld_ok(a.x, a.ld_x, a) || !ln_ld_ok(dy, ld_dy, a) || !ln_ld_ok(dx, ld_dx, a))
    return hipErrorInvalidValue;
  if (dx == a.x || dx == dy) return hipErrorInvalidValue;
  const bool affine = a.gamma != nullptr;
  // parameter gradients exist exactly for an affine layer, both or neither, with their workspace
  if ((dgamma == nullptr) != (dbeta == nullptr) || (dgamma != nullptr) != affine) return hipErrorInvalidValue;
  if (affine && (ws == nullptr || (reinterpret_cast<uintptr_t>(ws) & 15))) return hipErrorInvalidValue;
  LnGeo g = ln_geometry(a);
  g.ld_dy = ld_dy, g.ld_dx = ld_dx;
  const int grid = ln_grid(a.B, false);
  ln_dispatch(a.N, a.act, affine, [&](auto vpl, auto act, auto aff) {
    constexpr int VPL = decltype(vpl)::value;
    constexpr bool AFF = decltype(aff)::value;
    ln_bwd_kernel<VPL, decltype(act)::value, AFF, AFF && VPL <= kPsumVpl>
        <<<grid, kBlock, 0, s>>>(a.x, dy, a.gamma, a.beta, a.mean, a.rstd, dx, ws, g);
  });
  if (!affine) return hipGetLastError();
  if (!ln_psum(a.N)) {
    const int S = ln_slabs(a.B);
    const int64_t rps = ((a.B + S - 1) / S + kWaves - 1) / kWaves * kWaves;
    const dim3 pgrid((g.Np / 8 + kWave - 1) / kWave, S);
    ln_with_act(a.act, [&](auto act) {
      ln_param_partials_kernel<decltype(act)::value>
          <<<pgrid, kBlock, 0, s>>>(a.x, dy, a.gamma, a.beta, a.mean, a.rstd, ws, rps, g);
    });
  }
  ln_bwd_finalize_kernel<<<(g.N + kFinCols - 1) / kFinCols, kBlock, 0, s>>>(ws, ln_partial_rows(a.B, a.N), g.N, g.Np,
                                                                           dgamma, dbeta, grad_assign ? 1 : 0);
  return hipGetLastError();
}

}  // namespace ldnn
