// Fused softmax cross-entropy forward + backward + accuracy (SURVEY §2.3 K14,
// K15, K21): one kernel replaces the reference's nn.CrossEntropyLoss forward
// (BAR/main.py:52, BAR/trainer.py:207), its autograd backward, the argmax /
// (pred == labels).sum() of BAR/trainer.py:213-215 and the three per-step
// .item() host syncs (loss and correct count are accumulated on the device).
// It also emits the last Linear layer's bias gradient (column sums of dlogits).
//
// One wave per row (lanes stride over classes), 4 waves per block, 16 rows per
// block; per-block partials are combined in LDS and added with one atomic per
// statistic / bias column.
//
// Label smoothing (torch's label_smoothing=eps, mean reduction) is a compile-time
// SMOOTH instance of both kernels: targets q_c = eps/C + (1-eps)[c == label], so
//   loss_r = logsumexp(x_r) - (1-eps) x_r[label] - (eps/C) sum_{c<C} x_r[c]
//   dlogits = (softmax - q) * grad_scale
// on the same loads, stores and single launch; the row sum is one more wave_sum per
// row in the wave kernel and a register sum in the rows kernel.  conf = 1-eps and
// epsc = eps/C are formed on the host.  The plain (XM_PLAIN) instances are the code
// as it was.
//
// Soft targets (torch's class-probability targets, XM_SOFT): the kernels read a row of
// fp32 targets q_r (row stride ldq >= C) instead of a label.  With q'_c = conf q_c + epsc
// and s = sum_c q'_c (NOT assumed 1: torch does not normalise),
//   loss_r = s logsumexp(x_r) - sum_c q'_c x_r[c]
//   dlogits = (softmax s - q') * grad_scale
// and a row counts as correct when the first-index argmax of its logits is the
// first-index argmax of q_r over c < C.  One instance serves eps = 0 and eps > 0.
// The rows kernel (a lane owns a row) reads q with 16-B loads where ldq % 4 == 0 and
// the base is 16-B aligned (the last, partial group of a row and every other layout:
// 4-B loads); in the wave kernel lanes stride over the classes, so its 4-B loads are
// already whole 256-B lines per wave instruction.  The LD = 64 rows instance holds
// x, q' and the rounded gradient per lane without scratch (compiler output in
// profiles/r13), so the soft mode keeps the plain mode's split between the kernels.
//
// Class weights and ignore_index (torch's weight= / ignore_index=, mean reduction; XM_W for
// labels, XM_WSOFT for class-probability targets): the soft-target formula applied to
// t_c = w_c q'_c.  The weights w (fp32 [C], or all 1 when none are given) are staged once per
// workgroup into LDS.  Under labels the divisor is den = sum of w[label] over the kept rows (a
// row is kept when its label is neither ignore_index nor outside [0, C)); xent_wden_kernel, one
// workgroup reducing in a fixed order, writes {den, den > 0 ? 1 / den : 0, #kept} into a
// persistent workspace in front of the loss launch, which reads 1 / den from there: no host sync,
// the same bits on every run, and an all-ignored batch gives loss 0 and zero gradients (torch:
// NaN).  An ignored row writes a zero gradient row and adds nothing to the loss, #correct or
// dbias.  The finalize writes out[0] = weighted loss sum / den and adds B * out[0] into stats[0]
// ("loss sum / samples" stays the mean loss).  Under probability targets den = B comes from the
// host as before.  The PLAIN / SMOOTH / SOFT instances are the code as it was.
//
// Focal loss (Lin et al. 2017; XM_FOCAL, labels only, no smoothing): with a = w[y], p = softmax(x)[y],
// q = 1 - p, nlp = -log p and m = q^gamma a kept row has
//   loss_r  = a m nlp
//   dlogits = a f (softmax - onehot) / den,   f = m + gamma p q^(gamma-1) nlp = m (1 + gamma p nlp / q)
// i.e. the cross-entropy gradient row times one scalar per row, on the XM_W machinery (staged weights, the
// den pre-pass, ignored rows, the finalize).  q is formed from the other classes' exponentials,
// sum_{c != y} e_c / sum_c e_c (no cancellation; one more wave_sum in the wave kernel, a register sum in
// the rows kernel), and nlp as -log1p(-q) where q < 1/2 (lse - x_y cancels there), lse - x_y otherwise.
// A row whose q is below the smallest normal fp32 (p rounds to 1) takes m = f = 0: loss 0 and a zero gradient
// row, q^(gamma-1) is never formed at 0 and nothing stored is NaN or inf.  gamma (> 0: the host sends 0 to
// XM_W) travels in the `conf` argument, which like epsc and the host's grad_scale this mode does not use.
#include <algorithm>

#include "ldnn_common.h"
#include "ldnn_kernels.h"

namespace ldnn {

namespace {

constexpr int kRowsPerBlock = 16;  // 4 rows per wave: B = 4096 -> 256 blocks fill the chip
constexpr int kMaxColsPerLane = 16;  // C <= 1024

enum XentMode { XM_PLAIN = 0, XM_SMOOTH = 1, XM_SOFT = 2, XM_W = 3, XM_WSOFT = 4, XM_FOCAL = 5 };

// The focal row scalars from q = sum_{c != y} e_c / sum_c e_c, p = e_y / sum_c e_c and lse - x_y:
// m = q^gamma and f = m (1 + gamma p nlp / q), both 0 once q is below the smallest normal fp32; returns nlp.
// nlp / q -> 1 as q -> 0 and p nlp <= 1 / e, so no factor overflows for any finite gamma > 0.
__device__ __forceinline__ float focal_terms(float q, float p, float lse_m_xl, float gamma, float& m, float& f) {
  m = f = 0.f;
  if (!(q >= 1.17549435e-38f)) return 0.f;
  const float nlp = q < 0.5f ? -log1pf(-q) : lse_m_xl;
  m = __builtin_amdgcn_exp2f(gamma * __builtin_amdgcn_logf(q));  // v_exp_f32 / v_log_f32 are base 2
  f = m + (gamma * m) * (p * (nlp / q));
  return nlp;
}

// Last-block finalize (fin.out set): every block's statistic atomics are made
// device-visible before its arrival is counted; the last arrival swaps the sums
// out of the accumulator (leaving it zero), writes [loss_sum * scale, #correct]
// and adds both into the running stats.
// XM_W / XM_FOCAL: the scale is the pre-pass's 1 / den (device), and stats[0] gains B * out[0].
template <int MODE = XM_PLAIN>
__device__ __forceinline__ void xent_finish(const XentFin& fin, float* stats, const float* wden = nullptr,
                                            int B = 0) {
  if (fin.out == nullptr) return;
  __threadfence();
  __syncthreads();
  __shared__ int last;
  if (threadIdx.x == 0) last = atomicAdd(fin.cnt, 1u) == gridDim.x - 1;
  __syncthreads();
  if (!last || threadIdx.x != 0) return;
  __threadfence();
  const float l = atomicExch(fin.acc, 0.f), c = atomicExch(fin.acc + 1, 0.f);
  if constexpr (MODE == XM_W || MODE == XM_FOCAL) {
    const float o = l * wden[1];
    fin.out[0] = o;
    fin.out[1] = c;
    if (stats) {
      atomicAdd(stats, o * (float)B);
      atomicAdd(stats + 1, c);
    }
  } else {
    fin.out[0] = l * fin.scale;
    fin.out[1] = c;
    if (stats) {
      atomicAdd(stats, l);
      atomicAdd(stats + 1, c);
    }
  }
  atomicExch(fin.cnt, 0u);
}

// The denominator pre-pass of the weighted loss over labels: ws = {den, den > 0 ? 1 / den : 0,
// #kept rows}, den = sum over the kept rows of w[label] (w == nullptr: 1).  One workgroup; a
// thread sums its rows in row order, a wave its lanes by the fixed shuffle tree, thread 0 the
// four wave sums in wave order: no atomics, the same bits on every run.
__global__ __launch_bounds__(256) void xent_wden_kernel(const int64_t* __restrict__ labels,
                                                        const float* __restrict__ wt, int B, int C,
                                                        int64_t ignore_index, float* __restrict__ ws) {
  __shared__ float part[4][2];
  float den = 0.f, kept = 0.f;
  for (int r = threadIdx.x; r < B; r += 256) {
    const int64_t lab = labels[r];
    if (lab != ignore_index && lab >= 0 && lab < (int64_t)C) {
      den += wt ? wt[lab] : 1.f;
      kept += 1.f;
    }
  }
  den = wave_sum(den);
  kept = wave_sum(kept);
  if ((threadIdx.x & 63) == 0) {
    part[threadIdx.x >> 6][0] = den;
    part[threadIdx.x >> 6][1] = kept;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const float d = ((part[0][0] + part[1][0]) + part[2][0]) + part[3][0];
    ws[0] = d;
    ws[1] = d > 0.f ? 1.f / d : 0.f;
    ws[2] = ((part[0][1] + part[1][1]) + part[2][1]) + part[3][1];
  }
}

__global__ __launch_bounds__(256) void scale_bf16_kernel(const bf16_t* __restrict__ src, const float* __restrict__ scale,
                                                         bf16_t* __restrict__ out, int64_t n8) {
  const float k = *scale;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n8; i += stride) {
    const u16x8 v = reinterpret_cast<const u16x8*>(src)[i];
    u16x8 o;
#pragma unroll
    for (int j = 0; j < 8; ++j) o[j] = f2bf(bf2f(v[j]) * k);
    reinterpret_cast<u16x8*>(out)[i] = o;
  }
}

template <int MODE>
__global__ __launch_bounds__(256) void xent_kernel(const bf16_t* __restrict__ logits,
                                                   const int64_t* __restrict__ labels,
                                                   bf16_t* __restrict__ dlogits, float* __restrict__ stats,
                                                   float* __restrict__ dbias, int B, int C, int ld,
                                                   float grad_scale, int rows_per_block, XentFin fin,
                                                   float conf, float epsc, const float* __restrict__ q,
                                                   int ldq, const float* __restrict__ wt,
                                                   const float* __restrict__ wden, int64_t ignore_index) {
  // QLOAD: the targets are rows of q; SOFT: the loss / gradient take the soft-target form
  // (t = q', or w (.) q' in the weighted modes, where XM_W builds q' from the label)
  constexpr bool SMOOTH = MODE == XM_SMOOTH, QLOAD = MODE == XM_SOFT || MODE == XM_WSOFT;
  constexpr bool WH = MODE == XM_W, SOFT = QLOAD || WH;
  // FOCAL shares XM_W's label handling, 1 / den and finalize (WL) and the staged weights (WT)
  constexpr bool FOCAL = MODE == XM_FOCAL, WL = WH || FOCAL, WT = WL || MODE == XM_WSOFT;
  __shared__ float sdb[4][kMaxColsPerLane * 64];
  __shared__ float sstat[4][2];
  __shared__ float sw[WT ? kMaxColsPerLane * 64 : 1];  // the class weights (C <= ld <= 1024: 4 KB)
  if constexpr (WT) {
    for (int c = threadIdx.x; c < C; c += 256) sw[c] = wt ? wt[c] : 1.f;
    __syncthreads();
    if constexpr (WL) grad_scale = wden[1];  // 1 / den of the pre-pass (0: nothing kept)
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int nt = (ld + 63) / 64;
  float dacc[kMaxColsPerLane];
#pragma unroll
  for (int t = 0; t < kMaxColsPerLane; ++t) dacc[t] = 0.f;
  float loss_sum = 0.f, correct = 0.f;

  const int r_end = min(B, (blockIdx.x + 1) * rows_per_block);
  for (int r = blockIdx.x * rows_per_block + w; r < r_end; r += 4) {
    const bf16_t* row = logits + (size_t)r * ld;
    int lab = 0;
    if constexpr (WL) {
      const int64_t l64 = labels[r];
      if (l64 == ignore_index || l64 < 0 || l64 >= (int64_t)C) {
        // ignored (or not a class: never indexes w or the row): a zero gradient row, nothing else
#pragma unroll
        for (int t = 0; t < kMaxColsPerLane; ++t) {
          const int c = lane + 64 * t;
          if (t < nt && c < ld) dlogits[(size_t)r * ld + c] = 0;
        }
        continue;
      }
      lab = (int)l64;
    } else if constexpr (!QLOAD) {
      lab = (int)labels[r];
    }
    float xv[kMaxColsPerLane];
    float mx = -INFINITY;
    int amax = 0x7fffffff;
#pragma unroll
    for (int t = 0; t < kMaxColsPerLane; ++t) {
      const int c = lane + 64 * t;
      xv[t] = -INFINITY;
      if (t < nt && c < C) {
        xv[t] = bf2f(row[c]);
        if (xv[t] > mx) { mx = xv[t]; amax = c; }
      }
    }
    float qv[SOFT ? kMaxColsPerLane : 1];  // q' = conf q + epsc (0 beyond C); weighted: w (.) q'
    if constexpr (WH) {
#pragma unroll
      for (int t = 0; t < kMaxColsPerLane; ++t) {
        const int c = lane + 64 * t;
        qv[t] = 0.f;
        if (t < nt && c < C) qv[t] = sw[c] * (c == lab ? conf + epsc : epsc);
      }
    }
    if constexpr (QLOAD) {
      const float* qrow = q + (size_t)r * ldq;
      float qm = -INFINITY;
      int qa = 0x7fffffff;
#pragma unroll
      for (int t = 0; t < kMaxColsPerLane; ++t) {
        const int c = lane + 64 * t;
        qv[t] = 0.f;
        if (t < nt && c < C) {
          const float v = qrow[c];
          if (v > qm) { qm = v; qa = c; }
          qv[t] = conf * v + epsc;
          if constexpr (WT) qv[t] *= sw[c];
        }
      }
      // the targets' first-index argmax stands in for the label
      const float wqm = wave_max(qm);
      lab = (qm == wqm) ? qa : 0x7fffffff;
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) lab = min(lab, __shfl_xor(lab, o, 64));
    }
    // wave argmax (first index of the max)
    const float wmx = wave_max(mx);
    int cand = (mx == wmx) ? amax : 0x7fffffff;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) cand = min(cand, __shfl_xor(cand, o, 64));
    float se = 0.f, xl = 0.f, sx = 0.f;
#pragma unroll
    for (int t = 0; t < kMaxColsPerLane; ++t) {
      const int c = lane + 64 * t;
      if (t < nt && c < C) {
        if constexpr (FOCAL) {
          const float e = __expf(xv[t] - wmx);
          se += e;
          if (c == lab) xl = xv[t];
          else sx += e;  // the other classes' exponentials
          continue;
        }
        se += __expf(xv[t] - wmx);
        if constexpr (SOFT) {
          xl += qv[t] * xv[t];  // sum q' x
          sx += qv[t];          // s = sum q'
        } else {
          if (c == lab) xl = xv[t];
          if constexpr (SMOOTH) sx += xv[t];
        }
      }
    }
    se = wave_sum(se);
    xl = wave_sum(xl);
    if constexpr (SMOOTH || SOFT || FOCAL) sx = wave_sum(sx);
    const float lse = wmx + __logf(se);
    float inv = 1.f / se;
    if constexpr (SOFT) inv *= sx;
    if constexpr (FOCAL) {
      // from here on sx is the row's loss a m nlp and xl its gradient factor a f / den
      float m, f;
      const float nlp = focal_terms(sx * inv, __expf(xl - wmx) * inv, lse - xl, conf, m, f);
      sx = sw[lab] * m * nlp;
      xl = sw[lab] * f * grad_scale;
    }
#pragma unroll
    for (int t = 0; t < kMaxColsPerLane; ++t) {
      const int c = lane + 64 * t;
      if (t < nt && c < ld) {
        float g = 0.f;
        if constexpr (FOCAL) {
          if (c < C) g = (__expf(xv[t] - wmx) * inv - (c == lab ? 1.f : 0.f)) * xl;
        } else if constexpr (SOFT) {
          if (c < C) g = (__expf(xv[t] - wmx) * inv - qv[t]) * grad_scale;
        } else if constexpr (SMOOTH) {
          if (c < C) g = (__expf(xv[t] - wmx) * inv - (c == lab ? conf + epsc : epsc)) * grad_scale;
        } else {
          if (c < C) g = (__expf(xv[t] - wmx) * inv - (c == lab ? 1.f : 0.f)) * grad_scale;
        }
        const uint16_t gb = f2bf(g);
        dlogits[(size_t)r * ld + c] = gb;
        dacc[t] += bf2f(gb);
      }
    }
    if (lane == 0) {
      if constexpr (FOCAL) loss_sum += sx;
      else if constexpr (SOFT) loss_sum += sx * lse - xl;
      else if constexpr (SMOOTH) loss_sum += lse - conf * xl - epsc * sx;
      else loss_sum += lse - xl;
      correct += (cand == lab) ? 1.f : 0.f;
    }
  }

  if (lane == 0) {
    sstat[w][0] = loss_sum;
    sstat[w][1] = correct;
  }
  if (dbias) {
#pragma unroll
    for (int t = 0; t < kMaxColsPerLane; ++t)
      if (t < nt) sdb[w][lane + 64 * t] = dacc[t];
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    float* st = fin.out ? fin.acc : stats;
    if constexpr (WL) {
      // straight into stats: this block's share of B * (weighted loss sum / den)
      const float k = fin.out ? 1.f : grad_scale * (float)B;
      atomicAdd(st + 0, (sstat[0][0] + sstat[1][0] + sstat[2][0] + sstat[3][0]) * k);
    } else {
      atomicAdd(st + 0, sstat[0][0] + sstat[1][0] + sstat[2][0] + sstat[3][0]);
    }
    atomicAdd(st + 1, sstat[0][1] + sstat[1][1] + sstat[2][1] + sstat[3][1]);
  }
  if (dbias) {
    for (int c = threadIdx.x; c < ld; c += blockDim.x)
      atomicAdd(dbias + c, sdb[0][c] + sdb[1][c] + sdb[2][c] + sdb[3][c]);
  }
  xent_finish<MODE>(fin, stats, wden, B);
}


// Small class counts (ld <= 64, e.g. 10 classes padded to 16): one ROW PER LANE.
// A lane reads its whole row with 16-B loads and needs no cross-lane reduction,
// so a 4096-row batch is one load round trip instead of a chain of wave
// shuffles per row.  Column sums for the bias gradient: per-column wave
// reduction, then one atomic per column per wave.
template <int LD, int MODE>
__global__ __launch_bounds__(256) void xent_rows_kernel(const bf16_t* __restrict__ logits,
                                                        const int64_t* __restrict__ labels,
                                                        bf16_t* __restrict__ dlogits, float* __restrict__ stats,
                                                        float* __restrict__ dbias, int B, int C, int ld,
                                                        float grad_scale, XentFin fin, float conf, float epsc,
                                                        const float* __restrict__ q, int ldq, bool qvec,
                                                        const float* __restrict__ wt,
                                                        const float* __restrict__ wden, int64_t ignore_index) {
  constexpr bool SMOOTH = MODE == XM_SMOOTH, QLOAD = MODE == XM_SOFT || MODE == XM_WSOFT;
  constexpr bool WH = MODE == XM_W, SOFT = QLOAD || WH;
  // FOCAL shares XM_W's label handling, 1 / den and finalize (WL) and the staged weights (WT)
  constexpr bool FOCAL = MODE == XM_FOCAL, WL = WH || FOCAL, WT = WL || MODE == XM_WSOFT;
  __shared__ float sw[WT ? LD : 1];  // the class weights (0 beyond C): every lane reads the same word
  if constexpr (WT) {
    if (threadIdx.x < LD) sw[threadIdx.x] = (int)threadIdx.x < C ? (wt ? wt[threadIdx.x] : 1.f) : 0.f;
    __syncthreads();
    if constexpr (WL) grad_scale = wden[1];  // 1 / den of the pre-pass (0: nothing kept)
  }
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  const bool ok = r < B;
  float x[LD];
  float loss = 0.f, correct = 0.f;
  float g[LD];
#pragma unroll
  for (int c = 0; c < LD; ++c) g[c] = 0.f;
  if (ok) {
    const u16x8* row = reinterpret_cast<const u16x8*>(logits + (size_t)r * ld);
#pragma unroll
    for (int v = 0; v < LD / 8; ++v) {
      const u16x8 q = row[v];
#pragma unroll
      for (int j = 0; j < 8; ++j) x[v * 8 + j] = bf2f(q[j]);
    }
    int lab = 0;
    bool keep = true;  // XM_W / XM_FOCAL: false for an ignored label and for one that is no class
    if constexpr (WL) {
      const int64_t l64 = labels[r];
      keep = l64 != ignore_index && l64 >= 0 && l64 < (int64_t)C;
      lab = keep ? (int)l64 : 0;
    } else if constexpr (!QLOAD) {
      lab = (int)labels[r];
    }
    float mx = -INFINITY;
    int am = 0;
#pragma unroll
    for (int c = 0; c < LD; ++c)
      if (c < C && x[c] > mx) { mx = x[c]; am = c; }
    float se = 0.f, xl = 0.f, sx = 0.f;
    float qv[SOFT ? LD : 1];  // q' = conf q + epsc (0 beyond C); weighted: w (.) q'
    if constexpr (WH) {
#pragma unroll
      for (int c = 0; c < LD; ++c) {
        qv[c] = 0.f;
        if (c < C) {
          qv[c] = sw[c] * (c == lab ? conf + epsc : epsc);
          sx += qv[c];
          xl += qv[c] * x[c];
        }
      }
    } else if constexpr (QLOAD) {
      const float* qrow = q + (size_t)r * ldq;
#pragma unroll
      for (int v = 0; v < LD / 4; ++v) {
        floatx4 t = {0.f, 0.f, 0.f, 0.f};
        if (qvec && 4 * v + 3 < C) {
          t = reinterpret_cast<const floatx4*>(qrow)[v];
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (4 * v + j < C) t[j] = qrow[4 * v + j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) qv[4 * v + j] = t[j];
      }
      float qm = -INFINITY;
#pragma unroll
      for (int c = 0; c < LD; ++c) {
        if (c < C) {
          if (qv[c] > qm) { qm = qv[c]; lab = c; }  // first-index argmax of the raw targets
          qv[c] = conf * qv[c] + epsc;
          if constexpr (WT) qv[c] *= sw[c];
          sx += qv[c];          // s = sum q'
          xl += qv[c] * x[c];   // sum q' x
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < LD; ++c)
        if (c == lab) xl = x[c];
    }
#pragma unroll
    for (int c = 0; c < LD; ++c) {
      if (c < C) {
        if constexpr (SMOOTH) sx += x[c];
        x[c] = __expf(x[c] - mx);
        se += x[c];
      }
    }
    if constexpr (SOFT) loss = sx * (mx + __logf(se)) - xl;
    else if constexpr (SMOOTH) loss = mx + __logf(se) - conf * xl - epsc * sx;
    else loss = mx + __logf(se) - xl;  // = logsumexp - x_label
    correct = (am == lab) ? 1.f : 0.f;
    if constexpr (FOCAL) {
      float el = 0.f, so = 0.f;  // the label's exponential and the other classes' sum
#pragma unroll
      for (int c = 0; c < LD; ++c) {
        if (c < C) {
          if (c == lab) el = x[c];
          else so += x[c];
        }
      }
      // from here on loss is the row's a m nlp and xl its gradient factor a f / den
      float m, f;
      const float nlp = focal_terms(so / se, el / se, loss, conf, m, f);
      loss = sw[lab] * m * nlp;
      xl = sw[lab] * f * grad_scale;
    }
    if constexpr (WL) {
      if (!keep) loss = correct = 0.f;
    }
    float inv = 1.f / se;
    if constexpr (SOFT) inv *= sx;
    u16x8 out[LD / 8];
#pragma unroll
    for (int c = 0; c < LD; ++c) {
      float v = 0.f;
      if constexpr (FOCAL) {
        if (c < C) v = (x[c] * inv - (c == lab ? 1.f : 0.f)) * xl;
      } else if constexpr (SOFT) {
        if (c < C) v = (x[c] * inv - qv[c]) * grad_scale;
      } else if constexpr (SMOOTH) {
        if (c < C) v = (x[c] * inv - (c == lab ? conf + epsc : epsc)) * grad_scale;
      } else {
        if (c < C) v = (x[c] * inv - (c == lab ? 1.f : 0.f)) * grad_scale;
      }
      if constexpr (WL) {
        if (!keep) v = 0.f;  // a zero gradient row
      }
      const uint16_t b = f2bf(v);
      out[c / 8][c % 8] = b;
      g[c] = bf2f(b);
    }
    u16x8* drow = reinterpret_cast<u16x8*>(dlogits + (size_t)r * ld);
#pragma unroll
    for (int v = 0; v < LD / 8; ++v) drow[v] = out[v];
  }
  // block-level reduction first: one atomic per statistic / bias column per BLOCK
  // (same-address fp32 atomics serialise in L2; per-wave atomics cost ~9 us here)
  __shared__ float part[4][LD + 2];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  loss = wave_sum(loss);
  correct = wave_sum(correct);
  if (lane == 0) {
    part[w][LD] = loss;
    part[w][LD + 1] = correct;
  }
  if (dbias) {
#pragma unroll
    for (int c = 0; c < LD; ++c) {
      const float t = wave_sum(g[c]);
      if (lane == 0) part[w][c] = t;
    }
  }
  __syncthreads();
  const int t = threadIdx.x;
  if (t < LD + 2 && (dbias || t >= LD)) {
    float v = part[0][t] + part[1][t] + part[2][t] + part[3][t];
    if constexpr (WL) {
      // straight into stats: this block's share of B * (weighted loss sum / den)
      if (t == LD && !fin.out) v *= grad_scale * (float)B;
    }
    atomicAdd(t < LD ? dbias + t : (fin.out ? fin.acc : stats) + (t - LD), v);
  }
  xent_finish<MODE>(fin, stats, wden, B);
}

template <int MODE>
hipError_t launch_xent(const uint16_t* logits, const int64_t* labels, uint16_t* dlogits, float* stats, float* dbias,
                       int B, int C, int ld, float grad_scale, hipStream_t s, const XentFin& fin, float conf,
                       float epsc, const float* q = nullptr, int ldq = 0, const float* wt = nullptr,
                       const float* wden = nullptr, int64_t ignore_index = -100) {
  // 16-B target loads in the rows kernel (XM_SOFT / XM_WSOFT only)
  const bool qvec = (ldq % 4 == 0) && (reinterpret_cast<uintptr_t>(q) & 15) == 0;
  const bool vec_ok = (ld % 8 == 0) && ((reinterpret_cast<uintptr_t>(logits) | reinterpret_cast<uintptr_t>(dlogits)) & 15) == 0;
  if (vec_ok && ld <= 64) {
    const int g = (B + 255) / 256;
    switch (ld) {
#define XENT_ROWS_CASE(L) \
      case L: xent_rows_kernel<L, MODE><<<g, 256, 0, s>>>(logits, labels, dlogits, stats, dbias, B, C, ld, grad_scale, fin, conf, epsc, q, ldq, qvec, wt, wden, ignore_index); break;
      XENT_ROWS_CASE(8) XENT_ROWS_CASE(16) XENT_ROWS_CASE(24) XENT_ROWS_CASE(32) XENT_ROWS_CASE(40) XENT_ROWS_CASE(48) XENT_ROWS_CASE(56)
#undef XENT_ROWS_CASE
      default: xent_rows_kernel<64, MODE><<<g, 256, 0, s>>>(logits, labels, dlogits, stats, dbias, B, C, ld, grad_scale, fin, conf, epsc, q, ldq, qvec, wt, wden, ignore_index); break;
    }
    return hipGetLastError();
  }
  // one row per wave while that still leaves < 256 blocks (a 64-row batch: 16 blocks
  // instead of 4 waves walking 16 rows each), 16 rows per block beyond
  const int rpb = B <= 4 * 256 ? 4 : kRowsPerBlock;
  const int g = (B + rpb - 1) / rpb;
  xent_kernel<MODE><<<g, 256, 0, s>>>(logits, labels, dlogits, stats, dbias, B, C, ld, grad_scale, rpb, fin, conf, epsc, q, ldq, wt, wden, ignore_index);
  return hipGetLastError();
}

}  // namespace

hipError_t softmax_xent(const uint16_t* logits, const int64_t* labels, uint16_t* dlogits, float* stats,
                        float* dbias, int B, int C, int ld, float grad_scale, hipStream_t s, const XentFin* finp,
                        float label_smoothing) {
  if (ld > kMaxColsPerLane * 64 || C > ld) return hipErrorInvalidValue;
  if (!(label_smoothing >= 0.f && label_smoothing <= 1.f)) return hipErrorInvalidValue;  // (NaN too)
  const XentFin fin = finp ? *finp : XentFin{};
  if (fin.out && (fin.acc == nullptr || fin.cnt == nullptr)) return hipErrorInvalidValue;
  if (!fin.out && stats == nullptr) return hipErrorInvalidValue;
  if (B <= 0) return hipSuccess;
  if (label_smoothing == 0.f)
    return launch_xent<XM_PLAIN>(logits, labels, dlogits, stats, dbias, B, C, ld, grad_scale, s, fin, 1.f, 0.f);
  return launch_xent<XM_SMOOTH>(logits, labels, dlogits, stats, dbias, B, C, ld, grad_scale, s, fin, 1.f - label_smoothing,
                           label_smoothing / (float)C);
}

hipError_t softmax_xent_soft(const uint16_t* logits, const float* q, int ldq, uint16_t* dlogits, float* stats,
                             float* dbias, int B, int C, int ld, float grad_scale, hipStream_t s, const XentFin* finp,
                             float label_smoothing) {
  if (ld > kMaxColsPerLane * 64 || C > ld || C < 1 || ldq < C || q == nullptr) return hipErrorInvalidValue;
  if (!(label_smoothing >= 0.f && label_smoothing <= 1.f)) return hipErrorInvalidValue;  // (NaN too)
  const XentFin fin = finp ? *finp : XentFin{};
  if (fin.out && (fin.acc == nullptr || fin.cnt == nullptr)) return hipErrorInvalidValue;
  if (!fin.out && stats == nullptr) return hipErrorInvalidValue;
  if (B <= 0) return hipSuccess;
  return launch_xent<XM_SOFT>(logits, nullptr, dlogits, stats, dbias, B, C, ld, grad_scale, s, fin,
                              1.f - label_smoothing, label_smoothing / (float)C, q, ldq);
}

hipError_t softmax_xent_w(const uint16_t* logits, const int64_t* labels, uint16_t* dlogits, float* stats,
                          float* dbias, int B, int C, int ld, const float* weight, int64_t ignore_index,
                          float* wden_ws, hipStream_t s, const XentFin* finp, float label_smoothing) {
  if (ld > kMaxColsPerLane * 64 || C > ld || C < 1 || wden_ws == nullptr) return hipErrorInvalidValue;
  if (!(label_smoothing >= 0.f && label_smoothing <= 1.f)) return hipErrorInvalidValue;  // (NaN too)
  const XentFin fin = finp ? *finp : XentFin{};
  if (fin.out && (fin.acc == nullptr || fin.cnt == nullptr)) return hipErrorInvalidValue;
  if (!fin.out && stats == nullptr) return hipErrorInvalidValue;
  if (B <= 0) return hipSuccess;
  xent_wden_kernel<<<1, 256, 0, s>>>(labels, weight, B, C, ignore_index, wden_ws);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_xent<XM_W>(logits, labels, dlogits, stats, dbias, B, C, ld, 0.f, s, fin, 1.f - label_smoothing,
                           label_smoothing / (float)C, nullptr, 0, weight, wden_ws, ignore_index);
}

hipError_t softmax_xent_focal(const uint16_t* logits, const int64_t* labels, uint16_t* dlogits, float* stats,
                              float* dbias, int B, int C, int ld, const float* weight, int64_t ignore_index,
                              float* wden_ws, float gamma, hipStream_t s, const XentFin* finp) {
  if (!(gamma >= 0.f && gamma <= 3.402823466e+38f)) return hipErrorInvalidValue;  // negative, NaN, inf
  if (gamma == 0.f)  // the weighted cross-entropy itself: the focal instances never see 0
    return softmax_xent_w(logits, labels, dlogits, stats, dbias, B, C, ld, weight, ignore_index, wden_ws, s, finp, 0.f);
  if (ld > kMaxColsPerLane * 64 || C > ld || C < 1 || wden_ws == nullptr) return hipErrorInvalidValue;
  const XentFin fin = finp ? *finp : XentFin{};
  if (fin.out && (fin.acc == nullptr || fin.cnt == nullptr)) return hipErrorInvalidValue;
  if (!fin.out && stats == nullptr) return hipErrorInvalidValue;
  if (B <= 0) return hipSuccess;
  xent_wden_kernel<<<1, 256, 0, s>>>(labels, weight, B, C, ignore_index, wden_ws);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  // gamma rides in `conf`; epsc and the host's grad_scale are unused under this mode
  return launch_xent<XM_FOCAL>(logits, labels, dlogits, stats, dbias, B, C, ld, 0.f, s, fin, gamma, 0.f, nullptr, 0,
                               weight, wden_ws, ignore_index);
}

hipError_t softmax_xent_soft_w(const uint16_t* logits, const float* q, int ldq, uint16_t* dlogits, float* stats,
                               float* dbias, int B, int C, int ld, float grad_scale, const float* weight,
                               hipStream_t s, const XentFin* finp, float label_smoothing) {
  if (ld > kMaxColsPerLane * 64 || C > ld || C < 1 || ldq < C || q == nullptr) return hipErrorInvalidValue;
  if (!(label_smoothing >= 0.f && label_smoothing <= 1.f)) return hipErrorInvalidValue;  // (NaN too)
  const XentFin fin = finp ? *finp : XentFin{};
  if (fin.out && (fin.acc == nullptr || fin.cnt == nullptr)) return hipErrorInvalidValue;
  if (!fin.out && stats == nullptr) return hipErrorInvalidValue;
  if (B <= 0) return hipSuccess;
  return launch_xent<XM_WSOFT>(logits, nullptr, dlogits, stats, dbias, B, C, ld, grad_scale, s, fin,
                               1.f - label_smoothing, label_smoothing / (float)C, q, ldq, weight);
}

hipError_t scale_bf16_dev(const uint16_t* src, const float* scale, uint16_t* out, int64_t n, hipStream_t s) {
  if (n % 8 || ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out)) & 15)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const int64_t n8 = n / 8;
  const int g = (int)std::min<int64_t>((n8 + 255) / 256, 1024);
  scale_bf16_kernel<<<g, 256, 0, s>>>(src, scale, out, n8);
  return hipGetLastError();
}

}  // namespace ldnn
