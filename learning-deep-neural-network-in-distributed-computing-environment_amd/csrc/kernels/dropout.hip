// Dropout with counter-hashed masks: no mask is stored, the backward regenerates it.
//
// Mask definition (the NumPy twin ops/functional.py dropout_mask states the same and must
// agree bit for bit).  A tensor is seen as [R, N]: N the last logical dimension, R the product
// of the rest.  Four neighbouring columns of a row share one hash; with G = ceil(N / 4):
//
//   key   = smix(smix(seed64) ^ (module_index << 32 | counter))      all 64-bit, wrapping
//   h     = smix(key ^ ((r * G + (c >> 2)) * 0xD1B54A32D192ED03))
//   bits  = (h >> (16 * (c & 3))) & 0xFFFF
//   drop  = bits < thr        with thr = round(p * 65536), 0 <= thr <= 65536
//   scale = 65536.0f / (65536 - thr)   (fp32; thr == 65536: everything is dropped, output 0)
//   y     = drop ? 0 : bf16_rne(float(x) * scale)        dx = drop ? 0 : bf16_rne(float(g) * scale)
//
// smix is the splitmix64 finaliser of augment.hip / data/autoaugment.smix.  The realised rate is
// thr / 65536 and the scale is that rate's.  The mask depends on the logical (r, c) only: not on
// the row stride, the padding or the grid.
//
// Device state of one Dropout module, 8 x 32-bit words (host-written like the optimizers' lr):
//   [0] seed low  [1] seed high  [2] module_index  [3] counter  [4] thr  [5] scale (fp32 bits,
//   0 when thr == 65536)  [6] arrival count  [7] unused
// Ticket of one forward call, 8 x 32-bit words, saved by the autograd node:
//   [0] key low  [1] key high  [2] thr  [3] scale bits  [4] the counter the launch used
//
// dropout_fwd reads the state, one thread writes the ticket, and the last workgroup to arrive
// stores counter + 1 and clears the arrival count (the "last block" idiom of xent.hip's
// xent_finish): every replay of a captured step draws a new mask with no host write and no
// extra launch.  Every workgroup has used the counter it loaded (the key feeds its stores) before
// it joins the barrier in front of its arrival, so the last arrival's store cannot overtake a
// read.  dropout_bwd reads the ticket, never the live state: the forward may have run again, or
// the host may have reseeded, since.
//
// Both are one streaming pass at 4 B per element.  Vector path (ld_in % 8 == 0, ld_out % 8 == 0,
// 16-B aligned bases): a thread owns 8 columns of a row, one 16-B load, two hashes, one 16-B
// store; a row's vectors cover the whole padded output row, and columns N <= c < ld_out are
// written as zeros whatever the input held there.  Every other layout: a thread owns one 4-column
// group (one hash) with 2-B accesses.  A thread walks (row, vector) pairs with a grid stride whose
// quotient and remainder by the row length come from the host: no division in the loop; rows,
// groups and element offsets are 64-bit.  Grid as act_fwd's: 256 threads, at most 2048 workgroups.
#include "ldnn_common.h"
#include "ldnn_kernels.h"

namespace ldnn {
namespace {

constexpr int kBlock = 256;
constexpr uint64_t kGroupMul = 0xD1B54A32D192ED03ull;

__device__ __forceinline__ uint64_t smix64(uint64_t z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

__device__ __forceinline__ uint32_t ld_word(const uint32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_word(uint32_t* p, uint32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__device__ __forceinline__ uint16_t drop1(uint16_t x, uint32_t bits, uint32_t thr, float scale) {
  return bits < thr ? (uint16_t)0 : f2bf(bf2f(x) * scale);
}

struct DropGeo {
  int64_t R, N, ld_in, ld_out;
  int64_t G;        // hash groups per logical row, ceil(N / 4)
  int64_t per_row;  // work items per row: ld_out / 8 (vector path), ceil(ld_out / 4) (scalar)
  int64_t step_r, step_c;  // (gridDim.x * kBlock) / per_row and % per_row
};

// FWD: state -> key, ticket, arrival.  !FWD: ticket -> key.
template <bool FWD, bool VEC>
__global__ __launch_bounds__(kBlock) void dropout_kernel(const bf16_t* __restrict__ x, bf16_t* __restrict__ y,
                                                          uint32_t* state, uint32_t* ticket, DropGeo g) {
  uint64_t key;
  uint32_t thr, counter = 0;
  float scale;
  if constexpr (FWD) {
    const uint64_t seed = (uint64_t)ld_word(state + 0) | ((uint64_t)ld_word(state + 1) << 32);
    const uint32_t module = ld_word(state + 2);
    counter = ld_word(state + 3);
    thr = ld_word(state + 4);
    const uint32_t sb = ld_word(state + 5);
    scale = __uint_as_float(sb);
    key = smix64(smix64(seed) ^ (((uint64_t)module << 32) | (uint64_t)counter));
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      ticket[0] = (uint32_t)key;
      ticket[1] = (uint32_t)(key >> 32);
      ticket[2] = thr;
      ticket[3] = sb;
      ticket[4] = counter;
    }
  } else {
    key = (uint64_t)ticket[0] | ((uint64_t)ticket[1] << 32);
    thr = ticket[2];
    scale = __uint_as_float(ticket[3]);
  }

  const int64_t first = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  int64_t r = first / g.per_row, v = first - r * g.per_row;
  for (; r < g.R; r += g.step_r) {
    if constexpr (VEC) {
      const int64_t c0 = v * 8;
      u16x8 o = {0, 0, 0, 0, 0, 0, 0, 0};
      if (c0 < g.N) {
        const u16x8 in = *reinterpret_cast<const u16x8*>(x + r * g.ld_in + c0);
        const uint64_t grp = (uint64_t)(r * g.G + (c0 >> 2));
        const uint64_t h0 = smix64(key ^ (grp * kGroupMul));
        const uint64_t h1 = smix64(key ^ ((grp + 1) * kGroupMul));
        if (c0 + 8 <= g.N) {
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            o[j] = drop1(in[j], (uint32_t)(h0 >> (16 * j)) & 0xFFFFu, thr, scale);
            o[4 + j] = drop1(in[4 + j], (uint32_t)(h1 >> (16 * j)) & 0xFFFFu, thr, scale);
          }
        } else {  // the row's last, partial vector: columns >= N stay 0
          const int n = (int)(g.N - c0);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (j < n) o[j] = drop1(in[j], (uint32_t)(h0 >> (16 * j)) & 0xFFFFu, thr, scale);
            if (4 + j < n) o[4 + j] = drop1(in[4 + j], (uint32_t)(h1 >> (16 * j)) & 0xFFFFu, thr, scale);
          }
        }
      }
      *reinterpret_cast<u16x8*>(y + r * g.ld_out + c0) = o;
    } else {
      const int64_t c0 = v * 4;
      const uint64_t h = c0 < g.N ? smix64(key ^ ((uint64_t)(r * g.G + v) * kGroupMul)) : 0ull;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int64_t c = c0 + j;
        if (c < g.N) y[r * g.ld_out + c] = drop1(x[r * g.ld_in + c], (uint32_t)(h >> (16 * j)) & 0xFFFFu, thr, scale);
        else if (c < g.ld_out) y[r * g.ld_out + c] = 0;
      }
    }
    v += g.step_c;
    if (v >= g.per_row) {
      v -= g.per_row;
      ++r;
    }
  }

  if constexpr (FWD) {
    // last workgroup to arrive: next call's counter, arrival count back to 0
    __syncthreads();
    if (threadIdx.x == 0) {
      __threadfence();
      if (atomicAdd(state + 6, 1u) == gridDim.x - 1) {
        st_word(state + 3, counter + 1u);
        atomicExch(state + 6, 0u);
      }
    }
  }
}

template <bool FWD>
hipError_t launch_dropout(const uint16_t* x, uint16_t* y, uint32_t* state, uint32_t* ticket, int64_t R, int64_t N,
                          int64_t ld_in, int64_t ld_out, hipStream_t s) {
  if (x == nullptr || y == nullptr || ticket == nullptr || (FWD && state == nullptr)) return hipErrorInvalidValue;
  if (R < 0 || N < 1 || N > ld_in || N > ld_out) return hipErrorInvalidValue;
  if (((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 1) ||
      ((reinterpret_cast<uintptr_t>(state) | reinterpret_cast<uintptr_t>(ticket)) & 3))
    return hipErrorInvalidValue;
  if (R == 0) return hipSuccess;
  const bool vec = ld_in % 8 == 0 && ld_out % 8 == 0 &&
                   ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(y)) & 15) == 0;
  DropGeo g;
  g.R = R, g.N = N, g.ld_in = ld_in, g.ld_out = ld_out;
  g.G = (N + 3) / 4;
  g.per_row = vec ? ld_out / 8 : (ld_out + 3) / 4;
  if (R > INT64_MAX / g.per_row / 16) return hipErrorInvalidValue;  // (item and element offsets stay in int64)
  const int64_t items = R * g.per_row;
  int64_t grid = (items + kBlock - 1) / kBlock;
  if (grid > 2048) grid = 2048;
  const int64_t stride = grid * kBlock;
  g.step_r = stride / g.per_row;
  g.step_c = stride % g.per_row;
  if (vec) dropout_kernel<FWD, true><<<(int)grid, kBlock, 0, s>>>(x, y, state, ticket, g);
  else dropout_kernel<FWD, false><<<(int)grid, kBlock, 0, s>>>(x, y, state, ticket, g);
  return hipGetLastError();
}

}  // namespace

hipError_t dropout_fwd(const uint16_t* x, uint16_t* y, uint32_t* state, uint32_t* ticket, int64_t R, int64_t N,
                       int64_t ld_in, int64_t ld_out, hipStream_t s) {
  return launch_dropout<true>(x, y, state, ticket, R, N, ld_in, ld_out, s);
}

hipError_t dropout_bwd(const uint16_t* g, uint16_t* dx, const uint32_t* ticket, int64_t R, int64_t N, int64_t ld_in,
                       int64_t ld_out, hipStream_t s) {
  return launch_dropout<false>(g, dx, nullptr, const_cast<uint32_t*>(ticket), R, N, ld_in, ld_out, s);
}

}  // namespace ldnn
