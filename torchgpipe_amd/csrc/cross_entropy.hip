// Softmax cross-entropy loss over fp32 logit rows x[R][V] with int64 class indices t[R], forward
// and backward, for gfx950 (ops/loss.py).  ignore_index, label smoothing eps in [0, 1) and the
// reductions none / mean / sum:
//   lse_r  = log sum_v exp(x_rv)
//   loss_r = (1 - eps) (lse_r - x_{r,t_r}) + eps (lse_r - mean_v x_rv)      (0 for an ignored row)
//   dx_rv  = s_r (exp(x_rv - lse_r) - (1 - eps) [v = t_r] - eps / V)        (0 for an ignored row)
// with s_r the upstream gradient (times 1 / count for `mean`).  The log-softmax is never
// written: the forward reads the logits once and keeps two floats per row, stat[R][2] =
// (m_r, 1 / sum_v exp(x_rv - m_r)) with m_r the row's maximum; the backward reads the logits
// once more and writes dx.  The pair, not lse_r = m_r + log sum_v exp(x_rv - m_r) in one float:
// logits with a large common offset put lse_r where an fp32 ulp is 4e-6, and
// exp(x_rv - lse_r) would carry that as a relative error, while exp(x_rv - m_r) over the sum
// is good to a few ulp at any offset.  The loss is formed the same way, as
// log sum_v exp(x_rv - m_r) - (x_{r,t_r} - m_r).
//
// Forward.  A row is owned by a *group* of L lanes, as in layernorm.hip:
//   * narrow instance: L = 64, a wave per row, four rows per 256-thread workgroup, no LDS and
//     no barrier on the row path;
//   * wide instance:   L = 256, a workgroup per row; the four waves combine through LDS in
//     wave order.
// The group streams the row in batches of 4 Q L columns (Q 16-byte loads per lane, all issued
// before the first use, and the next batch's issued before this batch's arithmetic).  A lane
// keeps a running (max, sum exp(x - max)) pair, rescaled once per batch when the max moves, and
// with smoothing a running sum x.  exp(-inf - -inf) never happens: wherever a max can still be
// -inf the exponent is taken against 0 instead, which gives the same 0.  Lanes merge their
// pairs in a fixed __shfl_xor butterfly.  x_{r,t} is one more load through the row's resource,
// at offset 0 unless 0 <= t < V.
//
// Every access to the logits and to dx goes through a raw buffer resource that spans exactly
// one row (V * 4 bytes) on a base computed in 64 bits, so only a row has to stay below 2 GiB;
// columns past V read 0 (and are masked to -inf in the forward) and their stores are dropped.
//   * float4 path (V % 4 == 0, bases 16-byte aligned): quad j of a batch is columns
//     4 (lane + L j) .. + 3;
//   * dword path: element i is column lane + L i.
//
// Reduce (sum / mean): one workgroup adds loss_rows[R] in a fixed order in fp64, counts the
// rows that are not ignored, and writes the scalar and inv_count (1 / count for mean, else 1),
// which the backward reads from the device.
//
// Backward.  Narrow: a wave per row.  Wide: a workgroup per (row, chunk of 4 Q 256 columns), so
// the row's pair, t_r and s_r are loaded once per workgroup; the workgroup of an ignored row
// stores zeros and reads no logits.  The one-hot term is applied by the one lane whose
// registers hold column t_r.  No atomics anywhere: the same inputs give the same bits.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <atomic>
#include <limits>
#include <type_traits>

#include "kernels.h"

namespace tgpipe {

namespace {

typedef uint32_t uintx4 __attribute__((ext_vector_type(4)));

constexpr int kThreads = 256;  // forward and backward
constexpr int kReduceThreads = 1024;
// The switch-over: rows up to this width take the narrow instance (measured, see
// profiles/r21/cross_entropy/README.md).
constexpr int kWaveRowMax = 4096;
constexpr int kNarrowQ = 4;  // 16-byte loads per lane and batch: 1024 columns per wave and batch
constexpr int kWideQ = 8;    // forward: 8192 columns per workgroup and batch
// Backward, wide: registers per lane / 4 = columns per chunk / 1024, for the float4 and for the
// dword path (measured, same place).
constexpr int kBackwardQ = 8, kBackwardDwordQ = 4;

std::atomic<int> forced_wide{-1};
std::atomic<int> forced_chunk_q{0};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const float* p, int n) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), static_cast<short>(0), n * 4,
                                           0x00020000);
}

// The group's registers <- the batch of 4 Q L columns from column c0 (columns past the
// resource's end read 0).
template <int Q, bool VEC, int L>
__device__ __forceinline__ void load_batch(float (&v)[4 * Q], __amdgpu_buffer_rsrc_t r,
                                           uint32_t c0, int t) {
  if constexpr (VEC) {
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const auto q = __builtin_amdgcn_raw_buffer_load_b128(r, 4u * c0 + 16u * (t + L * j), 0, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * j + e] = __uint_as_float(q[e]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4 * Q; ++i)
      v[i] = __uint_as_float(
          __builtin_amdgcn_raw_buffer_load_b32(r, 4u * (c0 + t + L * i), 0, 0));
  }
}

// the batch <- the group's registers (columns past the resource's end are dropped).
template <int Q, bool VEC, int L>
__device__ __forceinline__ void store_batch(const float (&v)[4 * Q], __amdgpu_buffer_rsrc_t r,
                                            uint32_t c0, int t) {
  if constexpr (VEC) {
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const uintx4 q{__float_as_uint(v[4 * j]), __float_as_uint(v[4 * j + 1]),
                     __float_as_uint(v[4 * j + 2]), __float_as_uint(v[4 * j + 3])};
      __builtin_amdgcn_raw_buffer_store_b128(q, r, 4u * c0 + 16u * (t + L * j), 0, 0);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4 * Q; ++i)
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[i]), r, 4u * (c0 + t + L * i), 0,
                                            0);
  }
}

// the column, counted from the batch's first, of register i of lane t (float4 path: V % 4 == 0,
// so a quad is inside the row or outside it as a whole)
template <bool VEC, int L>
__device__ __forceinline__ int column(int i, int t) {
  return VEC ? 4 * (t + L * (i >> 2)) : t + L * i;
}

constexpr float kNegInf = -std::numeric_limits<float>::infinity();

// what exponents are taken against: the max, or 0 while nothing finite has been seen
__device__ __forceinline__ float pivot(float m) { return m == kNegInf ? 0.f : m; }

// (m, s) <- (m, s) merged with (m2, s2): s = sum exp(x - m) over both parts
__device__ __forceinline__ void merge(float& m, float& s, float m2, float s2) {
  const float mx = fmaxf(m, m2), p = pivot(mx);
  s = s * expf(m - p) + s2 * expf(m2 - p);
  m = mx;
}

template <bool VEC, bool WIDE, bool SMOOTH>
__global__ __launch_bounds__(kThreads) void cross_entropy_forward_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ target, float* __restrict__ stat,
    float* __restrict__ loss_rows, int R, int V, int64_t ignore_index, float eps) {
  constexpr int L = WIDE ? kThreads : 64, Q = WIDE ? kWideQ : kNarrowQ, E = 4 * Q;
  constexpr int kBatch = L * E;
  __shared__ float red[3][4];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int t = WIDE ? threadIdx.x : threadIdx.x & 63;
  const int row = WIDE ? blockIdx.x : blockIdx.x * 4 + wave;
  if (row >= R) return;  // narrow tail waves only: no barrier on their path

  const __amdgpu_buffer_rsrc_t r = row_rsrc(x + static_cast<int64_t>(row) * V, V);
  float m = kNegInf, s = 0.f, sx = 0.f;
  float next[E];
  load_batch<Q, VEC, L>(next, r, 0, t);
  for (int c0 = 0; c0 < V; c0 += kBatch) {
    float v[E];
#pragma unroll
    for (int i = 0; i < E; ++i) v[i] = next[i];
    if (c0 + kBatch < V) load_batch<Q, VEC, L>(next, r, c0 + kBatch, t);
    if constexpr (SMOOTH) {
#pragma unroll
      for (int i = 0; i < E; ++i) sx += v[i];  // columns past V read 0
    }
    float bm = kNegInf;
#pragma unroll
    for (int i = 0; i < E; ++i) {
      if (c0 + column<VEC, L>(i, t) >= V) v[i] = kNegInf;
      bm = fmaxf(bm, v[i]);
    }
    const float mx = fmaxf(m, bm), p = pivot(mx);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < E; ++i) acc += expf(v[i] - p);
    s = s * expf(m - p) + acc;
    m = mx;
  }

#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    merge(m, s, __shfl_xor(m, off), __shfl_xor(s, off));
    if constexpr (SMOOTH) sx += __shfl_xor(sx, off);
  }
  if constexpr (WIDE) {
    if ((threadIdx.x & 63) == 0) {
      red[0][wave] = m;
      red[1][wave] = s;
      red[2][wave] = sx;
    }
    __syncthreads();
    m = red[0][0];
    s = red[1][0];
    sx = red[2][0];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      merge(m, s, red[0][w], red[1][w]);
      sx += red[2][w];
    }
  }
  if (t != 0) return;

  const int64_t tg = target[row];
  const bool inside = tg >= 0 && tg < V;
  // inside the row whatever the target: offset 0 stands in, and its value is not used
  const float xt = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(
      r, inside ? 4u * static_cast<uint32_t>(tg) : 0u, 0, 0));
  // against the row maximum: differences of logits, not logits, meet log s
  const float ls = logf(s);
  float loss = ls - ((inside ? xt : std::numeric_limits<float>::quiet_NaN()) - m);
  if constexpr (SMOOTH)
    loss = (1.f - eps) * loss + eps * (ls - (sx / static_cast<float>(V) - m));
  stat[2 * static_cast<int64_t>(row)] = m;
  stat[2 * static_cast<int64_t>(row) + 1] = 1.f / s;
  loss_rows[row] = tg == ignore_index ? 0.f : loss;
}

// Sum over the block in a fixed order; the result is valid on thread 0.
__device__ __forceinline__ double block_sum(double v, double* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  double total = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < kReduceThreads / 64; ++w) total += lds[w];
  }
  return total;
}

// loss[0] = sum_r loss_rows[r] (/ count for mean), inv_count[0] = 1 / count for mean, else 1;
// count = rows whose target is not ignore_index.  loss == nullptr (`none`): inv_count only.
__global__ __launch_bounds__(kReduceThreads) void cross_entropy_reduce_kernel(
    const float* __restrict__ loss_rows, const int64_t* __restrict__ target, int R,
    int64_t ignore_index, bool mean, float* __restrict__ loss, float* __restrict__ inv_count) {
  __shared__ double lds[2][kReduceThreads / 64];
  if (loss == nullptr) {
    if (threadIdx.x == 0) inv_count[0] = 1.f;
    return;
  }
  double acc = 0.0, rows = 0.0;
  for (int r = threadIdx.x; r < R; r += kReduceThreads) {
    acc += static_cast<double>(loss_rows[r]);
    rows += target[r] != ignore_index ? 1.0 : 0.0;
  }
  const double total = block_sum(acc, lds[0]);
  const double count = block_sum(rows, lds[1]);
  if (threadIdx.x != 0) return;
  loss[0] = static_cast<float>(mean ? total / count : total);  // no rows: 0 / 0
  inv_count[0] = mean ? static_cast<float>(1.0 / count) : 1.f;
}

// grad: [R] with per_row (`none`), else one element that inv_count[0] multiplies.
template <int Q, bool VEC, bool WIDE>
__global__ __launch_bounds__(kThreads) void cross_entropy_backward_kernel(
    const float* __restrict__ grad, const float* __restrict__ inv_count,
    const float* __restrict__ x, const int64_t* __restrict__ target,
    const float* __restrict__ stat, float* __restrict__ dx, int R, int V, int chunks,
    int64_t ignore_index, float eps, bool per_row) {
  constexpr int L = WIDE ? kThreads : 64, E = 4 * Q;
  constexpr int kBatch = L * E;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int t = WIDE ? threadIdx.x : threadIdx.x & 63;
  const int block = static_cast<int>(blockIdx.x);
  const int row = WIDE ? block / chunks : block * 4 + wave;
  if (row >= R) return;
  // wide: the workgroup's one chunk; narrow: the whole row
  const int begin = WIDE ? (block - row * chunks) * kBatch : 0;
  const int end = WIDE ? min(V, begin + kBatch) : V;
  const __amdgpu_buffer_rsrc_t out = row_rsrc(dx + static_cast<int64_t>(row) * V, V);
  const int64_t tg = target[row];
  float v[E];
  if (tg == ignore_index) {
#pragma unroll
    for (int i = 0; i < E; ++i) v[i] = 0.f;
    for (int c0 = begin; c0 < end; c0 += kBatch) store_batch<Q, VEC, L>(v, out, c0, t);
    return;
  }
  const __amdgpu_buffer_rsrc_t in = row_rsrc(x + static_cast<int64_t>(row) * V, V);
  const float m = stat[2 * static_cast<int64_t>(row)];
  const float s = per_row ? grad[row] : grad[0] * inv_count[0];
  const float scale = s * stat[2 * static_cast<int64_t>(row) + 1];  // s_r / sum_v exp(x_rv - m_r)
  const float hot = (1.f - eps) * s, flat = s * eps / static_cast<float>(V);
  const int tcol = tg >= 0 && tg < V ? static_cast<int>(tg) : -1;  // -1: in no batch
  for (int c0 = begin; c0 < end; c0 += kBatch) {
    load_batch<Q, VEC, L>(v, in, c0, t);
#pragma unroll
    for (int i = 0; i < E; ++i) v[i] = fmaf(scale, expf(v[i] - m), -flat);
    // the register of the lane that holds column t_r
    const int rel = tcol - c0;
    const int unit = VEC ? rel >> 2 : rel;  // quad or element within the batch
    if (rel >= 0 && rel < kBatch && (unit & (L - 1)) == t) {
      const int reg = VEC ? 4 * (unit / L) + (rel & 3) : unit / L;
#pragma unroll
      for (int i = 0; i < E; ++i)
        if (i == reg) v[i] -= hot;
    }
    store_batch<Q, VEC, L>(v, out, c0, t);
  }
}

bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

bool use_wide(int V) {
  const int f = forced_wide.load();
  return f == 0 ? false : f == 1 ? true : V > kWaveRowMax;
}

int backward_q(bool vec) {
  const int q = forced_chunk_q.load();
  return q > 0 ? q : vec ? kBackwardQ : kBackwardDwordQ;
}

}  // namespace

void cross_entropy_force_instance(int wide, int chunk_cols) {
  forced_wide.store(wide == 0 || wide == 1 ? wide : -1);
  const int q = chunk_cols / (4 * kThreads);  // 4096 or 8192 columns; anything else: the default
  forced_chunk_q.store(chunk_cols % (4 * kThreads) == 0 && (q == 4 || q == 8) ? q : 0);
}

int cross_entropy_wave_row_max() { return kWaveRowMax; }

int cross_entropy_backward_chunk(bool vec) { return backward_q(vec) * 4 * kThreads; }

void launch_cross_entropy_forward(const float* x, const int64_t* target, float* stat,
                                  float* loss_rows, float* loss, float* inv_count, int R, int V,
                                  int64_t ignore_index, float eps, bool mean,
                                  hipStream_t stream) {
  const bool vec = V % 4 == 0 && aligned16(x);
  const bool wide = use_wide(V);
  const dim3 grid(wide ? R : (R + 3) / 4), block(kThreads);
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, x, target, stat, loss_rows, R, V,
                       ignore_index, eps);
  };
  auto smooth = [&](auto vec_c, auto wide_c) {
    constexpr bool VEC = decltype(vec_c)::value, WIDE = decltype(wide_c)::value;
    if (eps > 0.f) go(cross_entropy_forward_kernel<VEC, WIDE, true>);
    else go(cross_entropy_forward_kernel<VEC, WIDE, false>);
  };
  if (vec && wide) smooth(std::true_type{}, std::true_type{});
  else if (vec) smooth(std::true_type{}, std::false_type{});
  else if (wide) smooth(std::false_type{}, std::true_type{});
  else smooth(std::false_type{}, std::false_type{});
  hipLaunchKernelGGL(cross_entropy_reduce_kernel, dim3(1), dim3(kReduceThreads), 0, stream,
                     static_cast<const float*>(loss_rows), target, R, ignore_index, mean, loss,
                     inv_count);
}

void launch_cross_entropy_backward(const float* grad, const float* inv_count, const float* x,
                                   const int64_t* target, const float* stat, float* dx, int R,
                                   int V, int64_t ignore_index, float eps, bool per_row,
                                   hipStream_t stream) {
  const bool vec = V % 4 == 0 && aligned16(x) && aligned16(dx);
  const bool wide = use_wide(V);
  const int q = wide ? backward_q(vec) : kNarrowQ;
  const int chunks = wide ? (V + q * 4 * kThreads - 1) / (q * 4 * kThreads) : 1;
  const dim3 grid(wide ? R * chunks : (R + 3) / 4), block(kThreads);
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, grad, inv_count, x, target, stat, dx, R, V,
                       chunks, ignore_index, eps, per_row);
  };
  if (!wide) {
    if (vec) go(cross_entropy_backward_kernel<kNarrowQ, true, false>);
    else go(cross_entropy_backward_kernel<kNarrowQ, false, false>);
  } else if (q == 4) {
    if (vec) go(cross_entropy_backward_kernel<4, true, true>);
    else go(cross_entropy_backward_kernel<4, false, true>);
  } else {
    if (vec) go(cross_entropy_backward_kernel<8, true, true>);
    else go(cross_entropy_backward_kernel<8, false, true>);
  }
}

}  // namespace tgpipe
