// LayerNorm / RMSNorm over the last dimension of fp32 rows x[R][N], 1 <= N <= 8192, forward
// and backward, for gfx950.  RMS is a template parameter: the same kernels without the mean
// and without beta.
//
// A row is owned by a *group* of L lanes and lives in the group's registers between its one
// global read and its one global write:
//   * narrow instance: L = 64, a wave per row, four rows per 256-thread workgroup, no LDS and
//     no barrier on the row path;
//   * wide instance:   L = 256, a workgroup per row; the four waves combine their sums
//     through LDS in wave order.
// Lane t of the group holds E = 4 Q values (Q = ceil(N / 4L) rounded up to an instance):
//   * float4 path (N % 4 == 0, every base 16-byte aligned): quad j is columns
//     4 (t + L j) .. + 3, one 16-byte access;
//   * dword path: element i is column t + L i.
// Every access goes through a raw buffer resource that spans exactly the row (N * 4 bytes),
// so columns past N read 0 and their stores are dropped by the range check -- no tail code,
// and all of a row's loads are issued back to back before the first use.
//
// Statistics are two-pass on the registers: mean = sum(x) / N, then sum((x - mean)^2) with
// the columns past N masked to 0.  Cross-lane sums are a fixed __shfl_xor butterfly.
//
// Backward: one persistent pass over dy and x.  Group g walks rows g, g + groups, ...; per
// row it recomputes xhat from the saved mean / rstd, forms g = dy * weight, the row sums
// sum(g) and sum(g * xhat), and writes dx = rstd (g - sum(g)/N - xhat sum(g xhat)/N).  A lane
// owns the same columns in every row it visits and keeps their sum(dy * xhat) and sum(dy) in
// registers for the whole walk; at the end the narrow instance adds its four waves' partials
// in wave order through LDS (the wide one has nothing to combine: its threads own disjoint
// columns) and the workgroup stores one [planes][N] partial.  layernorm_reduce_kernel then
// sums the workgroups' partials -- eight contiguous segments of the workgroup index, each in
// index order, then the eight in order -- and stores the result or adds it into an existing
// gradient.  No atomics anywhere: the same inputs give the same bits.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <atomic>
#include <type_traits>

#include "kernels.h"

namespace tgpipe {

namespace {

typedef uint32_t uintx4 __attribute__((ext_vector_type(4)));

constexpr int kCUs = 256;       // MI355X
constexpr int kThreads = 256;   // every kernel here
constexpr int kWaveRowCap = 2048;  // widest row the narrow instance has registers for (Q = 8)
// The switch-over: rows up to this width take the narrow instance (measured, see
// profiles/r20/layernorm/README.md).
constexpr int kWaveRowMax = 1024;
// Persistent backward: workgroups per CU (narrow: 16 waves per CU, wide: 8)
constexpr int kNarrowPerCU = 4, kWidePerCU = 2;
constexpr int kSegments = 8, kReduceCols = 32;  // layernorm_reduce_kernel's block

std::atomic<int> forced_wide{-1};

__device__ __forceinline__ __amdgpu_buffer_rsrc_t row_rsrc(const float* p, int n) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(p), static_cast<short>(0), n * 4,
                                           0x00020000);
}

// The group's registers <- row (columns past the resource's end read 0).
template <int Q, bool VEC, int L>
__device__ __forceinline__ void load_row(float (&v)[4 * Q], __amdgpu_buffer_rsrc_t r, int t) {
  if constexpr (VEC) {
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const auto q = __builtin_amdgcn_raw_buffer_load_b128(r, 16u * (t + L * j), 0, 0);
#pragma unroll
      for (int e = 0; e < 4; ++e) v[4 * j + e] = __uint_as_float(q[e]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4 * Q; ++i)
      v[i] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(r, 4u * (t + L * i), 0, 0));
  }
}

// row <- the group's registers (columns past the resource's end are dropped).
template <int Q, bool VEC, int L>
__device__ __forceinline__ void store_row(const float (&v)[4 * Q], __amdgpu_buffer_rsrc_t r,
                                          int t) {
  if constexpr (VEC) {
#pragma unroll
    for (int j = 0; j < Q; ++j) {
      const uintx4 q{__float_as_uint(v[4 * j]), __float_as_uint(v[4 * j + 1]),
                     __float_as_uint(v[4 * j + 2]), __float_as_uint(v[4 * j + 3])};
      __builtin_amdgcn_raw_buffer_store_b128(q, r, 16u * (t + L * j), 0, 0);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4 * Q; ++i)
      __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v[i]), r, 4u * (t + L * i), 0, 0);
  }
}

// the column of register i of lane t
template <bool VEC, int L>
__device__ __forceinline__ int column(int i, int t) {
  return VEC ? 4 * (t + L * (i >> 2)) + (i & 3) : t + L * i;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
  return v;
}

// Sum over the group.  WIDE: `slot` holds one float per wave; the caller never reuses a slot
// before another barrier has passed.
template <bool WIDE>
__device__ __forceinline__ float group_sum(float v, float* slot, int wave) {
  v = wave_sum(v);
  if constexpr (WIDE) {
    if ((threadIdx.x & 63) == 0) slot[wave] = v;
    __syncthreads();
    v = ((slot[0] + slot[1]) + slot[2]) + slot[3];
  }
  return v;
}

template <int Q, bool VEC, bool WIDE, bool RMS>
__global__ __launch_bounds__(kThreads) void layernorm_forward_kernel(
    const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
    float* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd, int R, int N,
    float eps) {
  constexpr int L = WIDE ? kThreads : 64, E = 4 * Q;
  __shared__ float red[2][4];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int t = WIDE ? threadIdx.x : threadIdx.x & 63;
  const int row = WIDE ? blockIdx.x : blockIdx.x * 4 + wave;
  if (row >= R) return;  // narrow tail waves only: no barrier on their path

  float v[E], gw[E], gb[E];
  load_row<Q, VEC, L>(v, row_rsrc(x + static_cast<int64_t>(row) * N, N), t);
  if (w != nullptr) load_row<Q, VEC, L>(gw, row_rsrc(w, N), t);
  if (b != nullptr) load_row<Q, VEC, L>(gb, row_rsrc(b, N), t);

  const float n = static_cast<float>(N);
  float m = 0.f;
  if constexpr (!RMS) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < E; ++i) s += v[i];
    m = group_sum<WIDE>(s, red[0], wave) / n;
#pragma unroll
    for (int i = 0; i < E; ++i) v[i] = column<VEC, L>(i, t) < N ? v[i] - m : 0.f;
  }
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < E; ++i) q += v[i] * v[i];
  const float rs = 1.f / sqrtf(group_sum<WIDE>(q, red[1], wave) / n + eps);
#pragma unroll
  for (int i = 0; i < E; ++i) {
    v[i] *= rs;
    if (w != nullptr) v[i] *= gw[i];
    if (b != nullptr) v[i] += gb[i];
  }
  store_row<Q, VEC, L>(v, row_rsrc(y + static_cast<int64_t>(row) * N, N), t);
  if (t == 0) {
    if constexpr (!RMS) mean[row] = m;
    rstd[row] = rs;
  }
}

// PART: keep and write the affine-gradient partials, part[workgroup][RMS ? 1 : 2][N]
// (plane 0 sum(dy * xhat), plane 1 sum(dy)).  dx == nullptr skips the row sums and the store.
template <int Q, bool VEC, bool WIDE, bool RMS, bool PART>
__global__ __launch_bounds__(kThreads) void layernorm_backward_kernel(
    const float* __restrict__ dy, const float* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ w, float* __restrict__ dx,
    float* __restrict__ part, int R, int N) {
  constexpr int L = WIDE ? kThreads : 64, E = 4 * Q;
  constexpr int kPlanes = RMS ? 1 : 2;
  __shared__ float red[2][2][4];  // [row parity][sum][wave]
  __shared__ float comb[PART && !WIDE ? 4 * 64 * E : 1];
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int t = WIDE ? threadIdx.x : threadIdx.x & 63;
  const int group = WIDE ? blockIdx.x : blockIdx.x * 4 + wave;
  const int groups = WIDE ? gridDim.x : gridDim.x * 4;
  const float n = static_cast<float>(N);

  float gw[E], aw[E], ab[E];
  if (w != nullptr) load_row<Q, VEC, L>(gw, row_rsrc(w, N), t);
#pragma unroll
  for (int i = 0; i < E; ++i) aw[i] = ab[i] = 0.f;

  // wide: every thread of the workgroup runs the same trips, so the barriers match
  int parity = 0;
  for (int64_t row = group; row < R; row += groups, parity ^= 1) {
    float g[E], v[E];
    load_row<Q, VEC, L>(g, row_rsrc(dy + row * N, N), t);
    load_row<Q, VEC, L>(v, row_rsrc(x + row * N, N), t);
    const float rs = rstd[row];
    float m = 0.f;
    if constexpr (!RMS) m = mean[row];
    float s1 = 0.f, s2 = 0.f;
    // columns past N: dy = 0, so they add nothing to the sums or the partials
#pragma unroll
    for (int i = 0; i < E; ++i) {
      v[i] = (v[i] - m) * rs;
      if constexpr (PART) {
        aw[i] += g[i] * v[i];
        if constexpr (!RMS) ab[i] += g[i];
      }
      if (w != nullptr) g[i] *= gw[i];
      s1 += g[i];
      s2 += g[i] * v[i];
    }
    if (dx == nullptr) continue;
    float c1 = 0.f;
    if constexpr (!RMS) c1 = group_sum<false>(s1, nullptr, wave);
    float c2 = group_sum<false>(s2, nullptr, wave);
    if constexpr (WIDE) {
      if ((threadIdx.x & 63) == 0) {
        red[parity][0][wave] = c1;
        red[parity][1][wave] = c2;
      }
      __syncthreads();  // one barrier per row: the other parity's slots are free by now
      const float(*s)[4] = red[parity];
      c1 = ((s[0][0] + s[0][1]) + s[0][2]) + s[0][3];
      c2 = ((s[1][0] + s[1][1]) + s[1][2]) + s[1][3];
    }
    c1 /= n;
    c2 /= n;
#pragma unroll
    for (int i = 0; i < E; ++i) g[i] = rs * (g[i] - c1 - v[i] * c2);
    store_row<Q, VEC, L>(g, row_rsrc(dx + row * N, N), t);
  }

  if constexpr (PART) {
    float* out = part + static_cast<int64_t>(blockIdx.x) * kPlanes * N;
    if constexpr (WIDE) {
      store_row<Q, VEC, L>(aw, row_rsrc(out, N), t);
      if constexpr (!RMS) store_row<Q, VEC, L>(ab, row_rsrc(out + N, N), t);
    } else {
      constexpr int C = 64 * E;  // columns a wave covers
#pragma unroll
      for (int plane = 0; plane < kPlanes; ++plane) {
        if (plane > 0) __syncthreads();
#pragma unroll
        for (int i = 0; i < E; ++i)
          comb[wave * C + column<VEC, 64>(i, t)] = plane == 0 ? aw[i] : ab[i];
        __syncthreads();
        for (int c = threadIdx.x; c < N; c += kThreads)
          out[plane * N + c] = ((comb[c] + comb[C + c]) + comb[2 * C + c]) + comb[3 * C + c];
      }
    }
  }
}

// out[plane][c] (+)= sum_g part[g][plane][c]: a block of 32 columns x 8 segments of g; each
// segment in index order, then the segments in order.  grid (ceil(N / 32), planes); a null
// output skips its plane; bit `plane` of accumulate_mask adds into the output.
__global__ __launch_bounds__(kThreads) void layernorm_reduce_kernel(
    const float* __restrict__ part, int G, int planes, int N, float* __restrict__ dw,
    float* __restrict__ db, int accumulate_mask) {
  __shared__ float sm[kSegments][kReduceCols];
  const int plane = blockIdx.y;
  float* out = plane == 0 ? dw : db;
  if (out == nullptr) return;
  const int lane = threadIdx.x % kReduceCols, seg = threadIdx.x / kReduceCols;
  const int c = blockIdx.x * kReduceCols + lane;
  const int per = (G + kSegments - 1) / kSegments;
  const int g0 = seg * per, g1 = min(G, g0 + per);
  float s = 0.f;
  if (c < N)
    for (int g = g0; g < g1; ++g) s += part[(static_cast<int64_t>(g) * planes + plane) * N + c];
  sm[seg][lane] = s;
  __syncthreads();
  if (seg == 0 && c < N) {
    float total = sm[0][lane];
#pragma unroll
    for (int k = 1; k < kSegments; ++k) total += sm[k][lane];
    out[c] = (accumulate_mask >> plane) & 1 ? out[c] + total : total;
  }
}

bool aligned16(const void* p) { return p == nullptr || reinterpret_cast<uintptr_t>(p) % 16 == 0; }

bool use_wide(int N) {
  const int f = forced_wide.load();
  if (f == 0) return N > kWaveRowCap;
  if (f == 1) return true;
  return N > kWaveRowMax;
}

struct FwdArgs {
  const float *x, *w, *b;
  float *y, *mean, *rstd;
  int R, N;
  float eps;
};

template <int Q, bool WIDE, bool RMS>
void forward_q(const FwdArgs& a, bool vec, hipStream_t stream) {
  const dim3 grid(WIDE ? a.R : (a.R + 3) / 4), block(kThreads);
  if (vec)
    hipLaunchKernelGGL((layernorm_forward_kernel<Q, true, WIDE, RMS>), grid, block, 0, stream,
                       a.x, a.w, a.b, a.y, a.mean, a.rstd, a.R, a.N, a.eps);
  else
    hipLaunchKernelGGL((layernorm_forward_kernel<Q, false, WIDE, RMS>), grid, block, 0, stream,
                       a.x, a.w, a.b, a.y, a.mean, a.rstd, a.R, a.N, a.eps);
}

struct BwdArgs {
  const float *dy, *x, *mean, *rstd, *w;
  float *dx, *part;
  int R, N, grid;
};

template <int Q, bool WIDE, bool RMS>
void backward_q(const BwdArgs& a, bool vec, hipStream_t stream) {
  const dim3 grid(a.grid), block(kThreads);
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, grid, block, 0, stream, a.dy, a.x, a.mean, a.rstd, a.w, a.dx,
                       a.part, a.R, a.N);
  };
  if (a.part != nullptr) {
    if (vec) go(layernorm_backward_kernel<Q, true, WIDE, RMS, true>);
    else go(layernorm_backward_kernel<Q, false, WIDE, RMS, true>);
  } else {
    if (vec) go(layernorm_backward_kernel<Q, true, WIDE, RMS, false>);
    else go(layernorm_backward_kernel<Q, false, WIDE, RMS, false>);
  }
}

// The instance: the smallest Q whose 4 Q L columns hold the row.
template <typename Narrow, typename Wide>
void pick(bool use_wide_instance, int N, Narrow narrow, Wide wide) {
  if (use_wide_instance) {
    const int q = (N + 4 * kThreads - 1) / (4 * kThreads);
    if (q <= 2) wide(std::integral_constant<int, 2>{});
    else if (q <= 4) wide(std::integral_constant<int, 4>{});
    else wide(std::integral_constant<int, 8>{});
  } else {
    const int q = (N + 255) / 256;
    if (q <= 1) narrow(std::integral_constant<int, 1>{});
    else if (q <= 2) narrow(std::integral_constant<int, 2>{});
    else if (q <= 3) narrow(std::integral_constant<int, 3>{});
    else if (q <= 4) narrow(std::integral_constant<int, 4>{});
    else narrow(std::integral_constant<int, 8>{});
  }
}

}  // namespace

void layernorm_force_instance(int wide) { forced_wide.store(wide == 0 || wide == 1 ? wide : -1); }

int layernorm_wave_row_max() { return kWaveRowMax; }

// The only reader of the forcing hook: a call decides once and carries its plan along.
LayerNormPlan layernorm_plan(int R, int N) {
  LayerNormPlan plan;
  plan.wide = use_wide(N);
  plan.grid = plan.wide ? std::min(kWidePerCU * kCUs, R)
                        : std::min(kNarrowPerCU * kCUs, (R + 3) / 4);
  return plan;
}

int layernorm_backward_sweep(int N) {
  return use_wide(N) ? kWidePerCU * kCUs : 4 * kNarrowPerCU * kCUs;
}

void launch_layernorm_forward(const float* x, const float* w, const float* b, float* y,
                              float* mean, float* rstd, int R, int N, float eps, bool rms,
                              hipStream_t stream) {
  const FwdArgs a{x, w, b, y, mean, rstd, R, N, eps};
  const bool vec = N % 4 == 0 && aligned16(x) && aligned16(w) && aligned16(b) && aligned16(y);
  const bool wide = use_wide(N);
  auto go = [&](auto rms_c) {
    constexpr bool RMS = decltype(rms_c)::value;
    pick(
        wide, N, [&](auto q) { forward_q<decltype(q)::value, false, RMS>(a, vec, stream); },
        [&](auto q) { forward_q<decltype(q)::value, true, RMS>(a, vec, stream); });
  };
  if (rms) go(std::true_type{});
  else go(std::false_type{});
}

void launch_layernorm_backward(const float* dy, const float* x, const float* mean,
                               const float* rstd, const float* w, float* dx, float* part,
                               float* dw, float* db, bool accumulate_dw, bool accumulate_db,
                               int R, int N, bool rms, const LayerNormPlan& plan,
                               hipStream_t stream) {
  const BwdArgs a{dy, x, mean, rstd, w, dx, part, R, N, plan.grid};
  const bool vec = N % 4 == 0 && aligned16(dy) && aligned16(x) && aligned16(w) &&
                   aligned16(dx) && aligned16(part);
  auto go = [&](auto rms_c) {
    constexpr bool RMS = decltype(rms_c)::value;
    pick(
        plan.wide, N, [&](auto q) { backward_q<decltype(q)::value, false, RMS>(a, vec, stream); },
        [&](auto q) { backward_q<decltype(q)::value, true, RMS>(a, vec, stream); });
  };
  if (rms) go(std::true_type{});
  else go(std::false_type{});
  if (part == nullptr) return;
  const int planes = rms ? 1 : 2;
  hipLaunchKernelGGL(layernorm_reduce_kernel, dim3((N + kReduceCols - 1) / kReduceCols, planes),
                     dim3(kThreads), 0, stream, part, a.grid, planes, N, dw, db,
                     (accumulate_dw ? 1 : 0) | (accumulate_db ? 2 : 0));
}

}  // namespace tgpipe
