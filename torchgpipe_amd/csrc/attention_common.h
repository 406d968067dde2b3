// What the fused attention kernels of every head dim share (attention.hip: 64,
// attention128.hip: 128): the split-bf16 arithmetic, the buffer-load view of a [B, H, T, D]
// operand, the accumulator-register order of the 32 x 32 score tile, the grid order and the
// level dispatch.  Device code: included by the .hip files only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "kernels.h"

namespace tgpipe {

// attention128.hip
void launch_attention128_forward(const AttnArgs& args, bool causal, hipStream_t stream);
void launch_attention128_backward(const AttnArgs& args, bool causal, hipStream_t stream);

namespace attn {

typedef float floatx4 __attribute__((ext_vector_type(4)));
typedef float floatx16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

constexpr int kBlk = 32;                 // walked rows per stage
constexpr int kOwn = 128;                // owned rows per workgroup (4 waves x 32)
constexpr int kThreads = 256;
constexpr uint32_t kOOB = 0x7ffffff0u;   // buffer offset past every tensor (< 2 GiB)
constexpr int kPairs[6][2] = {{2, 0}, {0, 2}, {1, 1}, {1, 0}, {0, 1}, {0, 0}};

constexpr int first_pair(int lv) { return lv == 0 ? 0 : (lv == 1 ? 3 : 5); }

// one [B, H, T, D] operand of one (batch, head): buffer resource of the whole view, byte
// offset of the (b, h) slice, bytes between rows
struct Rows {
  __amdgpu_buffer_rsrc_t rs;
  uint32_t base, pitch;
};

__device__ __forceinline__ Rows rows_of(const AttnTensor& t, int b, int h) {
  Rows r;
  r.rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(t.p), static_cast<short>(0),
                                           static_cast<int>(t.bytes), 0x00020000);
  r.base = static_cast<uint32_t>((b * t.sb + h * t.sh) * 4);
  r.pitch = static_cast<uint32_t>(t.st * 4);
  return r;
}

__device__ __forceinline__ floatx4 bload4(__amdgpu_buffer_rsrc_t r, uint32_t off) {
  const auto v = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
  return floatx4{__uint_as_float(v[0]), __uint_as_float(v[1]), __uint_as_float(v[2]),
                 __uint_as_float(v[3])};
}

// split1 of conv_gemm.hip on N values: round to nearest, each part of the remainder of the
// one before; the first 3 - LV planes.
template <int LV, int N, typename V, typename F>
__device__ __forceinline__ void split(F&& get, V (&out)[3 - LV]) {
#pragma unroll
  for (int e = 0; e < N; ++e) {
    const float v = get(e);
    const __bf16 hi = static_cast<__bf16>(v);
    out[0][e] = hi;
    if constexpr (LV < 2) {
      const float r = v - static_cast<float>(hi);
      const __bf16 mid = static_cast<__bf16>(r);
      out[1][e] = mid;
      if constexpr (LV == 0) out[2][e] = static_cast<__bf16>(r - static_cast<float>(mid));
    }
  }
}

// the 32 x 32 tile's registers 0-7 and 8-15 as the B fragments of the next GEMM
template <int LV>
__device__ __forceinline__ void split_tile(const floatx16& t, bf16x8 (&f)[2][3 - LV]) {
#pragma unroll
  for (int u = 0; u < 2; ++u) split<LV, 8>([&](int e) { return t[8 * u + e]; }, f[u]);
}

__device__ __forceinline__ int walked_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

__device__ __forceinline__ void zero(floatx16& a) {
#pragma unroll
  for (int r = 0; r < 16; ++r) a[r] = 0.f;
}

// The workgroup's (row block, batch * head) in the one-dimensional grid.  Uniform work: row
// blocks fastest, so neighbours share their (b, h)'s walked tensors in cache.  Causal: a row
// block's walk grows (GROWS: queries own) or shrinks (keys own) with its index; every (b, h)
// of the longest walk is dispatched first, then the next, and the grid's tail is short walks.
struct Where {
  int rb, bh;
};
template <bool CAUSAL, bool GROWS>
__device__ __forceinline__ Where where(const AttnArgs& p) {
  const int nb = (p.T + kOwn - 1) / kOwn, id = blockIdx.x;
  if constexpr (CAUSAL) {
    const int n = p.B * p.H, r = id / n;
    return Where{GROWS ? nb - 1 - r : r, id % n};
  } else {
    return Where{id % nb, id / nb};
  }
}

// f(level constant, causal constant) for the level in force (read at launch: a captured graph
// keeps its own)
template <typename F>
void with_instance(bool causal, F&& f) {
  auto at = [&](auto lv) {
    if (causal) f(lv, std::true_type{});
    else f(lv, std::false_type{});
  };
  const int lv = conv_precision_level();
  if (lv == 1) at(std::integral_constant<int, 1>{});
  else if (lv == 2) at(std::integral_constant<int, 2>{});
  else at(std::integral_constant<int, 0>{});
}

inline dim3 attn_grid(const AttnArgs& a) { return dim3((a.T + kOwn - 1) / kOwn * a.B * a.H); }

}  // namespace attn
}  // namespace tgpipe
