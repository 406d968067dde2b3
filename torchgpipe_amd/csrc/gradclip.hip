// Global-norm gradient clipping over a list of gradients (ops/gradclip.py):
//
//   grad_sumsq:  sum of squares of every element of every tensor, in fp64 from the element
//                on -- each value is widened to double before it is squared, and the lane,
//                wave and block sums are double, so 1e25 does not overflow and 1e-25 does
//                not vanish.  One block per chunk writes one partial to its own workspace
//                slot; a one-block kernel adds the slots in a fixed order.  No atomics: the
//                result is the same from run to run.
//   grad_scale:  every block reads the (possibly since all-reduced) sum of squares, forms
//                coef = max_norm / (sqrt(sumsq) + eps) in fp64 and returns at once when
//                coef >= 1 -- a uniform branch ahead of any gradient access.  Otherwise
//                (coef < 1 or NaN) every element is multiplied in place by (float)coef;
//                bf16 is widened, multiplied in f32 and rounded to nearest even once.
//
// Multi-tensor launches take a by-value table (GradTable): per tensor its base pointer, the
// exclusive prefix sum of its chunk count and the length of its last chunk.  A block finds
// its tensor by binary search over the prefix array -- wave-uniform, from kernel arguments,
// so it is safe under graph capture (no device-resident table to keep alive).
//
// A chunk is kGradClipThreads lanes x kLoads 16-byte slots.  Lane l owns slots l, l + 256,
// ... of the chunk, counted from the tensor's first element, whatever the tensor's address:
// a full chunk of a 16-byte aligned tensor loads a slot with one 16-byte load, any other
// tensor (and the last, ragged chunk) with scalar loads of the same elements into the same
// registers.  The arithmetic after the loads is shared, so the sum is bitwise the same at any
// storage offset.  All of a lane's loads are issued before the first use: 32 KiB in flight
// per block, the streaming condition with one resident block per CU.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf16_round.h"
#include "kernels.h"

namespace tgpipe {
namespace {

constexpr int kThreads = kGradClipThreads;
constexpr int kLoads = 8;  // 16-byte slots per lane and chunk
constexpr int kFinalThreads = 1024;
constexpr int kMaxChunks = 1 << 30;  // per launch: the prefix sums are int32
static_assert(kGradClipChunkF32 == int64_t{kThreads} * kLoads * 4, "fp32 chunk");
static_assert(kGradClipChunkBF16 == int64_t{kThreads} * kLoads * 8, "bf16 chunk");

struct GradTable {
  void* ptr[kGradClipTensors];
  int32_t first[kGradClipTensors + 1];  // first[t]: chunks ahead of tensor t; first[count]: all
  int32_t last[kGradClipTensors];       // elements of tensor t's last chunk (1 .. chunk)
  int32_t count;
};
static_assert(sizeof(GradTable) <= 3200, "table + arguments + implicit arguments < 4 KB");

// The chunk a block works on: elements [0, valid) from `base`.
template <typename E>
struct Chunk {
  E* base;
  int valid;
  bool aligned;
};

template <typename E>
__device__ __forceinline__ Chunk<E> chunk_of(const GradTable& table) {
  constexpr int kVec = 16 / sizeof(E);
  constexpr int kChunk = kThreads * kLoads * kVec;
  const int b = static_cast<int>(blockIdx.x);
  int lo = 0, hi = table.count;  // the last t in [0, count) with first[t] <= b
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (table.first[mid] <= b) lo = mid; else hi = mid;
  }
  Chunk<E> c;
  c.base = static_cast<E*>(table.ptr[lo]) + static_cast<int64_t>(b - table.first[lo]) * kChunk;
  c.valid = b + 1 == table.first[lo + 1] ? table.last[lo] : kChunk;
  c.aligned = (reinterpret_cast<uintptr_t>(c.base) & 15) == 0;
  return c;
}

// 16 bytes of elements [e, e + kVec) as a 16-byte load would return them, from scalar loads;
// elements at or past `valid` (>= 1) read as zero bits.  The index is clamped instead of the
// load skipped, so the loads stay unconditional and all of a lane's are in flight at once.
__device__ __forceinline__ uint32_t load_elem(const float* p, int i, int valid) {
  const uint32_t v = __float_as_uint(p[i < valid ? i : valid - 1]);
  return i < valid ? v : 0u;
}
__device__ __forceinline__ uint32_t load_elem(const bf16_bits* p, int i, int valid) {
  const uint32_t v = p[i < valid ? i : valid - 1];
  return i < valid ? v : 0u;
}
__device__ __forceinline__ uint4 load_slot(const float* p, int e, int valid) {
  return make_uint4(load_elem(p, e, valid), load_elem(p, e + 1, valid),
                    load_elem(p, e + 2, valid), load_elem(p, e + 3, valid));
}
__device__ __forceinline__ uint4 load_slot(const bf16_bits* p, int e, int valid) {
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    w[k] = load_elem(p, e + 2 * k, valid) | (load_elem(p, e + 2 * k + 1, valid) << 16);
  return make_uint4(w[0], w[1], w[2], w[3]);
}

template <typename E>
__device__ __forceinline__ void load_chunk(const Chunk<E>& c, uint4 (&raw)[kLoads]) {
  constexpr int kVec = 16 / sizeof(E);
  constexpr int kChunk = kThreads * kLoads * kVec;
  const int tid = static_cast<int>(threadIdx.x);
  if (c.aligned && c.valid == kChunk) {
#pragma unroll
    for (int i = 0; i < kLoads; ++i)
      raw[i] = reinterpret_cast<const uint4*>(c.base)[i * kThreads + tid];
    return;
  }
#pragma unroll
  for (int i = 0; i < kLoads; ++i)
    raw[i] = load_slot(c.base, (i * kThreads + tid) * kVec, c.valid);
}

// The f32 value of element k (0 .. kVec - 1) of a slot.
template <typename E>
__device__ __forceinline__ float widen(const uint32_t (&w)[4], int k);
template <>
__device__ __forceinline__ float widen<float>(const uint32_t (&w)[4], int k) {
  return __uint_as_float(w[k]);
}
template <>
__device__ __forceinline__ float widen<bf16_bits>(const uint32_t (&w)[4], int k) {
  return __uint_as_float(k & 1 ? w[k >> 1] & 0xffff0000u : w[k >> 1] << 16);
}

// Sum over the block in a fixed order; the result is valid on thread 0.
template <int THREADS>
__device__ __forceinline__ double block_sum(double v, double* lds) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  const int wave = static_cast<int>(threadIdx.x) >> 6;
  if ((threadIdx.x & 63) == 0) lds[wave] = v;
  __syncthreads();
  double total = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < THREADS / 64; ++w) total += lds[w];
  }
  return total;
}

template <typename E>
__global__ __launch_bounds__(kThreads) void grad_sumsq_kernel(GradTable table,
                                                              double* __restrict__ partials) {
  constexpr int kVec = 16 / sizeof(E);
  __shared__ double lds[kThreads / 64];
  const Chunk<E> c = chunk_of<E>(table);
  uint4 raw[kLoads];
  load_chunk<E>(c, raw);
  double acc = 0.0;
#pragma unroll
  for (int i = 0; i < kLoads; ++i) {
    const uint32_t w[4] = {raw[i].x, raw[i].y, raw[i].z, raw[i].w};
#pragma unroll
    for (int k = 0; k < kVec; ++k) {
      const double x = static_cast<double>(widen<E>(w, k));
      acc = fma(x, x, acc);
    }
  }
  const double total = block_sum<kThreads>(acc, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// out[0] = partials[0] + ... + partials[n - 1], one block, a fixed order.
__global__ __launch_bounds__(kFinalThreads) void grad_sumsq_final_kernel(
    const double* __restrict__ partials, int64_t n, double* __restrict__ out) {
  __shared__ double lds[kFinalThreads / 64];
  double acc = 0.0;
  for (int64_t i = threadIdx.x; i < n; i += kFinalThreads) acc += partials[i];
  const double total = block_sum<kFinalThreads>(acc, lds);
  if (threadIdx.x == 0) out[0] = total;
}

__device__ __forceinline__ uint4 scale_slot(uint4 v, float f, const float*) {
  return make_uint4(__float_as_uint(__uint_as_float(v.x) * f),
                    __float_as_uint(__uint_as_float(v.y) * f),
                    __float_as_uint(__uint_as_float(v.z) * f),
                    __float_as_uint(__uint_as_float(v.w) * f));
}
__device__ __forceinline__ uint4 scale_slot(uint4 v, float f, const bf16_bits*) {
  uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const uint32_t lo = to_bf16(__uint_as_float(w[k] << 16) * f);
    const uint32_t hi = to_bf16(__uint_as_float(w[k] & 0xffff0000u) * f);
    w[k] = lo | (hi << 16);
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

__device__ __forceinline__ void store_slot(float* p, int e, int valid, uint4 v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (e + k < valid) p[e + k] = __uint_as_float(w[k]);
}
__device__ __forceinline__ void store_slot(bf16_bits* p, int e, int valid, uint4 v) {
  const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
  for (int k = 0; k < 8; ++k)
    if (e + k < valid) p[e + k] = static_cast<bf16_bits>(k & 1 ? w[k >> 1] >> 16 : w[k >> 1]);
}

template <typename E>
__global__ __launch_bounds__(kThreads) void grad_scale_kernel(GradTable table,
                                                              const double* __restrict__ sumsq,
                                                              double max_norm, double eps) {
  constexpr int kVec = 16 / sizeof(E);
  constexpr int kChunk = kThreads * kLoads * kVec;
  const double coef = max_norm / (sqrt(sumsq[0]) + eps);
  if (coef >= 1.0) return;  // not clipped: no gradient is read or written (NaN goes on)
  const float f = static_cast<float>(coef);
  const Chunk<E> c = chunk_of<E>(table);
  const int tid = static_cast<int>(threadIdx.x);
  uint4 raw[kLoads];
  load_chunk<E>(c, raw);
  if (c.aligned && c.valid == kChunk) {
#pragma unroll
    for (int i = 0; i < kLoads; ++i)
      reinterpret_cast<uint4*>(c.base)[i * kThreads + tid] = scale_slot(raw[i], f, c.base);
    return;
  }
#pragma unroll
  for (int i = 0; i < kLoads; ++i)  // element by element: nothing at or past `valid` is written
    store_slot(c.base, (i * kThreads + tid) * kVec, c.valid, scale_slot(raw[i], f, c.base));
}

int64_t chunk_elems(int elem_bytes) {
  return elem_bytes == 4 ? kGradClipChunkF32 : kGradClipChunkBF16;
}

// Calls launch(table, blocks, first_block) for each table's worth of `spans`; returns the
// number of blocks over all launches.
template <typename F>
int64_t for_each_table(const GradSpan* spans, int count, int elem_bytes, F launch) {
  const int64_t chunk = chunk_elems(elem_bytes);
  int64_t done = 0;
  GradTable table{};
  int64_t chunks = 0;
  auto flush = [&]() {
    if (table.count == 0) return;
    table.first[table.count] = static_cast<int32_t>(chunks);
    launch(table, static_cast<unsigned>(chunks), done);
    done += chunks;
    table = GradTable{};
    chunks = 0;
  };
  for (int i = 0; i < count; ++i) {
    if (spans[i].numel <= 0) continue;
    const int64_t n = (spans[i].numel + chunk - 1) / chunk;
    if (table.count == kGradClipTensors || chunks + n > kMaxChunks) flush();
    table.ptr[table.count] = spans[i].ptr;
    table.first[table.count] = static_cast<int32_t>(chunks);
    table.last[table.count] = static_cast<int32_t>(spans[i].numel - (n - 1) * chunk);
    ++table.count;
    chunks += n;
  }
  flush();
  return done;
}

}  // namespace

int64_t grad_clip_blocks(const GradSpan* spans, int count, int elem_bytes) {
  const int64_t chunk = chunk_elems(elem_bytes);
  int64_t blocks = 0;
  for (int i = 0; i < count; ++i)
    if (spans[i].numel > 0) blocks += (spans[i].numel + chunk - 1) / chunk;
  return blocks;
}

void launch_grad_sumsq(const GradSpan* spans, int count, int elem_bytes, double* partials,
                       double* out, hipStream_t stream) {
  const int64_t blocks = for_each_table(
      spans, count, elem_bytes, [&](const GradTable& table, unsigned grid, int64_t first) {
        if (elem_bytes == 4) {
          hipLaunchKernelGGL(grad_sumsq_kernel<float>, dim3(grid), dim3(kThreads), 0, stream,
                             table, partials + first);
        } else {
          hipLaunchKernelGGL(grad_sumsq_kernel<bf16_bits>, dim3(grid), dim3(kThreads), 0, stream,
                             table, partials + first);
        }
      });
  hipLaunchKernelGGL(grad_sumsq_final_kernel, dim3(1), dim3(kFinalThreads), 0, stream,
                     static_cast<const double*>(partials), blocks, out);
}

void launch_grad_scale(const GradSpan* spans, int count, int elem_bytes, const double* sumsq,
                       double max_norm, double eps, hipStream_t stream) {
  for_each_table(spans, count, elem_bytes,
                 [&](const GradTable& table, unsigned grid, int64_t) {
                   if (elem_bytes == 4) {
                     hipLaunchKernelGGL(grad_scale_kernel<float>, dim3(grid), dim3(kThreads), 0,
                                        stream, table, sumsq, max_norm, eps);
                   } else {
                     hipLaunchKernelGGL(grad_scale_kernel<bf16_bits>, dim3(grid), dim3(kThreads),
                                        0, stream, table, sumsq, max_norm, eps);
                   }
                 });
}

}  // namespace tgpipe
