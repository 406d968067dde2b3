// Wire format of inter-stage messages (ops/misc.py pack_wire / unpack_wire): K6's
// multi-segment pack / unpack with an optional precision change per segment, one launch
// per message (blockIdx.y = segment, by-value table).
//
//   kWireCopy    bytes verbatim (what segments_copy_kernel does): tensors that are not fp32
//   kWireEncode  fp32 -> bf16, round to nearest even (to_bf16: a finite value past the
//                largest bf16 becomes inf, NaN stays NaN)
//   kWireDecode  bf16 -> fp32, exact (the 16 bits become the high half)
//
// Vector path when both sides of a segment are 16-byte aligned: a thread turns 8 elements
// per step (encode: two 16-byte loads, one 16-byte store; decode: one load, two stores),
// grid-stride, the n % 8 tail element by element.  Otherwise every element goes alone.
// The encode reads its source once and nothing reads it again before the link does, so the
// grid is sized to keep the loads in flight rather than to cover the tensor: up to
// kWireBlocks blocks of 256 threads per launch, two steps (64 B of loads per thread) issued
// before the first store -- 2048 blocks x 256 x 64 B = 128 KiB per CU over 256 CUs, past
// the ~32 KiB per CU that saturates HBM.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "bf16_round.h"
#include "kernels.h"

namespace tgpipe {
namespace {

constexpr int kThreads = 256;
constexpr int64_t kWireBlocks = 2048;  // all segments of a launch together

struct WireTable {
  WireSegment seg[kMaxSegments];
};

__device__ __forceinline__ uint4 encode8(const uint4& a, const uint4& b) {
  uint4 r;
  r.x = to_bf16x2(__uint_as_float(a.x), __uint_as_float(a.y));
  r.y = to_bf16x2(__uint_as_float(a.z), __uint_as_float(a.w));
  r.z = to_bf16x2(__uint_as_float(b.x), __uint_as_float(b.y));
  r.w = to_bf16x2(__uint_as_float(b.z), __uint_as_float(b.w));
  return r;
}

__device__ __forceinline__ void wire_copy(const WireSegment& sg, int64_t tid, int64_t stride) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(sg.src) | reinterpret_cast<uintptr_t>(sg.dst);
  const char* sb = reinterpret_cast<const char*>(sg.src);
  char* db = reinterpret_cast<char*>(sg.dst);
  int64_t done = 0;
  if ((a & 15) == 0) {
    const int64_t nvec = sg.count / 16;
    const uint4* s = reinterpret_cast<const uint4*>(sg.src);
    uint4* d = reinterpret_cast<uint4*>(sg.dst);
    for (int64_t i = tid; i < nvec; i += stride) d[i] = s[i];
    done = nvec * 16;
  }
  for (int64_t i = done + tid; i < sg.count; i += stride) db[i] = sb[i];
}

__device__ __forceinline__ void wire_encode(const WireSegment& sg, int64_t tid, int64_t stride) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(sg.src) | reinterpret_cast<uintptr_t>(sg.dst);
  const float* sf = reinterpret_cast<const float*>(sg.src);
  uint16_t* dh = reinterpret_cast<uint16_t*>(sg.dst);
  int64_t done = 0;
  if ((a & 15) == 0) {
    const int64_t nvec = sg.count / 8;  // steps of 8 elements: 32 B in, 16 B out
    const uint4* s = reinterpret_cast<const uint4*>(sg.src);
    uint4* d = reinterpret_cast<uint4*>(sg.dst);
    int64_t i = tid;
    for (; i + stride < nvec; i += 2 * stride) {
      const uint4 a0 = s[2 * i], b0 = s[2 * i + 1];
      const uint4 a1 = s[2 * (i + stride)], b1 = s[2 * (i + stride) + 1];
      d[i] = encode8(a0, b0);
      d[i + stride] = encode8(a1, b1);
    }
    if (i < nvec) d[i] = encode8(s[2 * i], s[2 * i + 1]);
    done = nvec * 8;
  }
  for (int64_t i = done + tid; i < sg.count; i += stride)
    dh[i] = static_cast<uint16_t>(to_bf16(sf[i]));
}

__device__ __forceinline__ void wire_decode(const WireSegment& sg, int64_t tid, int64_t stride) {
  const uintptr_t a = reinterpret_cast<uintptr_t>(sg.src) | reinterpret_cast<uintptr_t>(sg.dst);
  const uint16_t* sh = reinterpret_cast<const uint16_t*>(sg.src);
  uint32_t* dw = reinterpret_cast<uint32_t*>(sg.dst);
  int64_t done = 0;
  if ((a & 15) == 0) {
    const int64_t nvec = sg.count / 8;  // steps of 8 elements: 16 B in, 32 B out
    const uint4* s = reinterpret_cast<const uint4*>(sg.src);
    uint4* d = reinterpret_cast<uint4*>(sg.dst);
    for (int64_t i = tid; i < nvec; i += stride) {
      const uint4 v = s[i];
      d[2 * i] = make_uint4(v.x << 16, v.x & 0xffff0000u, v.y << 16, v.y & 0xffff0000u);
      d[2 * i + 1] = make_uint4(v.z << 16, v.z & 0xffff0000u, v.w << 16, v.w & 0xffff0000u);
    }
    done = nvec * 8;
  }
  for (int64_t i = done + tid; i < sg.count; i += stride)
    dw[i] = static_cast<uint32_t>(sh[i]) << 16;
}

__global__ __launch_bounds__(kThreads) void wire_segments_kernel(WireTable table) {
  const WireSegment sg = table.seg[blockIdx.y];
  const int64_t stride = static_cast<int64_t>(gridDim.x) * blockDim.x;
  const int64_t tid = static_cast<int64_t>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (sg.mode == kWireEncode) {  // (uniform over the block)
    wire_encode(sg, tid, stride);
  } else if (sg.mode == kWireDecode) {
    wire_decode(sg, tid, stride);
  } else {
    wire_copy(sg, tid, stride);
  }
}

}  // namespace

void launch_wire_segments(const WireSegment* segs, int count, hipStream_t stream) {
  if (count <= 0) return;
  const int n = count < kMaxSegments ? count : kMaxSegments;
  WireTable table{};
  int64_t steps = 0;  // 16-byte stores of the largest segment
  for (int i = 0; i < n; ++i) {
    table.seg[i] = segs[i];
    const int64_t s = segs[i].mode == kWireCopy ? segs[i].count / 16 : segs[i].count / 8;
    if (s > steps) steps = s;
  }
  int64_t grid = (steps + kThreads - 1) / kThreads;
  const int64_t cap = kWireBlocks / n;
  if (grid > cap) grid = cap;
  if (grid < 1) grid = 1;
  hipLaunchKernelGGL(wire_segments_kernel, dim3(static_cast<unsigned>(grid), n), dim3(kThreads),
                     0, stream, table);
}

}  // namespace tgpipe
