// Fused optimizer steps over lists of parameters (torchgpipe_amd/optim.py):
//
//   sgd_step:      d = g + wd * p;  buf = mu * buf + (1 - damp) * d  (first step: buf = d);
//                  p -= lr * (nesterov ? d + mu * buf : buf)          (no momentum: p -= lr * d)
//   rmsprop_step:  d = g + wd * p;  sq = alpha * sq + (1 - alpha) * d * d;
//                  centred: ga = lerp(ga, d, 1 - alpha), avg = sqrt(sq - ga * ga) + eps,
//                  otherwise avg = sqrt(sq) + eps;
//                  buf = mu * buf + d / avg, p -= lr * buf            (no momentum: p -= lr * d / avg)
//
// in the order of torch/optim's single-tensor loops.  One pass: `grad` is read once, `param`
// and every state tensor are read once and written once.
//
// The learning rate is read from a device fp32 scalar, so a schedule changes it between the
// replays of a captured step.  With `sumsq` (the fp64 sum of squares of all gradients,
// grad_sumsq's result, possibly all-reduced since) every block forms
// coef = max_norm / (sqrt(sumsq) + eps) in fp64 as grad_scale_kernel does; when coef < 1 or is
// NaN each gradient is multiplied by (float)coef as it is loaded, rounded on its own
// (__fmul_rn: never contracted into the add that follows), so the step is bitwise what
// grad_scale_ followed by the unclipped step gives.  The gradients are never written.
//
// Launches follow gradclip.hip: a by-value table (OptimTable) with up to kOptimStreams
// pointers per tensor -- stream 0 the parameter, 1 the gradient, 2.. the state tensors -- the
// exclusive prefix sum of the chunk counts and the length of each tensor's last chunk; a
// block finds its tensor by binary search over the prefix array, from kernel arguments only.
//
// A chunk is kOptimThreads lanes x kLoads 16-byte slots per stream.  A full chunk whose
// pointers are all 16-byte aligned moves every slot with one 16-byte load or store; any other
// chunk loads the same elements with scalar loads into the same registers and stores element
// by element below `valid`.  The arithmetic is shared, so the results are bitwise the same at
// any storage offset.  All of a lane's loads are issued before the first use.  kLoads = 4:
// a stream is 16 VGPRs of loads, so the kernels compile to 76 VGPRs (SGD), 106 (SGD with
// momentum), 105 / 122 / 128 (RMSprop with three or four streams) and 141 (all five), without
// scratch: 6 / 4 / 4 / 4 / 4 / 3 waves per SIMD, i.e. at least three 256-lane blocks per CU,
// each with 32 - 80 KiB of loads in flight -- several times the 32 KiB per CU that streaming
// takes, with blocks left over to hide the stores.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace tgpipe {
namespace {

constexpr int kThreads = kOptimThreads;
constexpr int kLoads = 4;  // 16-byte slots per lane, stream and chunk
constexpr int kChunk = kThreads * kLoads * 4;
constexpr int kMaxChunks = 1 << 30;  // per launch: the prefix sums are int32
static_assert(kOptimChunk == int64_t{kChunk}, "fp32 chunk");

struct OptimTable {
  float* ptr[kOptimStreams][kOptimTensors];
  int32_t first[kOptimTensors + 1];  // first[t]: chunks ahead of tensor t; first[count]: all
  int32_t last[kOptimTensors];       // elements of tensor t's last chunk (1 .. chunk)
  int32_t count;
};

// What every block reads besides the table.
struct StepArgs {
  const float* lr;
  const double* sumsq;  // null: no clip
  double max_norm;
  double clip_eps;
  float momentum;
  float damp_rest;   // SGD: 1 - dampening
  float weight_decay;
  float alpha;       // RMSprop
  float alpha_rest;  // RMSprop: 1 - alpha
  float eps;         // RMSprop
  int nesterov;
  int first;
};
static_assert(sizeof(OptimTable) + sizeof(StepArgs) <= 3200,
              "table + arguments + implicit arguments < 4 KB");

// The chunk a block works on: elements [0, valid) from each stream's base.
template <int NS>
struct Chunk {
  float* base[NS];
  int valid;
  bool vector;  // a full chunk, every base 16-byte aligned
};

// rows[s]: the table row of the kernel's stream s.
template <int NS>
__device__ __forceinline__ Chunk<NS> chunk_of(const OptimTable& table, const int (&rows)[NS]) {
  const int b = static_cast<int>(blockIdx.x);
  int lo = 0, hi = table.count;  // the last t in [0, count) with first[t] <= b
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (table.first[mid] <= b) lo = mid; else hi = mid;
  }
  Chunk<NS> c;
  const int64_t offset = static_cast<int64_t>(b - table.first[lo]) * kChunk;
  uintptr_t bits = 0;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    c.base[s] = table.ptr[rows[s]][lo] + offset;
    bits |= reinterpret_cast<uintptr_t>(c.base[s]);
  }
  c.valid = b + 1 == table.first[lo + 1] ? table.last[lo] : kChunk;
  c.vector = (bits & 15) == 0 && c.valid == kChunk;
  return c;
}

// Elements at or past `valid` (>= 1) read as zero.  The index is clamped instead of the load
// skipped, so the loads stay unconditional and all of a lane's are in flight at once.
__device__ __forceinline__ float load_elem(const float* p, int i, int valid) {
  const float v = p[i < valid ? i : valid - 1];
  return i < valid ? v : 0.0f;
}

template <int NS>
__device__ __forceinline__ void load_chunk(const Chunk<NS>& c, float4 (&raw)[NS][kLoads]) {
  const int tid = static_cast<int>(threadIdx.x);
  if (c.vector) {
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
      for (int i = 0; i < kLoads; ++i)
        raw[s][i] = reinterpret_cast<const float4*>(c.base[s])[i * kThreads + tid];
    return;
  }
#pragma unroll
  for (int s = 0; s < NS; ++s)
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {
      const int e = (i * kThreads + tid) * 4;
      raw[s][i] = make_float4(load_elem(c.base[s], e, c.valid), load_elem(c.base[s], e + 1, c.valid),
                              load_elem(c.base[s], e + 2, c.valid),
                              load_elem(c.base[s], e + 3, c.valid));
    }
}

// Stores every stream but the gradient's (stream 1).
template <int NS>
__device__ __forceinline__ void store_chunk(const Chunk<NS>& c, const float4 (&raw)[NS][kLoads]) {
  const int tid = static_cast<int>(threadIdx.x);
  if (c.vector) {
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      if (s == 1) continue;
#pragma unroll
      for (int i = 0; i < kLoads; ++i)
        reinterpret_cast<float4*>(c.base[s])[i * kThreads + tid] = raw[s][i];
    }
    return;
  }
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    if (s == 1) continue;
#pragma unroll
    for (int i = 0; i < kLoads; ++i) {  // element by element: nothing at or past `valid`
      const int e = (i * kThreads + tid) * 4;
      const float w[4] = {raw[s][i].x, raw[s][i].y, raw[s][i].z, raw[s][i].w};
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (e + k < c.valid) c.base[s][e + k] = w[k];
    }
  }
}

// The clip coefficient as grad_scale_kernel forms it; `active` when it is below 1 or NaN.
struct Clip {
  bool active;
  float f;
};
__device__ __forceinline__ Clip clip_of(const StepArgs& a) {
  Clip c{false, 1.0f};
  if (a.sumsq != nullptr) {
    const double coef = a.max_norm / (sqrt(a.sumsq[0]) + a.clip_eps);
    c.active = !(coef >= 1.0);
    c.f = static_cast<float>(coef);
  }
  return c;
}

// The arithmetic below spells out every rounding (fmaf where torch's CPU kernels fuse --
// add(alpha), addcmul's last step, lerp -- and separately rounded products, quotients and sums
// where they do not), and nothing else may contract: on fp32 inputs the kernels then give
// what torch.optim's single-tensor loop gives on the CPU.
#pragma clang fp contract(off)

// The gradient the update uses: clipped (rounded on its own), then decayed.
__device__ __forceinline__ float decayed(float g, float p, const Clip& clip, float wd) {
  if (clip.active) g = __fmul_rn(g, clip.f);
  return wd != 0.0f ? fmaf(wd, p, g) : g;  // g.add(p, alpha=wd)
}

struct SgdOp {
  template <bool MOMENTUM>
  static __device__ __forceinline__ void apply(float& p, float g, float* state, const Clip& clip,
                                               float lr, const StepArgs& a) {
    float d = decayed(g, p, clip, a.weight_decay);
    if (MOMENTUM) {
      // buf.mul_(mu).add_(d, alpha=1 - dampening); the first step: buf = d
      const float buf = a.first ? d : fmaf(a.damp_rest, d, a.momentum * state[0]);
      state[0] = buf;
      d = a.nesterov ? fmaf(a.momentum, buf, d) : buf;  // d.add(buf, alpha=mu)
    }
    p = fmaf(-lr, d, p);  // p.add_(d, alpha=-lr)
  }
};

// torch's CPU lerp: start + w * diff below w = 0.5, end + (w - 1) * diff from there on, fused.
__device__ __forceinline__ float lerp_like_torch(float start, float end, float w) {
  const float diff = end - start;
  return w < 0.5f ? fmaf(w, diff, start) : fmaf(w - 1.0f, diff, end);
}

template <bool CENTERED, bool MOMENTUM>
__device__ __forceinline__ void rmsprop_elem(float& p, float g, float* state, const Clip& clip,
                                             float lr, const StepArgs& a) {
  // state: [0] square_avg, then grad_avg (centred), then momentum_buffer
  const float d = decayed(g, p, clip, a.weight_decay);
  // sq.mul_(alpha).addcmul_(d, d, value=1 - alpha)
  const float sq = fmaf(a.alpha_rest * d, d, a.alpha * state[0]);
  state[0] = sq;
  float avg;
  if (CENTERED) {
    const float ga = lerp_like_torch(state[1], d, a.alpha_rest);
    state[1] = ga;
    avg = sqrtf(fmaf(-ga, ga, sq));  // sq.addcmul(ga, ga, value=-1).sqrt_()
  } else {
    avg = sqrtf(sq);
  }
  avg = avg + a.eps;
  if (MOMENTUM) {
    constexpr int kBuf = CENTERED ? 2 : 1;
    const float buf = a.momentum * state[kBuf] + d / avg;  // buf.mul_(mu).addcdiv_(d, avg)
    state[kBuf] = buf;
    p = fmaf(-lr, buf, p);  // p.add_(buf, alpha=-lr)
  } else {
    p = p + (-lr * d) / avg;  // p.addcdiv_(d, avg, value=-lr)
  }
}

// Applies `elem(p, g, state[], ...)` to every element of the block's chunk.  NS streams:
// 0 param, 1 grad, 2.. state.
template <int NS, typename F>
__device__ __forceinline__ void step_chunk(const OptimTable& table, const StepArgs& a,
                                           const int (&rows)[NS], F elem) {
  const Clip clip = clip_of(a);
  const float lr = a.lr[0];
  const Chunk<NS> c = chunk_of<NS>(table, rows);
  float4 raw[NS][kLoads];
  load_chunk<NS>(c, raw);
#pragma unroll
  for (int i = 0; i < kLoads; ++i) {
    float v[NS][4];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
      v[s][0] = raw[s][i].x; v[s][1] = raw[s][i].y; v[s][2] = raw[s][i].z; v[s][3] = raw[s][i].w;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      float state[NS > 2 ? NS - 2 : 1];
#pragma unroll
      for (int s = 2; s < NS; ++s) state[s - 2] = v[s][k];
      elem(v[0][k], v[1][k], state, clip, lr, a);
#pragma unroll
      for (int s = 2; s < NS; ++s) v[s][k] = state[s - 2];
    }
#pragma unroll
    for (int s = 0; s < NS; ++s) raw[s][i] = make_float4(v[s][0], v[s][1], v[s][2], v[s][3]);
  }
  store_chunk<NS>(c, raw);
}

template <bool MOMENTUM>
__global__ __launch_bounds__(kThreads) void sgd_step_kernel(OptimTable table, StepArgs a) {
  constexpr int NS = MOMENTUM ? 3 : 2;
  int rows[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) rows[s] = s;
  step_chunk<NS>(table, a, rows,
                 [](float& p, float g, float* state, const Clip& clip, float lr,
                    const StepArgs& args) {
                   SgdOp::apply<MOMENTUM>(p, g, state, clip, lr, args);
                 });
}

// Table rows: 0 param, 1 grad, 2 square_avg, 3 grad_avg, 4 momentum_buffer.
template <bool CENTERED, bool MOMENTUM>
__global__ __launch_bounds__(kThreads) void rmsprop_step_kernel(OptimTable table, StepArgs a) {
  constexpr int NS = 3 + (CENTERED ? 1 : 0) + (MOMENTUM ? 1 : 0);
  int rows[NS];
  rows[0] = 0; rows[1] = 1; rows[2] = 2;
  if constexpr (CENTERED) rows[3] = 3;
  if constexpr (MOMENTUM) rows[NS - 1] = 4;
  step_chunk<NS>(table, a, rows,
                 [](float& p, float g, float* state, const Clip& clip, float lr,
                    const StepArgs& args) {
                   rmsprop_elem<CENTERED, MOMENTUM>(p, g, state, clip, lr, args);
                 });
}

// Calls launch(table, blocks) for each table's worth of `spans`.
template <typename F>
void for_each_table(const OptimSpan* spans, int count, F launch) {
  OptimTable table{};
  int64_t chunks = 0;
  auto flush = [&]() {
    if (table.count == 0) return;
    table.first[table.count] = static_cast<int32_t>(chunks);
    launch(table, static_cast<unsigned>(chunks));
    table = OptimTable{};
    chunks = 0;
  };
  for (int i = 0; i < count; ++i) {
    if (spans[i].numel <= 0) continue;
    const int64_t n = (spans[i].numel + kChunk - 1) / kChunk;
    if (table.count == kOptimTensors || chunks + n > kMaxChunks) flush();
    for (int s = 0; s < kOptimStreams; ++s) table.ptr[s][table.count] = spans[i].ptr[s];
    table.first[table.count] = static_cast<int32_t>(chunks);
    table.last[table.count] = static_cast<int32_t>(spans[i].numel - (n - 1) * kChunk);
    ++table.count;
    chunks += n;
  }
  flush();
}

StepArgs common_args(const float* lr, const double* sumsq, double max_norm, double clip_eps,
                     double momentum, double weight_decay) {
  StepArgs a{};
  a.lr = lr;
  a.sumsq = sumsq;
  a.max_norm = max_norm;
  a.clip_eps = clip_eps;
  a.momentum = static_cast<float>(momentum);
  a.weight_decay = static_cast<float>(weight_decay);
  return a;
}

}  // namespace

void launch_sgd_step(const OptimSpan* spans, int count, const float* lr, double momentum,
                     double dampening, bool nesterov, double weight_decay, bool first,
                     const double* sumsq, double max_norm, double clip_eps, hipStream_t stream) {
  StepArgs a = common_args(lr, sumsq, max_norm, clip_eps, momentum, weight_decay);
  a.damp_rest = static_cast<float>(1.0 - dampening);
  a.nesterov = nesterov ? 1 : 0;
  a.first = first ? 1 : 0;
  for_each_table(spans, count, [&](const OptimTable& table, unsigned grid) {
    if (momentum != 0.0) {
      hipLaunchKernelGGL(sgd_step_kernel<true>, dim3(grid), dim3(kThreads), 0, stream, table, a);
    } else {
      hipLaunchKernelGGL(sgd_step_kernel<false>, dim3(grid), dim3(kThreads), 0, stream, table, a);
    }
  });
}

void launch_rmsprop_step(const OptimSpan* spans, int count, const float* lr, double alpha,
                         double eps, double weight_decay, double momentum, bool centered,
                         const double* sumsq, double max_norm, double clip_eps,
                         hipStream_t stream) {
  StepArgs a = common_args(lr, sumsq, max_norm, clip_eps, momentum, weight_decay);
  a.alpha = static_cast<float>(alpha);
  a.alpha_rest = static_cast<float>(1.0 - alpha);
  a.eps = static_cast<float>(eps);
  const bool mom = momentum > 0.0;
  for_each_table(spans, count, [&](const OptimTable& table, unsigned grid) {
    const dim3 g(grid), b(kThreads);
    if (centered && mom) {
      hipLaunchKernelGGL((rmsprop_step_kernel<true, true>), g, b, 0, stream, table, a);
    } else if (centered) {
      hipLaunchKernelGGL((rmsprop_step_kernel<true, false>), g, b, 0, stream, table, a);
    } else if (mom) {
      hipLaunchKernelGGL((rmsprop_step_kernel<false, true>), g, b, 0, stream, table, a);
    } else {
      hipLaunchKernelGGL((rmsprop_step_kernel<false, false>), g, b, 0, stream, table, a);
    }
  });
}

}  // namespace tgpipe
