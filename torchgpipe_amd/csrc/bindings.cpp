// ATen bindings: registers the framework kernels as torch.ops.tgpipe.* (CUDA == HIP
// dispatch key on ROCm builds) and validates shapes / dtypes / devices before launching.
#include <algorithm>
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>
#include <ATen/hip/impl/HIPGuardImplMasqueradingAsCUDA.h>

#include <vector>

#include "aten_checks.h"
#include "kernels.h"

namespace tgpipe {
namespace {

hipStream_t stream_of(const at::Tensor& t) {
  return at::hip::getCurrentHIPStream(t.device().index()).stream();
}

// Optional device-resident Philox state: int64 [2] (seed, base offset) on the op's device.
const int64_t* rng_state(const c10::optional<at::Tensor>& rng, const at::Device& device) {
  if (!rng.has_value() || !rng->defined()) return nullptr;
  TORCH_CHECK(rng->is_cuda() && rng->device() == device && rng->scalar_type() == at::kLong &&
                  rng->is_contiguous() && rng->numel() == 2,
              "rng must be a contiguous int64 [2] (seed, offset) tensor on the op's device");
  return rng->data_ptr<int64_t>();
}

void check_f32_gpu(const at::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a GPU tensor");
  TORCH_CHECK(t.scalar_type() == at::kFloat, name, " must be float32");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

std::vector<at::Tensor> dna_forward(const at::Tensor& x, double p, double eps, double slope,
                                    int64_t seed, int64_t offset, bool dropout,
                                    const c10::optional<at::Tensor>& rng) {
  check_f32_or_bf16(x, "x", x);
  TORCH_CHECK(x.dim() >= 3, "expected (N, C, *spatial) input");
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout probability must be in [0, 1)");
  const int64_t planes = x.size(0) * x.size(1);
  const int64_t s = planes == 0 ? 0 : x.numel() / planes;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  auto y = at::empty_like(x);
  auto opts = x.options().dtype(at::kFloat);  // the saved statistics stay fp32
  auto mean = at::empty({planes}, opts);
  auto rstd = at::empty({planes}, opts);
  auto scale = at::empty({planes}, opts);
  if (x.scalar_type() == at::kBFloat16) {
    launch_dna_forward(bf16_ptr(x), bf16_mut(y), mean.data_ptr<float>(), rstd.data_ptr<float>(),
                       scale.data_ptr<float>(), planes, s, static_cast<float>(p),
                       static_cast<float>(eps), static_cast<float>(slope),
                       static_cast<uint64_t>(seed), static_cast<uint64_t>(offset), dropout,
                       rng_state(rng, x.device()), stream_of(x));
    return {y, mean, rstd, scale};
  }
  launch_dna_forward(x.data_ptr<float>(), y.data_ptr<float>(), mean.data_ptr<float>(),
                     rstd.data_ptr<float>(), scale.data_ptr<float>(), planes, s,
                     static_cast<float>(p), static_cast<float>(eps), static_cast<float>(slope),
                     static_cast<uint64_t>(seed), static_cast<uint64_t>(offset), dropout,
                     rng_state(rng, x.device()), stream_of(x));
  return {y, mean, rstd, scale};
}

at::Tensor dna_backward(const at::Tensor& dy_in, const at::Tensor& x, const at::Tensor& mean,
                        const at::Tensor& rstd, const at::Tensor& scale, double slope) {
  check_f32_or_bf16(x, "x", x);
  auto dy = dy_in.contiguous();
  check_f32_or_bf16(dy, "dy", x);
  TORCH_CHECK(dy.sizes() == x.sizes(), "dy and x must have the same shape");
  const int64_t planes = x.size(0) * x.size(1);
  const int64_t s = planes == 0 ? 0 : x.numel() / planes;
  TORCH_CHECK(mean.numel() == planes && rstd.numel() == planes && scale.numel() == planes,
              "saved statistics must have N*C elements");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  auto dx = at::empty_like(x);
  if (x.scalar_type() == at::kBFloat16) {
    launch_dna_backward(bf16_ptr(dy), bf16_ptr(x), mean.data_ptr<float>(),
                        rstd.data_ptr<float>(), scale.data_ptr<float>(), bf16_mut(dx), planes, s,
                        static_cast<float>(slope), stream_of(x));
    return dx;
  }
  launch_dna_backward(dy.data_ptr<float>(), x.data_ptr<float>(), mean.data_ptr<float>(),
                      rstd.data_ptr<float>(), scale.data_ptr<float>(), dx.data_ptr<float>(),
                      planes, s, static_cast<float>(slope), stream_of(x));
  return dx;
}

// The DropNormAct instance a plane of `s` elements of `elem_bytes` runs, its operands'
// addresses off slot alignment by `misalign` bytes: (GROUP, V, form) -- host only.
std::vector<int64_t> dna_plan_info(int64_t s, int64_t elem_bytes, int64_t misalign) {
  TORCH_CHECK(elem_bytes == 4 || elem_bytes == 2, "elem_bytes must be 4 (fp32) or 2 (bf16)");
  int64_t out[3];
  dna_plan(s, static_cast<int>(elem_bytes), static_cast<uintptr_t>(misalign), out);
  return {out[0], out[1], out[2]};
}

at::Tensor dropout(const at::Tensor& x_in, double p, int64_t seed, int64_t offset,
                   const c10::optional<at::Tensor>& rng) {
  auto x = x_in.contiguous();
  check_f32_gpu(x, "x");
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout probability must be in [0, 1)");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  auto y = at::empty_like(x);
  launch_dropout(x.data_ptr<float>(), y.data_ptr<float>(), x.numel(), static_cast<float>(p),
                 static_cast<uint64_t>(seed), static_cast<uint64_t>(offset),
                 rng_state(rng, x.device()), stream_of(x));
  return y;
}

at::Tensor philox_uniform(int64_t n, int64_t seed, int64_t offset, at::Device device,
                          const c10::optional<at::Tensor>& rng) {
  TORCH_CHECK(device.is_cuda(), "philox_uniform runs on the GPU");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(device);
  auto out = at::empty({n}, at::TensorOptions().dtype(at::kFloat).device(device));
  launch_philox_uniform(out.data_ptr<float>(), n, static_cast<uint64_t>(seed),
                        static_cast<uint64_t>(offset), rng_state(rng, out.device()),
                        stream_of(out));
  return out;
}

void spin(int64_t ns, at::Device device) {
  TORCH_CHECK(device.is_cuda(), "spin runs on the GPU");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(device);
  launch_spin(static_cast<uint64_t>(ns),
              at::hip::getCurrentHIPStream(device.index()).stream());
}

void copy_segments(at::TensorList srcs, at::TensorList dsts) {
  TORCH_CHECK(srcs.size() == dsts.size(), "srcs and dsts must pair up");
  if (srcs.empty()) return;
  const auto device = srcs[0].device();
  TORCH_CHECK(device.is_cuda(), "copy_segments runs on the GPU");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(device);
  std::vector<Segment> segs;
  for (size_t i = 0; i < srcs.size(); ++i) {
    TORCH_CHECK(srcs[i].is_contiguous() && dsts[i].is_contiguous(), "segments must be contiguous");
    TORCH_CHECK(srcs[i].device() == device && dsts[i].device() == device,
                "segments must live on one device");
    const int64_t bytes = srcs[i].numel() * srcs[i].element_size();
    TORCH_CHECK(bytes == dsts[i].numel() * dsts[i].element_size(), "segment size mismatch");
    segs.push_back({srcs[i].data_ptr(), dsts[i].data_ptr(), bytes});
  }
  const hipStream_t stream = at::hip::getCurrentHIPStream(device.index()).stream();
  for (size_t i = 0; i < segs.size(); i += kMaxSegments) {
    const int count = static_cast<int>(std::min<size_t>(kMaxSegments, segs.size() - i));
    launch_segments_copy(segs.data() + i, count, stream);
  }
}

// copy_segments with a mode per segment (kernels.h WireMode): 0 copies bytes, 1 rounds an
// fp32 source into a destination of 2 bytes per element, 2 widens such a source into an
// fp32 destination.  The bf16 side may be a byte view (a slice of a wire buffer).
void wire_segments(at::TensorList srcs, at::TensorList dsts, at::IntArrayRef modes) {
  TORCH_CHECK(srcs.size() == dsts.size() && srcs.size() == modes.size(),
              "srcs, dsts and modes must pair up");
  if (srcs.empty()) return;
  const auto device = srcs[0].device();
  TORCH_CHECK(device.is_cuda(), "wire_segments runs on the GPU");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(device);
  std::vector<WireSegment> segs;
  for (size_t i = 0; i < srcs.size(); ++i) {
    const at::Tensor& s = srcs[i];
    const at::Tensor& d = dsts[i];
    TORCH_CHECK(s.is_contiguous() && d.is_contiguous(), "segments must be contiguous");
    TORCH_CHECK(s.device() == device && d.device() == device,
                "segments must live on one device");
    const int64_t sbytes = s.numel() * s.element_size();
    const int64_t dbytes = d.numel() * d.element_size();
    const auto sp = reinterpret_cast<uintptr_t>(s.data_ptr());
    const auto dp = reinterpret_cast<uintptr_t>(d.data_ptr());
    int64_t count = 0;
    switch (modes[i]) {
      case kWireCopy:
        TORCH_CHECK(sbytes == dbytes, "segment ", i, ": size mismatch");
        count = sbytes;
        break;
      case kWireEncode:
        TORCH_CHECK(s.scalar_type() == at::kFloat, "segment ", i, ": encode takes float32");
        TORCH_CHECK(dbytes == 2 * s.numel(), "segment ", i,
                    ": the destination of an encode holds 2 bytes per element");
        TORCH_CHECK(dp % 2 == 0, "segment ", i, ": bf16 destination must be 2-byte aligned");
        count = s.numel();
        break;
      case kWireDecode:
        TORCH_CHECK(d.scalar_type() == at::kFloat, "segment ", i, ": decode writes float32");
        TORCH_CHECK(sbytes == 2 * d.numel(), "segment ", i,
                    ": the source of a decode holds 2 bytes per element");
        TORCH_CHECK(sp % 2 == 0, "segment ", i, ": bf16 source must be 2-byte aligned");
        count = d.numel();
        break;
      default:
        TORCH_CHECK(false, "segment ", i, ": unknown wire mode ", modes[i]);
    }
    if (count == 0) continue;  // empty tensors launch nothing
    segs.push_back({s.data_ptr(), d.data_ptr(), count, static_cast<int>(modes[i])});
  }
  const hipStream_t stream = at::hip::getCurrentHIPStream(device.index()).stream();
  for (size_t i = 0; i < segs.size(); i += kMaxSegments) {
    const int count = static_cast<int>(std::min<size_t>(kMaxSegments, segs.size() - i));
    launch_wire_segments(segs.data() + i, count, stream);
  }
}

// The dense tensors of one dtype (fp32 or bf16) on one GPU that the gradient-clipping
// kernels take, as spans; empty tensors are left out.  Returns the element size.
int grad_spans(at::TensorList grads, const char* op, std::vector<GradSpan>& spans) {
  int elem_bytes = 0;
  const at::Tensor* like = nullptr;
  for (const at::Tensor& g : grads) {
    TORCH_CHECK(g.defined() && g.is_cuda(), op, " takes GPU tensors");
    TORCH_CHECK(g.layout() == at::kStrided && g.is_non_overlapping_and_dense(), op,
                " takes dense tensors");
    TORCH_CHECK(g.scalar_type() == at::kFloat || g.scalar_type() == at::kBFloat16, op,
                " takes float32 or bfloat16 tensors");
    if (like == nullptr) like = &g;
    TORCH_CHECK(g.device() == like->device() && g.scalar_type() == like->scalar_type(), op,
                " takes tensors of one device and one dtype");
    elem_bytes = static_cast<int>(g.element_size());
    if (g.numel() > 0) spans.push_back({g.data_ptr(), g.numel()});
  }
  return elem_bytes;
}

void check_launched(const char* op) {
  const hipError_t err = hipGetLastError();
  TORCH_CHECK(err == hipSuccess, op, " failed to launch: ", hipGetErrorString(err));
}

at::Tensor grad_sumsq(at::TensorList grads) {
  std::vector<GradSpan> spans;
  const int elem_bytes = grad_spans(grads, "grad_sumsq", spans);
  auto opts = at::TensorOptions().dtype(at::kDouble);
  if (grads.empty()) return at::zeros({1}, opts.device(at::kCUDA));
  const auto device = grads[0].device();
  c10::hip::HIPGuardMasqueradingAsCUDA guard(device);
  if (spans.empty()) return at::zeros({1}, opts.device(device));
  const int count = static_cast<int>(spans.size());
  // at::empty: the caching allocator's blocks are safe to take and drop under graph capture
  auto partials = at::empty({grad_clip_blocks(spans.data(), count, elem_bytes)},
                            opts.device(device));
  auto out = at::empty({1}, opts.device(device));
  launch_grad_sumsq(spans.data(), count, elem_bytes, partials.data_ptr<double>(),
                    out.data_ptr<double>(), at::hip::getCurrentHIPStream(device.index()).stream());
  check_launched("grad_sumsq");
  return out;
}

void grad_scale_(at::TensorList grads, const at::Tensor& sumsq, double max_norm, double eps) {
  std::vector<GradSpan> spans;
  const int elem_bytes = grad_spans(grads, "grad_scale_", spans);
  if (spans.empty()) return;
  const auto device = grads[0].device();
  TORCH_CHECK(sumsq.is_cuda() && sumsq.device() == device && sumsq.scalar_type() == at::kDouble &&
                  sumsq.numel() >= 1,
              "sumsq must be a float64 tensor on the gradients' device");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(device);
  launch_grad_scale(spans.data(), static_cast<int>(spans.size()), elem_bytes,
                    sumsq.data_ptr<double>(), max_norm, eps,
                    at::hip::getCurrentHIPStream(device.index()).stream());
  check_launched("grad_scale_");
}

// (chunk elements fp32, chunk elements bf16, tensors per launch, threads per block)
std::vector<int64_t> grad_clip_info() {
  return {kGradClipChunkF32, kGradClipChunkBF16, kGradClipTensors, kGradClipThreads};
}

// The lists of a fused optimizer step (optim.hip) as spans: `lists[0]` the parameters,
// `lists[1]` the gradients, the others state tensors; `rows[l]` is list l's pointer slot in
// OptimSpan.  grad_spans' conditions -- GPU, dense, one device -- with fp32 only, and per
// position one numel and one memory layout, since the kernels walk storage order.  Empty
// tensors are left out.
void optim_spans(const std::vector<at::TensorList>& lists, const std::vector<int>& rows,
                 const char* op, std::vector<OptimSpan>& spans) {
  const at::TensorList params = lists[0];
  for (const at::TensorList& list : lists)
    TORCH_CHECK(list.size() == params.size(), op, " takes lists of one length");
  for (size_t i = 0; i < params.size(); ++i) {
    const at::Tensor& p = params[i];
    OptimSpan span{};
    for (size_t l = 0; l < lists.size(); ++l) {
      const at::Tensor& t = lists[l][i];
      TORCH_CHECK(t.defined() && t.is_cuda(), op, " takes GPU tensors");
      TORCH_CHECK(t.layout() == at::kStrided && t.is_non_overlapping_and_dense(), op,
                  " takes dense tensors");
      TORCH_CHECK(t.scalar_type() == at::kFloat, op, " takes float32 tensors");
      TORCH_CHECK(t.device() == params[0].device(), op, " takes tensors of one device");
      TORCH_CHECK(t.numel() == p.numel(), op, " takes tensors of equal numel per position");
      TORCH_CHECK(t.strides() == p.strides() || t.numel() <= 1, op,
                  " takes tensors of one memory layout per position");
      span.ptr[rows[l]] = t.data_ptr<float>();
    }
    span.numel = p.numel();
    if (span.numel > 0) spans.push_back(span);
  }
}

// The device scalars of a step: the fp32 learning rate and the optional fp64 sum of squares.
const float* optim_lr(const at::Tensor& lr, const at::Device& device, const char* op) {
  TORCH_CHECK(lr.is_cuda() && lr.device() == device && lr.scalar_type() == at::kFloat &&
                  lr.numel() == 1,
              op, ": lr must be a float32 scalar tensor on the parameters' device");
  return lr.data_ptr<float>();
}

const double* optim_sumsq(const c10::optional<at::Tensor>& sumsq, const at::Device& device,
                          const char* op) {
  if (!sumsq.has_value() || !sumsq->defined()) return nullptr;
  TORCH_CHECK(sumsq->is_cuda() && sumsq->device() == device &&
                  sumsq->scalar_type() == at::kDouble && sumsq->numel() >= 1,
              op, ": sumsq must be a float64 tensor on the parameters' device");
  return sumsq->data_ptr<double>();
}

// The custom-op schema's (a!) does not advance the version counter, and ops/conv.py,
// ops/convbn.py and convbn.cpp key their weight caches on it.
void bump_versions(at::TensorList tensors) {
  for (const at::Tensor& t : tensors)
    if (!t.is_inference()) t.unsafeGetTensorImpl()->bump_version();
}

void sgd_step_(at::TensorList params, at::TensorList grads, at::TensorList bufs,
               const at::Tensor& lr, double momentum, double dampening, bool nesterov,
               double weight_decay, bool first, const c10::optional<at::Tensor>& sumsq,
               double max_norm, double clip_eps) {
  TORCH_CHECK(momentum != 0.0 || bufs.empty(), "sgd_step_ takes no buffers without momentum");
  std::vector<at::TensorList> lists = {params, grads};
  if (momentum != 0.0) lists.push_back(bufs);
  std::vector<OptimSpan> spans;
  optim_spans(lists, {0, 1, 2}, "sgd_step_", spans);
  if (params.empty()) return;
  const auto device = params[0].device();
  const float* lr_ptr = optim_lr(lr, device, "sgd_step_");
  const double* sumsq_ptr = optim_sumsq(sumsq, device, "sgd_step_");
  if (spans.empty()) return;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(device);
  launch_sgd_step(spans.data(), static_cast<int>(spans.size()), lr_ptr, momentum, dampening,
                  nesterov, weight_decay, first, sumsq_ptr, max_norm, clip_eps,
                  at::hip::getCurrentHIPStream(device.index()).stream());
  check_launched("sgd_step_");
  bump_versions(params);
  if (momentum != 0.0) bump_versions(bufs);
}

void rmsprop_step_(at::TensorList params, at::TensorList grads, at::TensorList square_avgs,
                   at::TensorList grad_avgs, at::TensorList bufs, const at::Tensor& lr,
                   double alpha, double eps, double weight_decay, double momentum, bool centered,
                   const c10::optional<at::Tensor>& sumsq, double max_norm, double clip_eps) {
  TORCH_CHECK(centered || grad_avgs.empty(), "rmsprop_step_ takes grad_avgs only when centered");
  TORCH_CHECK(momentum > 0.0 || bufs.empty(), "rmsprop_step_ takes no buffers without momentum");
  std::vector<at::TensorList> lists = {params, grads, square_avgs};
  std::vector<int> rows = {0, 1, 2};
  if (centered) { lists.push_back(grad_avgs); rows.push_back(3); }
  if (momentum > 0.0) { lists.push_back(bufs); rows.push_back(4); }
  std::vector<OptimSpan> spans;
  optim_spans(lists, rows, "rmsprop_step_", spans);
  if (params.empty()) return;
  const auto device = params[0].device();
  const float* lr_ptr = optim_lr(lr, device, "rmsprop_step_");
  const double* sumsq_ptr = optim_sumsq(sumsq, device, "rmsprop_step_");
  if (spans.empty()) return;
  c10::hip::HIPGuardMasqueradingAsCUDA guard(device);
  launch_rmsprop_step(spans.data(), static_cast<int>(spans.size()), lr_ptr, alpha, eps,
                      weight_decay, momentum, centered, sumsq_ptr, max_norm, clip_eps,
                      at::hip::getCurrentHIPStream(device.index()).stream());
  check_launched("rmsprop_step_");
  bump_versions(params);
  bump_versions(square_avgs);
  if (centered) bump_versions(grad_avgs);
  if (momentum > 0.0) bump_versions(bufs);
}

// (chunk elements, tensors per launch, threads per block)
std::vector<int64_t> optim_info() {
  return {kOptimChunk, kOptimTensors, kOptimThreads};
}

// `out` (optional): an existing transform of the same shape to overwrite in place (the
// per-step cache refresh, ops/conv.py) instead of a new tensor plus a copy.
at::Tensor transform_out(const c10::optional<at::Tensor>& out, at::IntArrayRef shape,
                         const at::Tensor& like) {
  if (!out.has_value() || !out->defined()) return at::empty(shape, like.options());
  check_f32_gpu(*out, "out");
  TORCH_CHECK(out->sizes() == shape && out->device() == like.device(),
              "out must be the transform's shape on the weight's device");
  return *out;
}

at::Tensor wino_weight(const at::Tensor& w, bool flip, const c10::optional<at::Tensor>& out) {
  check_f32_gpu(w, "weight");
  TORCH_CHECK(w.dim() == 4 && w.size(2) == 3 && w.size(3) == 3, "weight must be [K][C][3][3]");
  const int64_t out_channels = flip ? w.size(1) : w.size(0);
  const int64_t red_channels = flip ? w.size(0) : w.size(1);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(w.device());
  auto u = transform_out(
      out, {wino_pad_reduction(red_channels), wino_pad_output(out_channels), 16}, w);
  launch_wino_weight(w.data_ptr<float>(), u.data_ptr<float>(), out_channels, red_channels, flip,
                     stream_of(w));
  return u;
}

at::Tensor wino_conv(const at::Tensor& x_in, const at::Tensor& u,
                     const c10::optional<at::Tensor>& bias, int64_t out_channels,
                     int64_t variant, int64_t splits) {
  auto x = x_in.contiguous();
  check_f32_gpu(x, "x");
  check_f32_gpu(u, "u");
  TORCH_CHECK(x.dim() == 4, "x must be NCHW");
  const int64_t n = x.size(0), r = x.size(1), h = x.size(2), w = x.size(3);
  TORCH_CHECK(u.dim() == 3 && u.size(2) == 16 && u.size(0) == wino_pad_reduction(r) &&
                  u.size(1) == wino_pad_output(out_channels),
              "transformed weight does not match the input/output channels");
  TORCH_CHECK(u.device() == x.device(), "u must live on the input's device");
  TORCH_CHECK(n * ((h + 1) / 2) * ((w + 1) / 2) < (int64_t{1} << 31) * 32,
              "too many output tiles for one launch");
  TORCH_CHECK(r * h * w < (int64_t{1} << 31) && out_channels < (1 << 24),
              "plane too large for 32-bit channel offsets");
  const float* bptr = nullptr;
  if (bias.has_value() && bias->defined()) {
    check_f32_gpu(*bias, "bias");
    TORCH_CHECK(bias->numel() == out_channels, "bias must have K elements");
    bptr = bias->data_ptr<float>();
  }
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  TORCH_CHECK(variant >= -1 && variant <= 2, "variant must be -1 (auto), 0, 1 or 2");
  auto y = at::empty({n, out_channels, h, w}, x.options());
  if (y.numel() == 0) return y;
  const WinoPlan plan = wino_plan(n, r, h, w, out_channels, static_cast<int>(variant),
                                  static_cast<int>(splits));
  at::Tensor ws;
  if (plan.workspace > 0) ws = at::empty({plan.workspace}, x.options());
  launch_wino_conv(x.data_ptr<float>(), u.data_ptr<float>(), bptr, y.data_ptr<float>(),
                   plan.workspace > 0 ? ws.data_ptr<float>() : nullptr, n, r, h, w, out_channels,
                   plan, stream_of(x));
  return y;
}

at::Tensor wino4_weight(const at::Tensor& w, bool flip, const c10::optional<at::Tensor>& out) {
  check_f32_gpu(w, "weight");
  TORCH_CHECK(w.dim() == 4 && w.size(2) == 3 && w.size(3) == 3, "weight must be [K][C][3][3]");
  const int64_t out_channels = flip ? w.size(1) : w.size(0);
  const int64_t red_channels = flip ? w.size(0) : w.size(1);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(w.device());
  auto u = transform_out(
      out, {wino4_pad_reduction(red_channels), wino4_pad_output(out_channels), 36}, w);
  launch_wino4_weight(w.data_ptr<float>(), u.data_ptr<float>(), out_channels, red_channels, flip,
                      stream_of(w));
  return u;
}

// The weight image of the fused split-bf16 kernel (variant 24): bf16 hi and mid planes of
// U as [Rp/16][Op/64][36 positions][4 KiB], Rp a multiple of 16.
std::vector<int64_t> wino4_emu_weight_shape(int64_t out_channels, int64_t red_channels) {
  return {wino4_emu_pad_reduction(red_channels) / 16, wino4_pad_output(out_channels) / 64, 36,
          1024};
}

at::Tensor wino4_weight_emu(const at::Tensor& w, bool flip,
                            const c10::optional<at::Tensor>& out) {
  check_f32_gpu(w, "weight");
  TORCH_CHECK(w.dim() == 4 && w.size(2) == 3 && w.size(3) == 3, "weight must be [K][C][3][3]");
  const int64_t out_channels = flip ? w.size(1) : w.size(0);
  const int64_t red_channels = flip ? w.size(0) : w.size(1);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(w.device());
  const auto wc = w.contiguous();
  auto u = transform_out(out, wino4_emu_weight_shape(out_channels, red_channels), w);
  TORCH_CHECK(u.is_contiguous(), "out must be contiguous");
  if (u.numel() == 0) return u;
  launch_wino4_emu_weight(wc.data_ptr<float>(), u.data_ptr<float>(), out_channels, red_channels,
                          flip, stream_of(w));
  return u;
}

at::Tensor wino4_conv(const at::Tensor& x_in, const at::Tensor& u,
                      const c10::optional<at::Tensor>& bias, int64_t out_channels,
                      int64_t variant, int64_t splits) {
  auto x = x_in.contiguous();
  check_f32_gpu(x, "x");
  check_f32_gpu(u, "u");
  TORCH_CHECK(x.dim() == 4, "x must be NCHW");
  const int64_t n = x.size(0), r = x.size(1), h = x.size(2), w = x.size(3);
  if (wino4_variant_emu(static_cast<int>(variant))) {
    // the split-bf16 kernel reads its own image (wino4_weight_emu)
    TORCH_CHECK(u.is_contiguous() && u.sizes() == at::IntArrayRef(wino4_emu_weight_shape(
                                                      out_channels, r)),
                "variant ", variant, " needs the wino4_weight_emu image of these input/output "
                "channels");
  } else {
    // the kernel's 36-float weight rows, channel padding and index ranges
    TORCH_CHECK(u.dim() == 3 && u.size(2) == 36 && u.size(0) == wino4_pad_reduction(r) &&
                    u.size(1) == wino4_pad_output(out_channels),
                "F(4x4) transformed weight does not match the input/output channels");
  }
  TORCH_CHECK(u.device() == x.device(), "u must live on the input's device");
  TORCH_CHECK(wino4_supported(n, r, h, w, out_channels),
              "input too large for the F(4x4) kernel (needs < 1 GiB); use wino_conv");
  const float* bptr = nullptr;
  if (bias.has_value() && bias->defined()) {
    check_f32_gpu(*bias, "bias");
    TORCH_CHECK(bias->numel() == out_channels, "bias must have K elements");
    bptr = bias->data_ptr<float>();
  }
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  auto y = at::empty({n, out_channels, h, w}, x.options());
  if (y.numel() == 0) return y;
  TORCH_CHECK(variant == -1 || wino4_variant_known(static_cast<int>(variant)),
              "variant must be -1, 4-10, 12, 14-18, 20-22 or 24");
  const WinoPlan plan = wino4_plan(n, r, h, w, out_channels, static_cast<int>(variant),
                                   static_cast<int>(splits));
  at::Tensor ws;
  if (plan.workspace > 0) ws = at::empty({plan.workspace}, x.options());
  launch_wino4_conv(x.data_ptr<float>(), u.data_ptr<float>(), bptr, y.data_ptr<float>(),
                    plan.workspace > 0 ? ws.data_ptr<float>() : nullptr, n, r, h, w,
                    out_channels, plan, stream_of(x));
  return y;
}

// Weight-gradient destination: a new tensor, or `into` (an existing .grad, contiguous
// fp32 [K][C][3][3]) that the kernels add into (gradient-accumulation fusion).
at::Tensor wgrad_destination(const c10::optional<at::Tensor>& into, const at::Tensor& x,
                             int64_t k, int64_t c) {
  if (!into.has_value()) return at::empty({k, c, 3, 3}, x.options());
  const at::Tensor& d = *into;
  TORCH_CHECK(d.is_contiguous() && d.scalar_type() == at::kFloat && d.device() == x.device() &&
                  d.dim() == 4 && d.size(0) == k && d.size(1) == c && d.size(2) == 3 &&
                  d.size(3) == 3,
              "into must be a contiguous fp32 [K][C][3][3] tensor on x's device");
  return d;
}

at::Tensor wino_wgrad(const at::Tensor& x_in, const at::Tensor& dy_in, int64_t splits,
                      int64_t variant, const c10::optional<at::Tensor>& into) {
  auto x = x_in.contiguous();
  auto dy = dy_in.contiguous();
  check_f32_gpu(x, "x");
  check_f32_gpu(dy, "dy");
  TORCH_CHECK(x.dim() == 4 && dy.dim() == 4, "x and dy must be NCHW");
  const int64_t n = x.size(0), c = x.size(1), h = x.size(2), w = x.size(3), k = dy.size(1);
  TORCH_CHECK(dy.size(0) == n && dy.size(2) == h && dy.size(3) == w,
              "dy must be [N][K][H][W] of a 3x3/s1/p1 convolution of x");
  TORCH_CHECK(dy.device() == x.device(), "x and dy must share a device");
  TORCH_CHECK(c * h * w < (int64_t{1} << 31) && k * h * w < (int64_t{1} << 31),
              "plane too large for 32-bit channel offsets");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  const bool accum = into.has_value();
  auto dw = wgrad_destination(into, x, k, c);
  if (n == 0 || h == 0 || w == 0) return accum ? dw : dw.zero_();
  TORCH_CHECK(variant == -1 || variant == 0 || variant == 2, "variant must be -1, 0 or 2");
  // auto: the 64 x 64 double-buffered kernel, except for <= 32 output channels where
  // half of its 64-wide k block would idle (benchmarks/wgrad_variants.py).  Variant 2
  // decodes tile indices through a float reciprocal: exact below 2^24 tiles.
  const int64_t tiles = n * ((h + 1) / 2) * ((w + 1) / 2);
  int v = variant >= 0 ? static_cast<int>(variant) : (k <= 32 ? 0 : 2);
  if (v == 2 && tiles >= (int64_t{1} << 24)) v = 0;
  // every split must own >= 1 step of 8 tiles (both variants step 8 tiles)
  const int64_t steps = (tiles + 7) / 8;
  const int s = static_cast<int>(std::min<int64_t>(
      splits > 0 ? splits : wino_wgrad_splits(n, c, k, h, w, v), steps));
  at::Tensor ws;
  if (s > 1) ws = at::empty({s * k * c * 9}, x.options());
  launch_wino_wgrad(x.data_ptr<float>(), dy.data_ptr<float>(), dw.data_ptr<float>(),
                    s > 1 ? ws.data_ptr<float>() : nullptr, n, c, k, h, w, s, v, accum,
                    stream_of(x));
  return dw;
}

at::Tensor wino4_wgrad(const at::Tensor& x_in, const at::Tensor& dy_in, int64_t splits,
                       int64_t variant, const c10::optional<at::Tensor>& into) {
  auto x = x_in.contiguous();
  auto dy = dy_in.contiguous();
  check_f32_gpu(x, "x");
  check_f32_gpu(dy, "dy");
  TORCH_CHECK(x.dim() == 4 && dy.dim() == 4, "x and dy must be NCHW");
  const int64_t n = x.size(0), c = x.size(1), h = x.size(2), w = x.size(3), k = dy.size(1);
  TORCH_CHECK(dy.size(0) == n && dy.size(2) == h && dy.size(3) == w,
              "dy must be [N][K][H][W] of a 3x3/s1/p1 convolution of x");
  TORCH_CHECK(dy.device() == x.device(), "x and dy must share a device");
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  const bool accum = into.has_value();
  auto dw = wgrad_destination(into, x, k, c);
  if (n == 0 || h == 0 || w == 0 || c == 0 || k == 0) return accum ? dw : dw.zero_();
  // 32-bit buffer offsets and tile indices
  TORCH_CHECK(wino4_wgrad_supported(n, c, k, h, w),
              "input too large for the F(4x4) weight-gradient kernel (needs < 1 GiB); "
              "use wino_wgrad");
  TORCH_CHECK(variant >= 0 && variant <= 3,
              "variant must be 0 (fused), 1 (non-fused), 2 (split-bf16 batched GEMM) or 3 (fused, "
              "x rows through LDS)");
  const WinoPlan plan = wino4_wgrad_plan(n, c, k, h, w, static_cast<int>(variant),
                                         static_cast<int>(splits));
  at::Tensor ws;
  if (plan.workspace > 0) ws = at::empty({plan.workspace}, x.options());
  launch_wino4_wgrad(x.data_ptr<float>(), dy.data_ptr<float>(), dw.data_ptr<float>(),
                     plan.workspace > 0 ? ws.data_ptr<float>() : nullptr, n, c, k, h, w, plan,
                     accum, stream_of(x));
  return dw;
}

// Batched-GEMM Winograd F(4x4): weights in the GEMM operand layout (cached per step by
// ops/conv.py), and the convolution (input transform, 36 GEMMs, output transform).
at::Tensor bg_weight(const at::Tensor& w, bool flip, int64_t kind,
                     const c10::optional<at::Tensor>& out, int64_t emu) {
  check_f32_gpu(w, "weight");
  TORCH_CHECK(w.dim() == 4 && w.size(2) == 3 && w.size(3) == 3, "weight must be [K][C][3][3]");
  auto wc = w.contiguous();
  const int64_t out_channels = flip ? w.size(1) : w.size(0);
  const int64_t red_channels = flip ? w.size(0) : w.size(1);
  c10::hip::HIPGuardMasqueradingAsCUDA guard(w.device());
  TORCH_CHECK(kind == 4 || kind == 2, "kind must be 4 (F(4x4)) or 2 (F(2x2))");
  auto a =
      transform_out(out, {bg_weight_numel(out_channels, red_channels, static_cast<int>(kind),
                                          static_cast<int>(emu))}, w);
  launch_bg_weight(wc.data_ptr<float>(), a.data_ptr<float>(), out_channels, red_channels, flip,
                   static_cast<int>(kind), stream_of(w), static_cast<int>(emu));
  return a;
}

at::Tensor bg_conv(const at::Tensor& x_in, const at::Tensor& a,
                   const c10::optional<at::Tensor>& bias, int64_t out_channels, int64_t bn,
                   int64_t splits, int64_t kind, int64_t waves, int64_t sub, int64_t emu,
                   const c10::optional<at::Tensor>& stats) {
  auto x = x_in.contiguous();
  check_f32_gpu(x, "x");
  check_f32_gpu(a, "a");
  TORCH_CHECK(x.dim() == 4, "x must be NCHW");
  const int64_t n = x.size(0), r = x.size(1), h = x.size(2), w = x.size(3);
  TORCH_CHECK(kind == 4 || kind == 2, "kind must be 4 (F(4x4)) or 2 (F(2x2))");
  TORCH_CHECK(a.dim() == 1 && a.numel() == bg_weight_numel(out_channels, r, static_cast<int>(kind),
                                                           static_cast<int>(emu)),
              "batched-GEMM transformed weight does not match the input/output channels");
  TORCH_CHECK(a.device() == x.device(), "a must live on the input's device");
  TORCH_CHECK(wino4_supported(n, r, h, w, out_channels),
              "input too large for the F(4x4) kernels (needs < 1 GiB)");
  const float* bptr = nullptr;
  if (bias.has_value() && bias->defined()) {
    check_f32_gpu(*bias, "bias");
    TORCH_CHECK(bias->numel() == out_channels, "bias must have K elements");
    bptr = bias->data_ptr<float>();
  }
  c10::hip::HIPGuardMasqueradingAsCUDA guard(x.device());
  auto y = at::empty({n, out_channels, h, w}, x.options());
  if (n == 0 || h == 0 || w == 0 || out_channels == 0) return y;
  const BgPlan plan = bg_plan(n, r, h, w, out_channels, static_cast<int>(bn),
                              static_cast<int>(splits), static_cast<int>(kind),
                              static_cast<int>(waves), static_cast<int>(sub),
                              static_cast<int>(emu));
  // 32-bit tile / element indices of the GEMM and transform kernels
  TORCH_CHECK(plan.ksteps * 16 * plan.np < (int64_t{1} << 31) &&
                  plan.mp * plan.np < (int64_t{1} << 31),
              "operands too large for the batched-GEMM kernels");
  // stats: the BatchNorm (mean, M2) partials of y, [2][groups][out_channels] with groups =
  // ceil(n / bg_stats_ipg(n, h, w, kind)) -- the caller's bn_train_forward reads them
  float* pm = nullptr;
  int ipg = 0;
  if (stats.has_value() && stats->defined()) {
    check_f32_gpu(*stats, "stats");
    ipg = bg_stats_ipg(n, h, w, static_cast<int>(kind));
    const int64_t groups = (n + ipg - 1) / ipg;
    TORCH_CHECK(stats->device() == x.device() && stats->is_contiguous() &&
                    stats->numel() == 2 * groups * out_channels,
                "stats must be a contiguous [2][ceil(n / bg_stats_ipg)][K] float32 tensor");
    pm = stats->data_ptr<float>();
  }
  auto ws = at::empty({plan.workspace}, x.options());
  launch_bg_conv(x.data_ptr<float>(), a.data_ptr<float>(), bptr, y.data_ptr<float>(),
                 ws.data_ptr<float>(), n, r, h, w, out_channels, plan, stream_of(x), pm,
                 pm == nullptr ? nullptr : pm + stats->numel() / 2, ipg);
  return y;
}

int64_t bg_stats_images(int64_t n, int64_t h, int64_t w, int64_t kind) {
  return bg_stats_ipg(n, h, w, static_cast<int>(kind));
}

// Split-K count of the F(4x4) kernels for one convolution: variant 0 = the weight gradient,
// otherwise that forward / backward-data variant (wino4_plan).
int64_t wino4_splits(int64_t n, int64_t c, int64_t k, int64_t h, int64_t w, int64_t variant) {
  if (variant == 0) return wino4_wgrad_plan(n, c, k, h, w, 0, 0).splits;
  return wino4_plan(n, c, h, w, k, static_cast<int>(variant), 0).splits;
}

// The host plans as integer lists (no tensors, no device calls; tests/ops/
// test_winograd_plans.py): c = reduction (input) channels, k = output channels.
// [variant that runs, og, splits, workspace floats]
std::vector<int64_t> wino4_plan_info(int64_t n, int64_t c, int64_t k, int64_t h, int64_t w,
                                     int64_t variant, int64_t splits) {
  const WinoPlan p = wino4_plan(n, c, h, w, k, static_cast<int>(variant),
                                static_cast<int>(splits));
  return {p.variant, p.og, p.splits, p.workspace};
}

// [variant that runs, splits, workspace floats]
std::vector<int64_t> wino4_wgrad_plan_info(int64_t n, int64_t c, int64_t k, int64_t h, int64_t w,
                                           int64_t variant, int64_t splits) {
  const WinoPlan p = wino4_wgrad_plan(n, c, k, h, w, static_cast<int>(variant),
                                      static_cast<int>(splits));
  return {p.variant, p.splits, p.workspace};
}

// [kind, emu, waves, bn, sub, splits, ksteps, mp, np, workspace floats]
std::vector<int64_t> bg_plan_info(int64_t n, int64_t c, int64_t k, int64_t h, int64_t w,
                                  int64_t bn, int64_t splits, int64_t kind, int64_t waves,
                                  int64_t sub, int64_t emu) {
  const BgPlan p = bg_plan(n, c, h, w, k, static_cast<int>(bn), static_cast<int>(splits),
                           static_cast<int>(kind), static_cast<int>(waves),
                           static_cast<int>(sub), static_cast<int>(emu));
  return {p.kind, p.emu ? 1 : 0, p.waves, p.bn, p.sub, p.splits, p.ksteps, p.mp, p.np,
          p.workspace};
}

}  // namespace
}  // namespace tgpipe

TORCH_LIBRARY(tgpipe, m) {
  m.def("dna_forward(Tensor x, float p, float eps, float slope, int seed, int offset, "
        "bool dropout, Tensor? rng=None) -> Tensor[]");
  m.def("dna_backward(Tensor dy, Tensor x, Tensor mean, Tensor rstd, Tensor scale, "
        "float slope) -> Tensor");
  // the DropNormAct instance for a plane size, element size and misalignment (host only)
  m.def("dna_plan_info(int s, int elem_bytes, int misalign) -> int[]", &tgpipe::dna_plan_info);
  m.def("dropout(Tensor x, float p, int seed, int offset, Tensor? rng=None) -> Tensor");
  m.def("philox_uniform(int n, int seed, int offset, Device device, Tensor? rng=None) -> Tensor");
  m.def("spin(int ns, Device device) -> ()");
  m.def("copy_segments(Tensor[] srcs, Tensor(a!)[] dsts) -> ()");
  // copy_segments with a mode per segment: 0 copy, 1 fp32 -> bf16 (RNE), 2 bf16 -> fp32
  m.def("wire_segments(Tensor[] srcs, Tensor(a!)[] dsts, int[] modes) -> ()");
  // global-norm gradient clipping: fp64 sum of squares [1], in-place scale reading it
  m.def("grad_sumsq(Tensor[] grads) -> Tensor");
  m.def("grad_scale_(Tensor(a!)[] grads, Tensor sumsq, float max_norm, float eps) -> ()");
  m.def("grad_clip_info() -> int[]", &tgpipe::grad_clip_info);
  // fused optimizer steps: lr is a device fp32 scalar; sumsq (fp64, device) clips in the pass
  m.def("sgd_step_(Tensor(a!)[] params, Tensor[] grads, Tensor(b!)[] bufs, Tensor lr, "
        "float momentum, float dampening, bool nesterov, float weight_decay, bool first, "
        "Tensor? sumsq, float max_norm, float clip_eps) -> ()");
  m.def("rmsprop_step_(Tensor(a!)[] params, Tensor[] grads, Tensor(b!)[] square_avgs, "
        "Tensor(c!)[] grad_avgs, Tensor(d!)[] bufs, Tensor lr, float alpha, float eps, "
        "float weight_decay, float momentum, bool centered, Tensor? sumsq, float max_norm, "
        "float clip_eps) -> ()");
  // [chunk elements, tensors per launch, threads per block]
  m.def("optim_info() -> int[]", &tgpipe::optim_info);
  m.def("wino_weight(Tensor w, bool flip, Tensor? out=None) -> Tensor");
  m.def("wino_wgrad(Tensor x, Tensor dy, int splits=0, int variant=-1, Tensor? into=None) -> Tensor");
  m.def("wino_conv(Tensor x, Tensor u, Tensor? bias, int out_channels, int variant=-1, "
        "int splits=0) -> Tensor");
  m.def("wino4_weight(Tensor w, bool flip, Tensor? out=None) -> Tensor");
  m.def("wino4_weight_emu(Tensor w, bool flip, Tensor? out=None) -> Tensor");
  m.def("wino4_wgrad(Tensor x, Tensor dy, int splits=0, int variant=0, Tensor? into=None) -> Tensor");
  m.def("wino4_conv(Tensor x, Tensor u, Tensor? bias, int out_channels, int variant=-1, "
        "int splits=0) -> Tensor");
  m.def("bg_weight(Tensor w, bool flip, int kind=4, Tensor? out=None, int emu=-1) -> Tensor");
  // split-K counts the F(4x4) host heuristics pick (host only, CPU-testable)
  m.def("wino4_splits(int n, int c, int k, int h, int w, int variant) -> int",
        &tgpipe::wino4_splits);
  m.def("bg_conv(Tensor x, Tensor a, Tensor? bias, int out_channels, int bn=0, int splits=0, "
        "int kind=4, int waves=0, int sub=0, int emu=-1, Tensor(b!)? stats=None) -> Tensor");
  // the F(4x4) / batched-GEMM host plans (host only, CPU-testable)
  m.def("wino4_plan_info(int n, int c, int k, int h, int w, int variant, int splits) -> int[]",
        &tgpipe::wino4_plan_info);
  m.def("wino4_wgrad_plan_info(int n, int c, int k, int h, int w, int variant, int splits) "
        "-> int[]", &tgpipe::wino4_wgrad_plan_info);
  m.def("bg_plan_info(int n, int c, int k, int h, int w, int bn, int splits, int kind, "
        "int waves, int sub, int emu) -> int[]", &tgpipe::bg_plan_info);
  // images per BatchNorm-statistics group of bg_conv's `stats` (host only)
  m.def("bg_stats_images(int n, int h, int w, int kind) -> int", &tgpipe::bg_stats_images);
}

TORCH_LIBRARY_IMPL(tgpipe, CUDA, m) {
  m.impl("dna_forward", &tgpipe::dna_forward);
  m.impl("dna_backward", &tgpipe::dna_backward);
  m.impl("dropout", &tgpipe::dropout);
  m.impl("copy_segments", &tgpipe::copy_segments);
  m.impl("wire_segments", &tgpipe::wire_segments);
  m.impl("grad_scale_", &tgpipe::grad_scale_);
  m.impl("sgd_step_", &tgpipe::sgd_step_);
  m.impl("rmsprop_step_", &tgpipe::rmsprop_step_);
  m.impl("wino_weight", &tgpipe::wino_weight);
  m.impl("wino_conv", &tgpipe::wino_conv);
  m.impl("wino_wgrad", &tgpipe::wino_wgrad);
  m.impl("wino4_weight", &tgpipe::wino4_weight);
  m.impl("wino4_weight_emu", &tgpipe::wino4_weight_emu);
  m.impl("wino4_conv", &tgpipe::wino4_conv);
  m.impl("wino4_wgrad", &tgpipe::wino4_wgrad);
  m.impl("bg_weight", &tgpipe::bg_weight);
  m.impl("bg_conv", &tgpipe::bg_conv);
}

TORCH_LIBRARY_IMPL(tgpipe, CompositeExplicitAutograd, m) {
  m.impl("philox_uniform", &tgpipe::philox_uniform);
  m.impl("spin", &tgpipe::spin);
  m.impl("grad_sumsq", &tgpipe::grad_sumsq);  // an empty list has no dispatch key
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "torchgpipe_amd native HIP kernels (gfx950)";
}
