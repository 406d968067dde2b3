// Checks and pointer helpers shared by the ATen bindings (bindings.cpp, convbn.cpp) for the
// dtype-following ops: DropNormAct, up2x_cat, maxpool2x2 take fp32 or bf16, every operand of
// one call alike.
#pragma once
#include <torch/extension.h>

#include "kernels.h"

namespace tgpipe {

// `t`: a contiguous GPU tensor, fp32 or bf16, of the dtype (and device) of the op's first
// operand `like`; at most `max_elems` elements where the caller's kernels have a limit.
inline void check_f32_or_bf16(const at::Tensor& t, const char* name, const at::Tensor& like,
                              int64_t max_elems = 0) {
  TORCH_CHECK(t.is_cuda() && t.device() == like.device(), name, " must be on ", like.device());
  TORCH_CHECK(t.scalar_type() == at::kFloat || t.scalar_type() == at::kBFloat16, name,
              " must be float32 or bfloat16");
  TORCH_CHECK(t.scalar_type() == like.scalar_type(), name, " must have the dtype of the op's "
              "other operands (", like.scalar_type(), ")");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(max_elems <= 0 || t.numel() <= max_elems, name,
              " is too large (< 2 GiB per tensor)");
}

inline const bf16_bits* bf16_ptr(const at::Tensor& t) {
  return reinterpret_cast<const bf16_bits*>(t.data_ptr<at::BFloat16>());
}
inline bf16_bits* bf16_mut(at::Tensor& t) {
  return reinterpret_cast<bf16_bits*>(t.data_ptr<at::BFloat16>());
}

}  // namespace tgpipe
