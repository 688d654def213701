// Host-side argument checks shared by the op wrappers.
#pragma once
#include <torch/extension.h>

// optional int64[1] live row count on the operand's device -> pointer
// (nullptr when absent or undefined).  `op` prefixes the error text.
static inline const int64_t* n_live_ptr(
    const c10::optional<at::Tensor>& n_dev, const at::Tensor& like,
    const char* op) {
  if (!n_dev.has_value() || !n_dev->defined()) return nullptr;
  TORCH_CHECK(n_dev->is_cuda() && n_dev->device() == like.device() &&
                  n_dev->numel() == 1 && n_dev->scalar_type() == at::kLong,
              op, ": n_dev must be an int64[1] tensor on the operand's device");
  return n_dev->data_ptr<int64_t>();
}
