// The engine keys of the step API's leaf batch (azmi_search_leaf_keys): row r of the batch is entry rows[r] of the step, and the
// find kernel left that entry's key where it hashed the leaf (emit_leaf: ar.leaf_key by tree; a K > 1 step: SbWuArrays::keys by
// entry).  One launch brings them into row order; the row count stays on the device.
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

namespace azmi {

__global__ __launch_bounds__(256) void k_sb_leaf_keys(const uint64_t* key_of, const uint32_t* rows, const uint32_t* n_rows, uint32_t cap, uint64_t* out) {
  const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= cap || r >= *n_rows) return;
  out[r] = key_of[rows[r]];
}

}  // namespace azmi
