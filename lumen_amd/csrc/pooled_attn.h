// Pooled-query attention over the residual stream (pooled_attn.hip) shared with its torch binding (ops.cpp).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace lumen {

struct PooledAttnArgs {
  const uint16_t* x; int64_t ldx;   // residual rows [B*S, W] bf16, row stride in elements
  const float* st;                  // [B*S, 2] fp32 (rstd, -mean * rstd)
  const uint16_t* g;                // [B, H, W] bf16: the query through the LN-folded K weights
  const float* s;                   // [B, H] fp32: row sums of g
  const int* kv_len;                // optional per-sequence key count
  uint16_t* z;                      // [B*H, W] bf16
  float* c;                         // [B*H] fp32
  int S, W, H;
};

hipError_t pooled_attn_x(const PooledAttnArgs& a, int B, hipStream_t stream);

}  // namespace lumen
