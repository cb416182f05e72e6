// Register widening of quantised weights to bf16 MFMA / dot operands, shared by the weight-only
// GEMMs (gemm_w8.hip, gemm_w4.hip) and the quantised grouped expert GEMMs (moe_wq.hip).
#pragma once
#include "common.h"

namespace lumen {

// 16 e4m3fn codes (one 16-byte load, k order) -> two bf16x8 operands (every e4m3 value is exact in bf16)
__device__ __forceinline__ void fp8x16_to_bf16(const u32x4_t w, bf16x8_t& f0, bf16x8_t& f1) {
  f0 = __builtin_bit_cast(bf16x8_t, fp8x8_to_bf16(w[0], w[1]));
  f1 = __builtin_bit_cast(bf16x8_t, fp8x8_to_bf16(w[2], w[3]));
}

// the (scale, wmin) halves of a 4-bit group's fp16 parameter dword
__device__ __forceinline__ float h2f_lo(uint32_t p) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(p & 0xffffu)); }
__device__ __forceinline__ float h2f_hi(uint32_t p) { return (float)__builtin_bit_cast(_Float16, (uint16_t)(p >> 16)); }

// 8 codes (one dword, nibble i = k i) -> 8 bf16 of code * s + mn, in k order
__device__ __forceinline__ u32x4_t w4x8_to_bf16(const uint32_t w, const float s, const float mn) {
  const uint32_t lo = w & 0x0f0f0f0fu, hi = (w >> 4) & 0x0f0f0f0fu;   // byte b: k = 2 b | k = 2 b + 1
  u32x4_t o;
#pragma unroll
  for (int b = 0; b < 4; ++b) {
    const float e = (float)((lo >> (8 * b)) & 0xffu), d = (float)((hi >> (8 * b)) & 0xffu);
    o[b] = pack2bf(fmaf(e, s, mn), fmaf(d, s, mn));
  }
  return o;
}

// 8 codes (one dword) -> 8 exact bf16 of 128 + code (0x4300 | c), pairs (k i, k i + 4): the A operand
// that meets them is permuted by pair_i_i4
__device__ __forceinline__ bf16x8_t w4x8_exact(const uint32_t w) {
  return __builtin_bit_cast(
      bf16x8_t, (u32x4_t){(w & 0x000f000fu) | 0x43004300u, ((w >> 4) & 0x000f000fu) | 0x43004300u,
                          ((w >> 8) & 0x000f000fu) | 0x43004300u, ((w >> 12) & 0x000f000fu) | 0x43004300u});
}

// 8 bf16 a_0 .. a_7 -> (a_0, a_4), (a_1, a_5), (a_2, a_6), (a_3, a_7)
__device__ __forceinline__ bf16x8_t pair_i_i4(const u32x4_t a) {
  return __builtin_bit_cast(bf16x8_t, (u32x4_t){(a[0] & 0xffffu) | (a[2] << 16), (a[0] >> 16) | (a[2] & 0xffff0000u),
                                                (a[1] & 0xffffu) | (a[3] << 16), (a[1] >> 16) | (a[3] & 0xffff0000u)});
}

}  // namespace lumen
