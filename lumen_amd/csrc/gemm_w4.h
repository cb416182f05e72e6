// Weight-only 4-bit group-quantised GEMMs for the LLM decoder (gemm_w4.hip).  The decode launch
// plan (w4_dec_plan) is declared with the scaffold, gemm_wdec.h.
#pragma once
#include "gemm_wdec.h"

namespace lumen {

// C[M, N] = epi(A[M, K] . dq(W4)[N, K]^T), dq(W4)[n, k] = code[n, k] * scale[n, k / G] + wmin[n, k / G].
// W4: uint8 [N, K / 2], two codes per byte, low nibble = even k.  params: fp16 [N, K / G, 2]
// (scale, wmin) contiguous, read as one dword per group.  G in {32, 128}, K % G == 0.
hipError_t gemm_w4(const uint16_t* A, int64_t lda, const uint8_t* W4, int64_t ldw, const uint32_t* params, int G,
                   void* C, int64_t ldc, int M, int N, int K, const GemmEpi& ep, float* ws, uint32_t* cnt, int ksplit,
                   hipStream_t stream);

}  // namespace lumen
