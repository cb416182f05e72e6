// Sparse mixture-of-experts MLP (Qwen3-MoE): device-side routing, a stable counting sort of the
// (token, choice) pairs by expert, the two grouped expert GEMMs and the weighted combine
// (moe.hip).  No step reads anything back on the host and every launch is sized from
// (T, E, k, H, I) alone, so one captured graph replays for any routing.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lumen {

constexpr int MOE_MAX_EXPERTS = 256;
constexpr int MOE_MAX_TOPK = 8;
// pairs (T * k) up to this bound take the 16-row kernels (decode / verify: most experts hold
// 0 - 4 rows); above it an expert's rows run 64 per pass so its weights are re-read 4x less
constexpr int MOE_DECODE_PAIRS = 512;
// most pairs a call may hold: the grouping is one workgroup's walk over all of them
constexpr int MOE_MAX_PAIRS = 1 << 20;

// Workspace of one call, P = T * k pairs (all written before they are read: no initialisation).
struct MoeWork {
  int* cnt;         // [E] rows per expert
  int* off;         // [E] exclusive offsets into the sorted order
  int* active;      // [E + 1] ids of the non-empty experts, ascending; active[E] = how many
  int* pos;         // [P] pair -> sorted position (-1: dropped, id outside [0, E))
  int* src_tok;     // [P] sorted position -> token row
  uint16_t* g;      // [P, I] bf16 silu(gate) * up, sorted order
  float* y;         // [P, H] fp32 down projections, sorted order
};

// x [T, H] bf16 (row stride ldx), gate_w [E, H] bf16 -> ids [T, k] int32, w [T, k] fp32
hipError_t moe_route(const uint16_t* x, int64_t ldx, const uint16_t* gate_w, int T, int E, int k, int H, int norm_topk,
                     float* logits, int* ids, float* w, hipStream_t stream);

// ids [T, k] -> work.cnt / off / active / pos / src_tok
hipError_t moe_group(const int* ids, int T, int E, int k, const MoeWork& work, hipStream_t stream);

// x [T, H] bf16, gu_w [E, 2I, H], down_w [E, H, I] -> work.y, through work.g (after moe_group)
hipError_t moe_expert_gemms(const uint16_t* x, int64_t ldx, const uint16_t* gu_w, const uint16_t* down_w, int T, int E,
                            int k, int H, int I, const MoeWork& work, hipStream_t stream);

// Quantised experts (moe_wq.hip).  MOE_W_FP8: e4m3fn codes [E, N, K] with fp32 scales [E, N], H and I
// multiples of 64.  MOE_W_W4: two 4-bit codes per byte [E, N, K / 2] with fp16 (scale, wmin) per group
// [E, N, K / G, 2], G = 128 where K is a multiple of 128, otherwise 32.
enum MoeWeightFormat : int { MOE_W_BF16 = 0, MOE_W_FP8 = 1, MOE_W_W4 = 2 };

// moe_expert_gemms for fp8 / 4-bit experts: gu_s / down_s are the scales or group parameters
hipError_t moe_expert_gemms_q(const uint16_t* x, int64_t ldx, const void* gu_w, const void* gu_s, const void* down_w,
                              const void* down_s, int format, int T, int E, int k, int H, int I, const MoeWork& work,
                              hipStream_t stream);

// One grouped GEMM with no epilogue: work.y [T k, N] fp32 in sorted order, row p = x[src_tok[p]] times
// the matrix [N, K] of the pair's expert (after moe_group; work.g is not used).  N % 16 == 0.
hipError_t moe_grouped_gemm(const uint16_t* x, int64_t ldx, const uint16_t* w, int T, int E, int k, int N, int K,
                            const MoeWork& work, hipStream_t stream);
hipError_t moe_grouped_gemm_q(const uint16_t* x, int64_t ldx, const void* w, const void* s, int format, int T, int E,
                              int k, int N, int K, const MoeWork& work, hipStream_t stream);

// out[t] = residual[t] + sum_j w[t, j] * y[pos[t k + j]] (fp32, fixed j order, one bf16 rounding)
hipError_t moe_combine(const float* w, const uint16_t* residual, int64_t ldr, uint16_t* out, int64_t ldo, int T, int k,
                       int H, const MoeWork& work, hipStream_t stream);

}  // namespace lumen
