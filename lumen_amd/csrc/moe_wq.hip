// Quantised experts of the sparse mixture-of-experts MLP: the fp8 and 4-bit instantiations of
// moe_gemm_kernel (moe_gemm.h) for the gate|up and down GEMMs, 16- and 64-row tiles:
//
//   MoeFp8         4 kernels    e4m3fn codes, fp32 scale per output row of every expert
//   MoeW4<true>    4 kernels    4-bit codes, fp16 (scale, wmin) per group of 128 along K
//   MoeW4<false>   4 kernels    ... per group of 32 (K no multiple of 128)
//
// The router GEMM stays bf16 / fp32 (moe.hip).  The decode and verify GEMMs are bound by the expert
// weight stream, so the bytes per weight are what a format changes; activations stay bf16,
// accumulation is fp32 and the summation order is fixed, as for bf16 experts.
#include "common.h"
#include "moe.h"
#include "moe_gemm.h"

namespace lumen {

namespace {
// log2 of the 4-bit group size of a [*, K] matrix (ops.w4_group)
inline int w4_gshift(int K) { return K % 128 == 0 ? 7 : 5; }
}  // namespace

hipError_t moe_expert_gemms_q(const uint16_t* x, int64_t ldx, const void* gu_w, const void* gu_s, const void* down_w,
                              const void* down_s, int format, int T, int E, int k, int H, int I, const MoeWork& work,
                              hipStream_t stream) {
  if (gu_s == nullptr || down_s == nullptr) return hipErrorInvalidValue;
  if (format == MOE_W_FP8) {
    if (H % 64 != 0 || I % 64 != 0) return hipErrorInvalidValue;
    return moe_launch_experts<MoeFp8>(x, ldx, gu_w, gu_s, down_w, down_s, (int64_t)2 * I * H, (int64_t)H * I, 0, 0, T, E,
                                      k, H, I, work, stream);
  }
  if (format != MOE_W_W4 || H % 32 != 0 || I % 32 != 0) return hipErrorInvalidValue;
  // the group size follows K per GEMM: gate|up has K = H, down K = I
  const int gs_gu = w4_gshift(H), gs_dn = w4_gshift(I);
  const int64_t st_gu = (int64_t)2 * I * (H / 2), st_dn = (int64_t)H * (I / 2);
#define MOE_W4_LAUNCH(GU_, DN_)                                                                              \
  moe_launch_experts<MoeW4<GU_>, MoeW4<DN_>>(x, ldx, gu_w, gu_s, down_w, down_s, st_gu, st_dn, gs_gu, gs_dn, T, E, k, H, \
                                             I, work, stream)
  if (gs_gu == 7) return gs_dn == 7 ? MOE_W4_LAUNCH(true, true) : MOE_W4_LAUNCH(true, false);
  return gs_dn == 7 ? MOE_W4_LAUNCH(false, true) : MOE_W4_LAUNCH(false, false);
#undef MOE_W4_LAUNCH
}

hipError_t moe_grouped_gemm_q(const uint16_t* x, int64_t ldx, const void* w, const void* s, int format, int T, int E,
                              int k, int N, int K, const MoeWork& work, hipStream_t stream) {
  if (s == nullptr || N % 16 != 0) return hipErrorInvalidValue;
  if (format == MOE_W_FP8) {
    if (K % 64 != 0) return hipErrorInvalidValue;
    return moe_launch_grouped<MoeFp8>(x, ldx, w, s, (int64_t)N * K, 0, T, E, k, N, K, work, stream);
  }
  if (format != MOE_W_W4 || K % 32 != 0) return hipErrorInvalidValue;
  const int64_t st = (int64_t)N * (K / 2);
  if (w4_gshift(K) == 7) return moe_launch_grouped<MoeW4<true>>(x, ldx, w, s, st, 7, T, E, k, N, K, work, stream);
  return moe_launch_grouped<MoeW4<false>>(x, ldx, w, s, st, 5, T, E, k, N, K, work, stream);
}

}  // namespace lumen
