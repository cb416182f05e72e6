// torch.ops.lumen.* registration of the sparse mixture-of-experts MLP (moe.hip): moe_route (router
// logits + top-k + weights), moe_experts (group by expert, the two grouped GEMMs, combine) for bf16
// experts, moe_experts_q for fp8 / 4-bit experts and moe_grouped_linear (one grouped GEMM, any format).
// Workspaces are torch allocations of the call, so stream capture into a graph's pool keeps working.
#include <ATen/ATen.h>
#include <ATen/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>
#include <torch/library.h>

#include <tuple>

#include "moe.h"

namespace {

#define CHECK_HIP_MOE(expr)                                                                \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    TORCH_CHECK(_e == hipSuccess, "lumen HIP error: ", hipGetErrorString(_e), " @ ", #expr); \
  } while (0)

inline hipStream_t cur() { return c10::hip::getCurrentHIPStream().stream(); }
inline uint16_t* bfp(const at::Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }

// bf16 rows [rows, cols] with unit inner stride, 16-byte aligned rows
void check_rows(const at::Tensor& t, int64_t rows, int64_t cols, const at::Tensor& like, const char* what) {
  TORCH_CHECK_VALUE(t.is_cuda() && t.device() == like.device() && t.scalar_type() == at::kBFloat16 && t.dim() == 2 &&
                        t.size(0) == rows && t.size(1) == cols && t.stride(1) == 1 && t.stride(0) % 8 == 0 &&
                        reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
                    "moe: ", what, " must be bf16 [", rows, ", ", cols, "] rows, 16-byte aligned, on x's device");
}

void check_weight(const at::Tensor& t, at::IntArrayRef shape, const at::Tensor& like, const char* what) {
  TORCH_CHECK_VALUE(t.is_cuda() && t.device() == like.device() && t.scalar_type() == at::kBFloat16 &&
                        t.is_contiguous() && t.sizes() == shape && reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
                    "moe: ", what, " must be contiguous bf16 ", shape, " on x's device, got ", t.sizes());
}

// Format of expert weights from their dtype (ops.linear's convention): bf16, float8_e4m3fn + fp32
// scales, uint8 (two 4-bit codes) + fp16 (scale, wmin).
int weight_format(const at::Tensor& w, const char* what) {
  if (w.scalar_type() == at::kBFloat16) return lumen::MOE_W_BF16;
  if (w.scalar_type() == at::kFloat8_e4m3fn) return lumen::MOE_W_FP8;
  TORCH_CHECK_VALUE(w.scalar_type() == at::kByte, "moe: ", what, " must be bf16, float8_e4m3fn or uint8 (4-bit codes)");
  return lumen::MOE_W_W4;
}

// codes [E, N, K] (4-bit: [E, N, K / 2]) and their scales [E, N] fp32 / parameters [E, N, K / G, 2] fp16
void check_qweight(const at::Tensor& t, const at::Tensor& s, int fmt, int64_t E, int64_t N, int64_t K,
                   const at::Tensor& like, const char* what) {
  const bool w4 = fmt == lumen::MOE_W_W4;
  TORCH_CHECK_VALUE(w4 ? K % 32 == 0 : K % 64 == 0, "moe: ", what, ": K % ", w4 ? 32 : 64, " == 0 for this format, got ", K);
  TORCH_CHECK_VALUE(N % 16 == 0, "moe: ", what, ": N % 16 == 0, got ", N);
  TORCH_CHECK_VALUE(t.is_cuda() && t.device() == like.device() && t.is_contiguous() && t.dim() == 3 && t.size(0) == E &&
                        t.size(1) == N && t.size(2) == (w4 ? K / 2 : K) &&
                        reinterpret_cast<uintptr_t>(t.data_ptr()) % 16 == 0,
                    "moe: ", what, " must be contiguous codes [", E, ", ", N, ", ", w4 ? K / 2 : K, "] on x's device, got ",
                    t.sizes());
  if (w4) {
    const int64_t G = K % 128 == 0 ? 128 : 32;
    TORCH_CHECK_VALUE(s.is_cuda() && s.device() == like.device() && s.is_contiguous() && s.scalar_type() == at::kHalf &&
                          s.dim() == 4 && s.size(0) == E && s.size(1) == N && s.size(2) == K / G && s.size(3) == 2,
                      "moe: ", what, " parameters must be contiguous fp16 [", E, ", ", N, ", ", K / G, ", 2], got ",
                      s.sizes());
  } else {
    TORCH_CHECK_VALUE(s.is_cuda() && s.device() == like.device() && s.is_contiguous() && s.scalar_type() == at::kFloat &&
                          s.dim() == 2 && s.size(0) == E && s.size(1) == N,
                      "moe: ", what, " scales must be contiguous fp32 [", E, ", ", N, "], got ", s.sizes());
  }
}

void check_dims(int64_t T, int64_t E, int64_t k, int64_t H, int64_t I) {
  TORCH_CHECK_VALUE(E >= 1 && E <= lumen::MOE_MAX_EXPERTS, "moe: 1 <= E <= ", lumen::MOE_MAX_EXPERTS, ", got ", E);
  TORCH_CHECK_VALUE(k >= 1 && k <= E && k <= lumen::MOE_MAX_TOPK, "moe: 1 <= k <= min(E, ", lumen::MOE_MAX_TOPK,
                    "), got k = ", k, ", E = ", E);
  TORCH_CHECK_VALUE(H >= 32 && H % 32 == 0, "moe: H % 32 == 0, got ", H);
  TORCH_CHECK_VALUE(I < 0 || (I >= 32 && I % 32 == 0), "moe: I % 32 == 0, got ", I);
  TORCH_CHECK_VALUE(T >= 0 && T * k <= lumen::MOE_MAX_PAIRS, "moe: T * k <= ", lumen::MOE_MAX_PAIRS,
                    " (chunk a longer prefill), got ", T * k);
}

// x [T, H] bf16, gate_w [E, H] bf16 -> (ids int32 [T, k], w fp32 [T, k])
std::tuple<at::Tensor, at::Tensor> moe_route(const at::Tensor& x, const at::Tensor& gate_w, int64_t k, bool norm_topk) {
  TORCH_CHECK_VALUE(x.dim() == 2 && gate_w.dim() == 2, "moe_route: x [T, H], gate_w [E, H]");
  const int64_t T = x.size(0), H = x.size(1), E = gate_w.size(0);
  check_dims(T, E, k, H, -1);
  check_rows(x, T, H, x, "x");
  check_weight(gate_w, {E, H}, x, "gate_w");
  const at::DeviceGuard g(x.device());
  at::Tensor ids = at::empty({T, k}, x.options().dtype(at::kInt));
  at::Tensor w = at::empty({T, k}, x.options().dtype(at::kFloat));
  if (T == 0) return {ids, w};
  at::Tensor logits = at::empty({T, E}, x.options().dtype(at::kFloat));
  CHECK_HIP_MOE(lumen::moe_route(bfp(x), x.stride(0), bfp(gate_w), (int)T, (int)E, (int)k, (int)H, norm_topk ? 1 : 0,
                                 logits.data_ptr<float>(), ids.data_ptr<int>(), w.data_ptr<float>(), cur()));
  return {ids, w};
}

// Workspace of one call (torch allocations: capture-safe): besides a few ints per pair, g bf16 [T k, I]
// and y fp32 [T k, H], i.e. 2 k (I + 2 H) bytes per row -- 25 + 134 MB at T = 2048 of the Qwen3-30B-A3B
// layer -- allocated per call and linear in the prefill length (a caller bounds it by chunking the prefill).
struct Work {
  at::Tensor iw, gbuf, ybuf;
  lumen::MoeWork w{};
};

Work make_work(const at::Tensor& x, int64_t T, int64_t E, int64_t k, int64_t H, int64_t I) {
  Work wk;
  const int64_t P = T * k;
  wk.iw = at::empty({3 * E + 1 + 2 * P}, x.options().dtype(at::kInt));
  wk.gbuf = at::empty({P, I}, x.options());
  wk.ybuf = at::empty({P, H}, x.options().dtype(at::kFloat));
  int* ip = wk.iw.data_ptr<int>();
  wk.w.cnt = ip;
  wk.w.off = ip + E;
  wk.w.active = ip + 2 * E;
  wk.w.pos = ip + 3 * E + 1;
  wk.w.src_tok = ip + 3 * E + 1 + P;
  wk.w.g = bfp(wk.gbuf);
  wk.w.y = wk.ybuf.data_ptr<float>();
  return wk;
}

// returns whether a residual was given
bool check_expert_tensors(const at::Tensor& x, const at::Tensor& gu_w, const at::Tensor& down_w,
                          const c10::optional<at::Tensor>& residual, const at::Tensor& out, int64_t k) {
  TORCH_CHECK_VALUE(x.dim() == 2 && gu_w.dim() == 3 && down_w.dim() == 3,
                    "moe: x [T, H], gu_w [E, 2I, H], down_w [E, H, I]");
  const int64_t T = x.size(0), H = x.size(1), E = gu_w.size(0), I = down_w.size(2);
  check_dims(T, E, k, H, I);
  check_rows(x, T, H, x, "x");
  check_weight(gu_w, {E, 2 * I, H}, x, "gu_w");
  check_weight(down_w, {E, H, I}, x, "down_w");
  check_rows(out, T, H, x, "out");
  const bool has_res = residual.has_value() && residual->defined();
  if (has_res) check_rows(*residual, T, H, x, "residual");
  return has_res;
}

// the grouped GEMMs and the combine, once the pairs are grouped in wk
void experts_tail(const at::Tensor& x, const float* w, const at::Tensor& gu_w, const at::Tensor& down_w,
                  const at::Tensor* residual, at::Tensor& out, int64_t k, Work& wk, hipStream_t st) {
  const int64_t T = x.size(0), H = x.size(1), E = gu_w.size(0), I = down_w.size(2);
  CHECK_HIP_MOE(lumen::moe_expert_gemms(bfp(x), x.stride(0), bfp(gu_w), bfp(down_w), (int)T, (int)E, (int)k, (int)H,
                                        (int)I, wk.w, st));
  CHECK_HIP_MOE(lumen::moe_combine(w, residual ? bfp(*residual) : nullptr, residual ? residual->stride(0) : 0, bfp(out),
                                   out.stride(0), (int)T, (int)k, (int)H, wk.w, st));
}

// out[t] = residual[t] + sum_j w[t, j] * down_e(silu(gate_e x_t) * up_e x_t), e = ids[t, j]; pairs whose id
// lies outside [0, E) contribute nothing.  residual may be out.
void moe_experts(const at::Tensor& x, const at::Tensor& ids, const at::Tensor& w, const at::Tensor& gu_w,
                 const at::Tensor& down_w, const c10::optional<at::Tensor>& residual, at::Tensor out) {
  TORCH_CHECK_VALUE(ids.dim() == 2, "moe_experts: ids [T, k]");
  const int64_t k = ids.size(1);
  const bool has_res = check_expert_tensors(x, gu_w, down_w, residual, out, k);
  const int64_t T = x.size(0), H = x.size(1), E = gu_w.size(0), I = down_w.size(2);
  TORCH_CHECK_VALUE(ids.is_cuda() && ids.device() == x.device() && ids.scalar_type() == at::kInt && ids.is_contiguous() &&
                        ids.size(0) == T, "moe_experts: ids int32 [T, k] contiguous");
  TORCH_CHECK_VALUE(w.is_cuda() && w.device() == x.device() && w.scalar_type() == at::kFloat && w.is_contiguous() &&
                        w.dim() == 2 && w.size(0) == T && w.size(1) == k, "moe_experts: w fp32 [T, k] contiguous");
  if (T == 0) return;
  const at::DeviceGuard g(x.device());
  Work wk = make_work(x, T, E, k, H, I);
  const hipStream_t st = cur();
  CHECK_HIP_MOE(lumen::moe_group(ids.data_ptr<int>(), (int)T, (int)E, (int)k, wk.w, st));
  experts_tail(x, w.data_ptr<float>(), gu_w, down_w, has_res ? &*residual : nullptr, out, k, wk, st);
}

void check_ids(const at::Tensor& x, const at::Tensor& ids, int64_t T) {
  TORCH_CHECK_VALUE(ids.is_cuda() && ids.device() == x.device() && ids.scalar_type() == at::kInt && ids.is_contiguous() &&
                        ids.dim() == 2 && ids.size(0) == T, "moe: ids int32 [T, k] contiguous");
}

// moe_experts for fp8 / 4-bit experts: the format follows gu_w's dtype, gu_s / down_s are the fp32
// scales [E, 2I] / [E, H] or the fp16 group parameters [E, 2I, H / G, 2] / [E, H, I / G, 2].
void moe_experts_q(const at::Tensor& x, const at::Tensor& ids, const at::Tensor& w, const at::Tensor& gu_w,
                   const at::Tensor& gu_s, const at::Tensor& down_w, const at::Tensor& down_s,
                   const c10::optional<at::Tensor>& residual, at::Tensor out) {
  TORCH_CHECK_VALUE(x.dim() == 2 && ids.dim() == 2 && gu_w.dim() == 3 && down_w.dim() == 3,
                    "moe_experts_q: x [T, H], ids [T, k], gu_w [E, 2I, *], down_w [E, H, *]");
  const int fmt = weight_format(gu_w, "gu_w");
  TORCH_CHECK_VALUE(fmt != lumen::MOE_W_BF16 && weight_format(down_w, "down_w") == fmt,
                    "moe_experts_q: gu_w and down_w must both be float8_e4m3fn or both uint8");
  const int64_t T = x.size(0), H = x.size(1), E = gu_w.size(0), I = gu_w.size(1) / 2, k = ids.size(1);
  check_dims(T, E, k, H, I);
  check_rows(x, T, H, x, "x");
  check_qweight(gu_w, gu_s, fmt, E, 2 * I, H, x, "gu_w");
  check_qweight(down_w, down_s, fmt, E, H, I, x, "down_w");
  check_rows(out, T, H, x, "out");
  const bool has_res = residual.has_value() && residual->defined();
  if (has_res) check_rows(*residual, T, H, x, "residual");
  check_ids(x, ids, T);
  TORCH_CHECK_VALUE(w.is_cuda() && w.device() == x.device() && w.scalar_type() == at::kFloat && w.is_contiguous() &&
                        w.dim() == 2 && w.size(0) == T && w.size(1) == k, "moe_experts_q: w fp32 [T, k] contiguous");
  if (T == 0) return;
  const at::DeviceGuard g(x.device());
  Work wk = make_work(x, T, E, k, H, I);
  const hipStream_t st = cur();
  CHECK_HIP_MOE(lumen::moe_group(ids.data_ptr<int>(), (int)T, (int)E, (int)k, wk.w, st));
  CHECK_HIP_MOE(lumen::moe_expert_gemms_q(bfp(x), x.stride(0), gu_w.data_ptr(), gu_s.data_ptr(), down_w.data_ptr(),
                                          down_s.data_ptr(), fmt, (int)T, (int)E, (int)k, (int)H, (int)I, wk.w, st));
  CHECK_HIP_MOE(lumen::moe_combine(w.data_ptr<float>(), has_res ? bfp(*residual) : nullptr,
                                   has_res ? residual->stride(0) : 0, bfp(out), out.stride(0), (int)T, (int)k, (int)H,
                                   wk.w, st));
}

// One grouped GEMM: x [T, K] bf16, ids [T, k], W [E, N, K] in any expert format -> (y fp32 [T k, N] in
// sorted order, pos int32 [T k]: pair -> its row of y, -1 for an id outside [0, E)).
std::tuple<at::Tensor, at::Tensor> moe_grouped_linear(const at::Tensor& x, const at::Tensor& ids, const at::Tensor& W,
                                                      const c10::optional<at::Tensor>& w_scale) {
  TORCH_CHECK_VALUE(x.dim() == 2 && ids.dim() == 2 && W.dim() == 3, "moe_grouped_linear: x [T, K], ids [T, k], W [E, N, *]");
  const int fmt = weight_format(W, "W");
  const int64_t T = x.size(0), K = x.size(1), E = W.size(0), N = W.size(1), k = ids.size(1);
  TORCH_CHECK_VALUE(E >= 1 && E <= lumen::MOE_MAX_EXPERTS, "moe: 1 <= E <= ", lumen::MOE_MAX_EXPERTS, ", got ", E);
  TORCH_CHECK_VALUE(k >= 1 && T * k <= lumen::MOE_MAX_PAIRS, "moe: 1 <= k and T * k <= ", lumen::MOE_MAX_PAIRS);
  check_rows(x, T, K, x, "x");
  check_ids(x, ids, T);
  const bool has_s = w_scale.has_value() && w_scale->defined();
  if (fmt == lumen::MOE_W_BF16) {
    TORCH_CHECK_VALUE(!has_s, "moe_grouped_linear: bf16 weights take no w_scale");
    TORCH_CHECK_VALUE(K % 32 == 0 && N % 16 == 0, "moe_grouped_linear: K % 32 == 0 and N % 16 == 0, got ", K, ", ", N);
    check_weight(W, {E, N, K}, x, "W");
  } else {
    TORCH_CHECK_VALUE(has_s, "moe_grouped_linear: quantised weights need w_scale");
    check_qweight(W, *w_scale, fmt, E, N, K, x, "W");
  }
  const at::DeviceGuard g(x.device());
  const int64_t P = T * k;
  at::Tensor iw = at::empty({3 * E + 1 + 2 * P}, x.options().dtype(at::kInt));
  at::Tensor y = at::empty({P, N}, x.options().dtype(at::kFloat));
  at::Tensor pos = iw.narrow(0, 3 * E + 1, P);
  if (T == 0) return {y, pos};
  lumen::MoeWork wk{};
  int* ip = iw.data_ptr<int>();
  wk.cnt = ip; wk.off = ip + E; wk.active = ip + 2 * E; wk.pos = ip + 3 * E + 1; wk.src_tok = ip + 3 * E + 1 + P;
  wk.y = y.data_ptr<float>();
  const hipStream_t st = cur();
  CHECK_HIP_MOE(lumen::moe_group(ids.data_ptr<int>(), (int)T, (int)E, (int)k, wk, st));
  if (fmt == lumen::MOE_W_BF16)
    CHECK_HIP_MOE(lumen::moe_grouped_gemm(bfp(x), x.stride(0), bfp(W), (int)T, (int)E, (int)k, (int)N, (int)K, wk, st));
  else
    CHECK_HIP_MOE(lumen::moe_grouped_gemm_q(bfp(x), x.stride(0), W.data_ptr(), w_scale->data_ptr(), fmt, (int)T, (int)E,
                                            (int)k, (int)N, (int)K, wk, st));
  return {y, pos};
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(lumen, m) {
  m.def("moe_route(Tensor x, Tensor gate_w, int k, bool norm_topk) -> (Tensor, Tensor)");
  m.def("moe_experts(Tensor x, Tensor ids, Tensor w, Tensor gu_w, Tensor down_w, Tensor? residual, Tensor(a!) out) -> ()");
  m.def("moe_experts_q(Tensor x, Tensor ids, Tensor w, Tensor gu_w, Tensor gu_s, Tensor down_w, Tensor down_s, "
        "Tensor? residual, Tensor(a!) out) -> ()");
  m.def("moe_grouped_linear(Tensor x, Tensor ids, Tensor W, Tensor? w_scale) -> (Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(lumen, CUDA, m) {
  m.impl("moe_route", &moe_route);
  m.impl("moe_experts", &moe_experts);
  m.impl("moe_experts_q", &moe_experts_q);
  m.impl("moe_grouped_linear", &moe_grouped_linear);
}
