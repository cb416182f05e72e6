// torch.ops.lumen.* registration of the sparse mixture-of-experts MLP (moe.hip): moe_route (router
// logits + top-k + weights) and moe_experts (group by expert, the two grouped GEMMs, combine).
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

}  // namespace

TORCH_LIBRARY_FRAGMENT(lumen, m) {
  m.def("moe_route(Tensor x, Tensor gate_w, int k, bool norm_topk) -> (Tensor, Tensor)");
  m.def("moe_experts(Tensor x, Tensor ids, Tensor w, Tensor gu_w, Tensor down_w, Tensor? residual, Tensor(a!) out) -> ()");
}

TORCH_LIBRARY_IMPL(lumen, CUDA, m) {
  m.impl("moe_route", &moe_route);
  m.impl("moe_experts", &moe_experts);
}
