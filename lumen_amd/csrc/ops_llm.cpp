// torch.ops.lumen.* registration of the decoder-LLM kernels (llm.hip): fused RoPE +
// paged KV-cache write, paged flash-decoding attention, paged prefill / verify attention, repetition penalty.
#include <ATen/ATen.h>
#include <ATen/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <hip/hip_runtime.h>
#include <torch/library.h>

#include "llm.h"
#include "sampler.h"

namespace lumen {
uint32_t* splitk_counters(const at::Tensor& like, int64_t tiles);   // ops.cpp
}

namespace {

int64_t* g_decode_dbg = nullptr;   // profiling only (decode_set_dbg)

#define CHECK_HIP3(expr)                                                                   \
  do {                                                                                     \
    hipError_t _e = (expr);                                                                \
    TORCH_CHECK(_e == hipSuccess, "lumen HIP error: ", hipGetErrorString(_e), " @ ", #expr); \
  } while (0)

inline hipStream_t cur() { return c10::hip::getCurrentHIPStream().stream(); }
inline uint16_t* bfp(const at::Tensor& t) { return reinterpret_cast<uint16_t*>(t.data_ptr()); }

// bf16 or float8_e4m3fn caches (both the same dtype); returns 1 for fp8
int check_cache(const at::Tensor& kc, const at::Tensor& vc, int64_t Hkv, int64_t D) {
  const bool f8 = kc.scalar_type() == at::kFloat8_e4m3fn;
  TORCH_CHECK(kc.is_cuda() && (kc.scalar_type() == at::kBFloat16 || f8) && kc.is_contiguous() && kc.dim() == 4,
              "k_cache: bf16 / float8_e4m3fn [NB, Hkv, 64, D]");
  TORCH_CHECK(vc.is_cuda() && vc.scalar_type() == kc.scalar_type() && vc.is_contiguous() && vc.dim() == 4,
              "v_cache: same dtype as k_cache, [NB, Hkv, D, 64]");
  TORCH_CHECK(kc.size(1) == Hkv && kc.size(2) == lumen::KV_BLOCK && kc.size(3) == D, "k_cache shape");
  TORCH_CHECK(vc.size(0) == kc.size(0) && vc.size(1) == Hkv && vc.size(2) == D && vc.size(3) == lumen::KV_BLOCK,
              "v_cache shape");
  return f8 ? 1 : 0;
}

// per-head q / k RMSNorm weights (Qwen3): both or neither, f32 [D], 16-byte aligned; returns true when given
bool check_qk_norm(const c10::optional<at::Tensor>& qg, const c10::optional<at::Tensor>& kg, double eps, int64_t D,
                   const at::Tensor& like, const float** q_gamma, const float** k_gamma) {
  const bool hq = qg.has_value() && qg->defined(), hk = kg.has_value() && kg->defined();
  TORCH_CHECK(hq == hk, "qk norm: q_gamma and k_gamma come together");
  if (!hq) return false;
  TORCH_CHECK(D == 32 || D == 64 || D == 128, "qk norm: head dim 32, 64 or 128");
  TORCH_CHECK(eps > 0, "qk norm: eps > 0");
  for (const at::Tensor* t : {&*qg, &*kg})
    TORCH_CHECK(t->is_cuda() && t->device() == like.device() && t->scalar_type() == at::kFloat && t->is_contiguous() &&
                t->numel() == D && reinterpret_cast<uintptr_t>(t->data_ptr()) % 16 == 0, "qk norm: gamma f32 [D]");
  *q_gamma = qg->data_ptr<float>();
  *k_gamma = kg->data_ptr<float>();
  return true;
}

// qkv [T, >= (H + 2 Hkv) D] bf16 (rotated in place); pos int32 [T]; cos_sin f32 [P, D/2, 2];
// slots int64 [T] (optional): writes rotated k / v into the paged cache.  q_gamma / k_gamma f32 [D]
// (optional): per-head RMSNorm of q and k before the rotation.  mrope_axes uint8 [D/2] on the host
// (optional, values 0 / 1 / 2): multimodal RoPE, pos int32 [3, T] and frequency i rotated by the
// position of axis mrope_axes[i] (ops/llm.py mrope_axes).
void rope_kv(at::Tensor qkv, const at::Tensor& pos, const at::Tensor& cos_sin, const c10::optional<at::Tensor>& slots,
             at::Tensor k_cache, at::Tensor v_cache, int64_t H, int64_t Hkv, int64_t D,
             const c10::optional<at::Tensor>& q_gamma, const c10::optional<at::Tensor>& k_gamma, double qk_eps,
             const c10::optional<at::Tensor>& mrope_axes) {
  TORCH_CHECK(qkv.is_cuda() && qkv.scalar_type() == at::kBFloat16 && qkv.dim() == 2 && qkv.stride(1) == 1, "qkv");
  TORCH_CHECK(qkv.size(1) >= (H + 2 * Hkv) * D, "qkv: too few columns");
  TORCH_CHECK(D % 2 == 0 && D <= 256, "rope: head dim");
  const int64_t T = qkv.size(0);
  const bool mrope = mrope_axes.has_value() && mrope_axes->defined();
  TORCH_CHECK(pos.is_cuda() && pos.scalar_type() == at::kInt && pos.is_contiguous(), "pos int32");
  TORCH_CHECK(mrope || pos.numel() == T, "pos int32 [T]");
  TORCH_CHECK(!mrope || (pos.dim() == 2 && pos.size(0) == 3 && pos.size(1) == T), "mrope: pos int32 [3, T]");
  TORCH_CHECK(cos_sin.is_cuda() && cos_sin.scalar_type() == at::kFloat && cos_sin.is_contiguous() &&
              cos_sin.dim() == 3 && cos_sin.size(1) == D / 2 && cos_sin.size(2) == 2, "cos_sin f32 [P, D/2, 2]");
  lumen::RopeKVArgs a{};
  a.qkv = bfp(qkv); a.ld = qkv.stride(0);
  a.pos = pos.data_ptr<int>(); a.cos_sin = cos_sin.data_ptr<float>();
  if (slots.has_value() && slots->defined()) {
    TORCH_CHECK(slots->is_cuda() && slots->scalar_type() == at::kLong && slots->numel() == T && slots->is_contiguous(),
                "slots int64 [T]");
    a.kv_fp8 = check_cache(k_cache, v_cache, Hkv, D);
    a.slots = slots->data_ptr<int64_t>();
    a.k_cache = reinterpret_cast<uint16_t*>(k_cache.data_ptr()); a.v_cache = reinterpret_cast<uint16_t*>(v_cache.data_ptr());
  }
  a.T = (int)T; a.H = (int)H; a.Hkv = (int)Hkv; a.D = (int)D;
  if (check_qk_norm(q_gamma, k_gamma, qk_eps, D, qkv, &a.q_gamma, &a.k_gamma)) a.eps = (float)qk_eps;
  if (mrope) {
    TORCH_CHECK(D == 32 || D == 64 || D == 128, "mrope: head dim 32, 64 or 128");
    TORCH_CHECK(mrope_axes->is_cpu() && mrope_axes->scalar_type() == at::kByte && mrope_axes->is_contiguous() &&
                mrope_axes->numel() == D / 2, "mrope: axes uint8 [D/2] on the host");
    const uint8_t* ax = mrope_axes->data_ptr<uint8_t>();
    for (int64_t i = 0; i < D / 2; ++i) {
      TORCH_CHECK(ax[i] <= 2, "mrope: axes are 0 (t), 1 (h) or 2 (w)");
      a.mrope_axes[i >> 5] |= (uint64_t)ax[i] << ((i & 31) * 2);
    }
    a.mrope = 1;
  }
  const at::DeviceGuard g(qkv.device());
  CHECK_HIP3(lumen::rope_kv(a, cur()));
}

// q [B, >= H D] rows (bf16); block_table int32 [B, max_blocks]; ctx_len int32 [B]; out [B, >= H D] rows.
void paged_decode(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
                  const at::Tensor& block_table, const at::Tensor& ctx_len, at::Tensor out, int64_t H, int64_t Hkv,
                  double scale, int64_t nsplit, int64_t blocks_per_split, const c10::optional<at::Tensor>& part_o,
                  const c10::optional<at::Tensor>& part_ml, const c10::optional<at::Tensor>& pos,
                  const c10::optional<at::Tensor>& cos_sin, const c10::optional<at::Tensor>& slots,
                  const c10::optional<at::Tensor>& pf0, const c10::optional<at::Tensor>& pf1) {
  const int64_t D = k_cache.size(3);
  const int kv_fp8 = check_cache(k_cache, v_cache, Hkv, D);
  TORCH_CHECK(D == 32 || D == 64 || D == 128, "paged_decode: head dim 32, 64 or 128");
  TORCH_CHECK(H % Hkv == 0 && H / Hkv <= 16, "paged_decode: at most 16 query heads per kv head");
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16 && q.dim() == 2 && q.stride(1) == 1 && q.size(1) >= H * D &&
              q.stride(0) % 8 == 0, "paged_decode: q rows");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kBFloat16 && out.dim() == 2 && out.stride(1) == 1 &&
              out.size(1) >= H * D, "paged_decode: out rows");
  const int64_t B = q.size(0);
  TORCH_CHECK(out.size(0) == B, "paged_decode: out batch");
  TORCH_CHECK(block_table.is_cuda() && block_table.scalar_type() == at::kInt && block_table.dim() == 2 &&
              block_table.size(0) == B && block_table.stride(1) == 1, "block_table int32 [B, max_blocks]");
  TORCH_CHECK(ctx_len.is_cuda() && ctx_len.scalar_type() == at::kInt && ctx_len.numel() == B && ctx_len.is_contiguous(),
              "ctx_len int32 [B]");
  // the kernel widens the splits to cover each sequence's own context (blocks per split =
  // max(blocks_per_split, ceil(blocks / nsplit))), so any split count covers the table
  TORCH_CHECK(nsplit >= 1 && blocks_per_split >= 1, "paged_decode: nsplit / blocks_per_split");
  lumen::DecodeArgs a{};
  a.q = bfp(q); a.q_sb = q.stride(0);
  a.k_cache = reinterpret_cast<const uint16_t*>(k_cache.data_ptr());
  a.v_cache = reinterpret_cast<const uint16_t*>(v_cache.data_ptr());
  a.kv_fp8 = kv_fp8;
  a.block_table = block_table.data_ptr<int>(); a.bt_stride = (int)block_table.stride(0);
  a.ctx_len = ctx_len.data_ptr<int>();
  a.o = bfp(out); a.o_sb = out.stride(0);
  a.H = (int)H; a.Hkv = (int)Hkv; a.nsplit = (int)nsplit; a.blocks_per_split = (int)blocks_per_split;
  a.scale_log2 = (float)(scale * 1.4426950408889634);
  if (nsplit > 1) {
    TORCH_CHECK(part_o.has_value() && part_ml.has_value(), "paged_decode: split workspace required");
    TORCH_CHECK(part_o->scalar_type() == at::kFloat && part_o->is_contiguous() && part_o->numel() >= B * H * nsplit * D,
                "part_o");
    TORCH_CHECK(part_ml->scalar_type() == at::kFloat && part_ml->is_contiguous() && part_ml->numel() >= B * H * nsplit * 2,
                "part_ml");
    a.part_o = part_o->data_ptr<float>(); a.part_ml = part_ml->data_ptr<float>();
    TORCH_CHECK(nsplit <= 32, "paged_decode: at most 32 context splits");
    a.split_cnt = lumen::splitk_counters(q, B * Hkv);
  }
  if (pos.has_value() && pos->defined()) {   // fused RoPE + current-token cache write
    TORCH_CHECK(D == 64 || D == 128, "paged_decode: fused rope needs head dim 64 or 128");
    TORCH_CHECK(q.size(1) >= (H + 2 * Hkv) * D, "paged_decode: fused rope needs the packed qkv rows");
    TORCH_CHECK(pos->is_cuda() && pos->scalar_type() == at::kInt && pos->numel() == B && pos->is_contiguous(),
                "pos int32 [B]");
    TORCH_CHECK(cos_sin.has_value() && cos_sin->is_cuda() && cos_sin->scalar_type() == at::kFloat &&
                cos_sin->is_contiguous() && cos_sin->size(-1) == 2 && cos_sin->size(-2) * 2 == D, "cos_sin f32 [P, D/2, 2]");
    TORCH_CHECK(slots.has_value() && slots->is_cuda() && slots->scalar_type() == at::kLong && slots->numel() == B &&
                slots->is_contiguous(), "slots int64 [B]");
    a.pos = pos->data_ptr<int>();
    a.cos_sin = cos_sin->data_ptr<float>();
    a.slots = slots->data_ptr<int64_t>();
    a.k_cache_w = reinterpret_cast<uint16_t*>(k_cache.data_ptr());
    a.v_cache_w = reinterpret_cast<uint16_t*>(v_cache.data_ptr());
  }
  const c10::optional<at::Tensor>* pfs[2] = {&pf0, &pf1};
  for (int r = 0; r < 2; ++r) {
    const auto& t = *pfs[r];
    if (t.has_value() && t->defined()) {
      TORCH_CHECK(t->is_cuda() && t->is_contiguous() && t->device() == q.device(), "paged_decode: prefetch tensor");
      a.pf[r] = reinterpret_cast<const uint8_t*>(t->data_ptr());
      a.pf_bytes[r] = t->numel() * t->element_size();
    }
  }
  if (B == 0) return;
  a.dbg = g_decode_dbg;
  const at::DeviceGuard g(q.device());
  CHECK_HIP3(lumen::paged_decode(a, (int)B, (int)D, cur()));
}

// q [T, >= H D] rows of the rotated packed QKV buffer (bf16); blocks int64 [>= ceil((start_pos + T) / 64)]:
// the sequence's block list; out [T, >= H D] rows.  One sequence per call.
void paged_prefill(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache, const at::Tensor& blocks,
                   int64_t start_pos, int64_t H, int64_t Hkv, double scale, at::Tensor out) {
  TORCH_CHECK(k_cache.dim() == 4, "k_cache: [NB, Hkv, 64, D]");
  const int64_t D = k_cache.size(3);
  const int kv_fp8 = check_cache(k_cache, v_cache, Hkv, D);
  TORCH_CHECK(D == 32 || D == 64 || D == 128, "paged_prefill: head dim 32, 64 or 128");
  TORCH_CHECK(Hkv > 0 && H % Hkv == 0 && H / Hkv <= 16, "paged_prefill: at most 16 query heads per kv head");
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16 && q.dim() == 2 && q.stride(1) == 1 && q.size(1) >= H * D &&
              q.stride(0) % 8 == 0 && reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0, "paged_prefill: q rows");
  const int64_t T = q.size(0);
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kBFloat16 && out.dim() == 2 && out.stride(1) == 1 &&
              out.size(1) >= H * D && out.size(0) == T, "paged_prefill: out rows");
  TORCH_CHECK(q.device() == k_cache.device() && out.device() == q.device() && v_cache.device() == q.device() &&
              blocks.device() == q.device(), "paged_prefill: tensors on one device");
  TORCH_CHECK(blocks.scalar_type() == at::kLong && blocks.dim() == 1 && blocks.is_contiguous(), "blocks int64 [n]");
  TORCH_CHECK(start_pos >= 0 && start_pos + T < (int64_t(1) << 31), "paged_prefill: start_pos");
  TORCH_CHECK(blocks.numel() * lumen::KV_BLOCK >= start_pos + T, "paged_prefill: block list shorter than start_pos + T");
  if (T == 0) return;
  lumen::PrefillArgs a{};
  a.q = bfp(q); a.q_ld = q.stride(0);
  a.k_cache = reinterpret_cast<const uint16_t*>(k_cache.data_ptr());
  a.v_cache = reinterpret_cast<const uint16_t*>(v_cache.data_ptr());
  a.blocks = blocks.data_ptr<int64_t>();
  a.o = bfp(out); a.o_ld = out.stride(0);
  a.start_pos = (int)start_pos; a.T = (int)T; a.H = (int)H; a.Hkv = (int)Hkv;
  a.num_blocks = (int)k_cache.size(0);
  a.scale_log2 = (float)(scale * 1.4426950408889634);
  a.kv_fp8 = kv_fp8;
  const at::DeviceGuard g(q.device());
  CHECK_HIP3(lumen::paged_prefill(a, (int)D, cur()));
}

// q [B * T, >= H D] rows of the rotated packed QKV buffer (bf16), sequence-major; block_table int32 [B, W];
// ctx_len / n_rows int32 [B]; out [B * T, >= H D] rows.  T * (H / Hkv) <= 64.
void paged_verify(const at::Tensor& q, const at::Tensor& k_cache, const at::Tensor& v_cache,
                  const at::Tensor& block_table, const at::Tensor& ctx_len, const at::Tensor& n_rows, at::Tensor out,
                  int64_t T, int64_t H, int64_t Hkv, double scale, int64_t nsplit, int64_t blocks_per_split,
                  const c10::optional<at::Tensor>& part_o, const c10::optional<at::Tensor>& part_ml) {
  TORCH_CHECK(k_cache.dim() == 4, "k_cache: [NB, Hkv, 64, D]");
  const int64_t D = k_cache.size(3);
  const int kv_fp8 = check_cache(k_cache, v_cache, Hkv, D);
  TORCH_CHECK(D == 32 || D == 64 || D == 128, "paged_verify: head dim 32, 64 or 128");
  TORCH_CHECK(Hkv > 0 && H % Hkv == 0 && H / Hkv <= 16, "paged_verify: at most 16 query heads per kv head");
  TORCH_CHECK(T >= 1 && T * (H / Hkv) <= 64, "paged_verify: T * (H / Hkv) must be in 1 .. 64");
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == at::kBFloat16 && q.dim() == 2 && q.stride(1) == 1 && q.size(1) >= H * D &&
              q.stride(0) % 8 == 0 && reinterpret_cast<uintptr_t>(q.data_ptr()) % 16 == 0 && q.size(0) % T == 0,
              "paged_verify: q rows");
  const int64_t B = q.size(0) / T;
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kBFloat16 && out.dim() == 2 && out.stride(1) == 1 &&
              out.size(1) >= H * D && out.size(0) == B * T, "paged_verify: out rows");
  TORCH_CHECK(block_table.is_cuda() && block_table.scalar_type() == at::kInt && block_table.dim() == 2 &&
              block_table.size(0) == B && block_table.size(1) >= 1 && block_table.stride(1) == 1,
              "block_table int32 [B, max_blocks]");
  TORCH_CHECK(ctx_len.is_cuda() && ctx_len.scalar_type() == at::kInt && ctx_len.numel() == B && ctx_len.is_contiguous(),
              "ctx_len int32 [B]");
  TORCH_CHECK(n_rows.is_cuda() && n_rows.scalar_type() == at::kInt && n_rows.numel() == B && n_rows.is_contiguous(),
              "n_rows int32 [B]");
  TORCH_CHECK(q.device() == k_cache.device() && out.device() == q.device() && v_cache.device() == q.device() &&
              block_table.device() == q.device() && ctx_len.device() == q.device() && n_rows.device() == q.device(),
              "paged_verify: tensors on one device");
  TORCH_CHECK(nsplit >= 1 && nsplit <= 32 && blocks_per_split >= 1, "paged_verify: nsplit / blocks_per_split");
  if (B == 0) return;
  lumen::VerifyArgs a{};
  a.q = bfp(q); a.q_ld = q.stride(0);
  a.k_cache = reinterpret_cast<const uint16_t*>(k_cache.data_ptr());
  a.v_cache = reinterpret_cast<const uint16_t*>(v_cache.data_ptr());
  a.kv_fp8 = kv_fp8;
  a.block_table = block_table.data_ptr<int>(); a.bt_stride = (int)block_table.stride(0);
  a.bt_width = (int)block_table.size(1);
  a.ctx_len = ctx_len.data_ptr<int>(); a.n_rows = n_rows.data_ptr<int>();
  a.o = bfp(out); a.o_ld = out.stride(0);
  a.T = (int)T; a.H = (int)H; a.Hkv = (int)Hkv; a.nsplit = (int)nsplit; a.blocks_per_split = (int)blocks_per_split;
  a.num_blocks = (int)k_cache.size(0);
  a.scale_log2 = (float)(scale * 1.4426950408889634);
  if (nsplit > 1) {
    TORCH_CHECK(part_o.has_value() && part_ml.has_value(), "paged_verify: split workspace required");
    TORCH_CHECK(part_o->scalar_type() == at::kFloat && part_o->is_contiguous() && part_o->device() == q.device() &&
                part_o->numel() >= B * T * H * nsplit * D, "part_o");
    TORCH_CHECK(part_ml->scalar_type() == at::kFloat && part_ml->is_contiguous() && part_ml->device() == q.device() &&
                part_ml->numel() >= B * T * H * nsplit * 2, "part_ml");
    a.part_o = part_o->data_ptr<float>(); a.part_ml = part_ml->data_ptr<float>();
    a.split_cnt = lumen::splitk_counters(q, B * Hkv);
  }
  const at::DeviceGuard g(q.device());
  CHECK_HIP3(lumen::paged_verify(a, (int)B, (int)D, cur()));
}

// profiling: per-workgroup timestamps of paged_decode into dbg [B, Hkv, nsplit, 8] int64 (empty: off)
void decode_set_dbg(const at::Tensor& dbg) {
  TORCH_CHECK(dbg.is_cuda() && dbg.scalar_type() == at::kLong && dbg.is_contiguous(), "decode_set_dbg: int64");
  g_decode_dbg = dbg.numel() > 0 ? dbg.data_ptr<int64_t>() : nullptr;
}

void rep_penalty_(at::Tensor logits, const at::Tensor& ids, const at::Tensor& penalty) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kFloat && logits.dim() == 2 && logits.stride(1) == 1,
              "rep_penalty: logits f32 [B, V]");
  const int64_t B = logits.size(0);
  TORCH_CHECK(ids.is_cuda() && ids.scalar_type() == at::kInt && ids.is_contiguous() && ids.dim() == 2 && ids.size(0) == B,
              "rep_penalty: ids int32 [B, n]");
  TORCH_CHECK(penalty.is_cuda() && penalty.scalar_type() == at::kFloat && penalty.numel() == B, "penalty f32 [B]");
  const at::DeviceGuard g(logits.device());
  CHECK_HIP3(lumen::rep_penalty(logits.data_ptr<float>(), logits.stride(0), ids.data_ptr<int>(), (int)ids.size(1),
                                penalty.data_ptr<float>(), (int)B, (int)logits.size(1), cur()));
}

// The in-graph sampler (sampler.hip): per row of logits f32 [B, V] (never written) the repetition
// penalty over the row's seen-bitmap slot, 1/T, the top-64 candidates, the nucleus cut and the draw
// with the uniform u.  Writes tok int32 [B] and out_ids int64 [B] (may alias in_ids), marks
// in_ids[b] in seen[seen_slot[b]]; out_v / out_i [B, 64] and out_lse [B] are optional.
// Guided form: all seven guide tensors or none.  g_allow int32 [A, ceil(V / 32)] and g_dfa int16
// [A, 256] are the arena of grammar states, tok_off int32 [V + 1] / tok_dat uint8 the CSR of the
// token bytes, g_slot / g_in int32 [B], g_state int32 [S] (written).
void sample_rows(const at::Tensor& logits, const at::Tensor& inv_t, const at::Tensor& top_p, const at::Tensor& penalty,
                 const at::Tensor& u, const at::Tensor& greedy, const at::Tensor& seen_slot, at::Tensor seen,
                 const at::Tensor& in_ids, at::Tensor out_ids, at::Tensor tok, const c10::optional<at::Tensor>& out_v,
                 const c10::optional<at::Tensor>& out_i, const c10::optional<at::Tensor>& out_lse,
                 const c10::optional<at::Tensor>& g_allow, const c10::optional<at::Tensor>& g_dfa,
                 const c10::optional<at::Tensor>& tok_off, const c10::optional<at::Tensor>& tok_dat,
                 const c10::optional<at::Tensor>& g_slot, const c10::optional<at::Tensor>& g_in,
                 const c10::optional<at::Tensor>& g_state) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kFloat && logits.dim() == 2 && logits.stride(1) == 1,
              "sample_rows: logits f32 [B, V]");
  const int64_t B = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V >= lumen::SAMPLE_K && V < (int64_t(1) << 31), "sample_rows: V >= 64");
  auto row = [&](const at::Tensor& t, at::ScalarType ty, const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == ty && t.is_contiguous() && t.numel() == B, "sample_rows: ", what);
  };
  row(inv_t, at::kFloat, "inv_t f32 [B]");
  row(top_p, at::kDouble, "top_p f64 [B]");
  row(penalty, at::kFloat, "penalty f32 [B]");
  row(u, at::kDouble, "u f64 [B]");
  row(greedy, at::kInt, "greedy int32 [B]");
  row(seen_slot, at::kInt, "seen_slot int32 [B]");
  row(in_ids, at::kLong, "in_ids int64 [B]");
  row(out_ids, at::kLong, "out_ids int64 [B]");
  row(tok, at::kInt, "tok int32 [B]");
  const int64_t words = (V + 31) / 32;
  TORCH_CHECK(seen.is_cuda() && seen.scalar_type() == at::kInt && seen.is_contiguous() && seen.dim() == 2 &&
              seen.size(1) == words, "sample_rows: seen int32 [S, ceil(V / 32)]");
  lumen::SampleArgs a{};
  a.logits = logits.data_ptr<float>(); a.ld = logits.stride(0);
  a.B = (int)B; a.V = (int)V;
  a.inv_t = inv_t.data_ptr<float>(); a.top_p = top_p.data_ptr<double>(); a.penalty = penalty.data_ptr<float>();
  a.u = u.data_ptr<double>(); a.greedy = greedy.data_ptr<int>(); a.seen_slot = seen_slot.data_ptr<int>();
  a.seen = seen.data_ptr<int>(); a.S = (int)seen.size(0); a.words = (int)words;
  a.in_ids = in_ids.data_ptr<int64_t>(); a.out_ids = out_ids.data_ptr<int64_t>(); a.tok = tok.data_ptr<int>();
  const bool cand = out_v.has_value() && out_v->defined();
  TORCH_CHECK(cand == (out_i.has_value() && out_i->defined()), "sample_rows: out_v and out_i come together");
  if (cand) {
    TORCH_CHECK(out_v->is_cuda() && out_v->scalar_type() == at::kFloat && out_v->is_contiguous() &&
                out_v->numel() == B * lumen::SAMPLE_K, "sample_rows: out_v f32 [B, 64]");
    TORCH_CHECK(out_i->is_cuda() && out_i->scalar_type() == at::kInt && out_i->is_contiguous() &&
                out_i->numel() == B * lumen::SAMPLE_K, "sample_rows: out_i int32 [B, 64]");
    a.out_v = out_v->data_ptr<float>(); a.out_i = out_i->data_ptr<int>();
  }
  if (out_lse.has_value() && out_lse->defined()) {
    TORCH_CHECK(out_lse->is_cuda() && out_lse->scalar_type() == at::kFloat && out_lse->numel() == B &&
                out_lse->is_contiguous(), "sample_rows: out_lse f32 [B]");
    a.out_lse = out_lse->data_ptr<float>();
  }
  auto has = [](const c10::optional<at::Tensor>& t) { return t.has_value() && t->defined(); };
  const int ng = has(g_allow) + has(g_dfa) + has(tok_off) + has(tok_dat) + has(g_slot) + has(g_in) + has(g_state);
  TORCH_CHECK(ng == 0 || ng == 7, "sample_rows: the guide tensors come together");
  if (ng == 7) {
    auto dev = [&](const at::Tensor& t, at::ScalarType ty, const char* what) {
      TORCH_CHECK(t.is_cuda() && t.device() == logits.device() && t.scalar_type() == ty && t.is_contiguous(),
                  "sample_rows: ", what);
    };
    dev(*g_allow, at::kInt, "g_allow int32 [A, ceil(V / 32)]");
    dev(*g_dfa, at::kShort, "g_dfa int16 [A, 256]");
    dev(*tok_off, at::kInt, "tok_off int32 [V + 1]");
    dev(*tok_dat, at::kByte, "tok_dat uint8");
    dev(*g_state, at::kInt, "g_state int32 [S]");
    row(*g_slot, at::kInt, "g_slot int32 [B]");
    row(*g_in, at::kInt, "g_in int32 [B]");
    const int64_t A = g_allow->dim() == 2 ? g_allow->size(0) : 0;
    TORCH_CHECK(A >= 1 && A <= 32767 && g_allow->size(1) == words, "sample_rows: g_allow int32 [A, ceil(V / 32)], A < 2^15");
    TORCH_CHECK(g_dfa->dim() == 2 && g_dfa->size(0) == A && g_dfa->size(1) == 256, "sample_rows: g_dfa int16 [A, 256]");
    TORCH_CHECK(tok_off->numel() == V + 1, "sample_rows: tok_off int32 [V + 1]");
    TORCH_CHECK(g_state->numel() >= 1, "sample_rows: g_state int32 [S]");
    a.g_allow = g_allow->data_ptr<int>(); a.g_dfa = g_dfa->data_ptr<int16_t>();
    a.tok_off = tok_off->data_ptr<int>(); a.tok_dat = tok_dat->data_ptr<uint8_t>();
    a.g_slot = g_slot->data_ptr<int>(); a.g_in = g_in->data_ptr<int>(); a.g_state = g_state->data_ptr<int>();
    a.g_A = (int)A; a.g_S = (int)g_state->numel();
  }
  const at::DeviceGuard g(logits.device());
  const int64_t nws = lumen::sample_ws_floats((int)B, (int)V);
  at::Tensor ws;
  if (nws > 0) ws = at::empty({nws}, logits.options());
  CHECK_HIP3(lumen::sample_rows(a, nws > 0 ? ws.data_ptr<float>() : nullptr, cur()));
}

// The sampler's verify form (speculative decoding): logits f32 [B * T, V], row b * T + i = input i of
// sequence b, live while i < n_rows[b].  inv_t / top_p / penalty / greedy / seen_slot are per
// sequence [B]; u, in_ids and tok per row [B * T].  Row (b, i) is penalised over b's bitmap slot and
// in_ids[b * T .. b * T + i]; tok of a dead row is -1.  verify_accept then writes n_acc int32 [B]
// and marks in_ids[b * T .. b * T + n_acc[b]] in the slot -- the draw itself marks nothing.
// Guided form: all seven guide tensors or none, as for sample_rows, but g_in is int32 [B * T]: the
// grammar state in which each row draws (-1: unguided).  g_slot and g_state are neither read nor
// written.
void sample_verify_rows(const at::Tensor& logits, int64_t T, const at::Tensor& n_rows, const at::Tensor& inv_t,
                        const at::Tensor& top_p, const at::Tensor& penalty, const at::Tensor& u,
                        const at::Tensor& greedy, const at::Tensor& seen_slot, at::Tensor seen,
                        const at::Tensor& in_ids, at::Tensor tok, at::Tensor n_acc,
                        const c10::optional<at::Tensor>& out_v, const c10::optional<at::Tensor>& out_i,
                        const c10::optional<at::Tensor>& out_lse, const c10::optional<at::Tensor>& g_allow,
                        const c10::optional<at::Tensor>& g_dfa, const c10::optional<at::Tensor>& tok_off,
                        const c10::optional<at::Tensor>& tok_dat, const c10::optional<at::Tensor>& g_slot,
                        const c10::optional<at::Tensor>& g_in, const c10::optional<at::Tensor>& g_state) {
  TORCH_CHECK(logits.is_cuda() && logits.scalar_type() == at::kFloat && logits.dim() == 2 && logits.stride(1) == 1,
              "sample_verify_rows: logits f32 [B * T, V]");
  const int64_t R = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V >= lumen::SAMPLE_K && V < (int64_t(1) << 31), "sample_verify_rows: V >= 64");
  TORCH_CHECK(T >= 1 && T <= lumen::SAMPLE_VERIFY_MAX_T && R % T == 0, "sample_verify_rows: T in 1 .. 8, rows = B * T");
  const int64_t B = R / T;
  TORCH_CHECK(B <= 64, "sample_verify_rows: at most 64 sequences");
  auto vec = [&](const at::Tensor& t, at::ScalarType ty, int64_t n, const char* what) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == ty && t.is_contiguous() && t.numel() == n &&
                t.device() == logits.device(), "sample_verify_rows: ", what);
  };
  vec(n_rows, at::kInt, B, "n_rows int32 [B]");
  vec(inv_t, at::kFloat, B, "inv_t f32 [B]");
  vec(top_p, at::kDouble, B, "top_p f64 [B]");
  vec(penalty, at::kFloat, B, "penalty f32 [B]");
  vec(greedy, at::kInt, B, "greedy int32 [B]");
  vec(seen_slot, at::kInt, B, "seen_slot int32 [B]");
  vec(n_acc, at::kInt, B, "n_acc int32 [B]");
  vec(u, at::kDouble, R, "u f64 [B * T]");
  vec(in_ids, at::kLong, R, "in_ids int64 [B * T]");
  vec(tok, at::kInt, R, "tok int32 [B * T]");
  const int64_t words = (V + 31) / 32;
  TORCH_CHECK(seen.is_cuda() && seen.scalar_type() == at::kInt && seen.is_contiguous() && seen.dim() == 2 &&
              seen.size(1) == words && seen.device() == logits.device(),
              "sample_verify_rows: seen int32 [S, ceil(V / 32)]");
  lumen::SampleArgs a{};
  a.logits = logits.data_ptr<float>(); a.ld = logits.stride(0);
  a.B = (int)B; a.V = (int)V; a.T = (int)T;
  a.n_rows = n_rows.data_ptr<int>(); a.n_acc = n_acc.data_ptr<int>();
  a.inv_t = inv_t.data_ptr<float>(); a.top_p = top_p.data_ptr<double>(); a.penalty = penalty.data_ptr<float>();
  a.u = u.data_ptr<double>(); a.greedy = greedy.data_ptr<int>(); a.seen_slot = seen_slot.data_ptr<int>();
  a.seen = seen.data_ptr<int>(); a.S = (int)seen.size(0); a.words = (int)words;
  a.in_ids = in_ids.data_ptr<int64_t>(); a.tok = tok.data_ptr<int>();
  const bool cand = out_v.has_value() && out_v->defined();
  TORCH_CHECK(cand == (out_i.has_value() && out_i->defined()), "sample_verify_rows: out_v and out_i come together");
  if (cand) {
    vec(*out_v, at::kFloat, R * lumen::SAMPLE_K, "out_v f32 [B * T, 64]");
    vec(*out_i, at::kInt, R * lumen::SAMPLE_K, "out_i int32 [B * T, 64]");
    a.out_v = out_v->data_ptr<float>(); a.out_i = out_i->data_ptr<int>();
  }
  if (out_lse.has_value() && out_lse->defined()) {
    vec(*out_lse, at::kFloat, R, "out_lse f32 [B * T]");
    a.out_lse = out_lse->data_ptr<float>();
  }
  auto has = [](const c10::optional<at::Tensor>& t) { return t.has_value() && t->defined(); };
  const int ng = has(g_allow) + has(g_dfa) + has(tok_off) + has(tok_dat) + has(g_slot) + has(g_in) + has(g_state);
  TORCH_CHECK(ng == 0 || ng == 7, "sample_verify_rows: the guide tensors come together");
  if (ng == 7) {
    auto dev = [&](const at::Tensor& t, at::ScalarType ty, const char* what) {
      TORCH_CHECK(t.is_cuda() && t.device() == logits.device() && t.scalar_type() == ty && t.is_contiguous(),
                  "sample_verify_rows: ", what);
    };
    dev(*g_allow, at::kInt, "g_allow int32 [A, ceil(V / 32)]");
    dev(*g_dfa, at::kShort, "g_dfa int16 [A, 256]");
    dev(*tok_off, at::kInt, "tok_off int32 [V + 1]");
    dev(*tok_dat, at::kByte, "tok_dat uint8");
    dev(*g_state, at::kInt, "g_state int32 [S]");
    dev(*g_slot, at::kInt, "g_slot int32 (not read)");
    vec(*g_in, at::kInt, R, "g_in int32 [B * T]");
    const int64_t A = g_allow->dim() == 2 ? g_allow->size(0) : 0;
    TORCH_CHECK(A >= 1 && A <= 32767 && g_allow->size(1) == words,
                "sample_verify_rows: g_allow int32 [A, ceil(V / 32)], A < 2^15");
    TORCH_CHECK(g_dfa->dim() == 2 && g_dfa->size(0) == A && g_dfa->size(1) == 256,
                "sample_verify_rows: g_dfa int16 [A, 256]");
    TORCH_CHECK(tok_off->numel() == V + 1, "sample_verify_rows: tok_off int32 [V + 1]");
    TORCH_CHECK(g_state->numel() >= 1, "sample_verify_rows: g_state int32 [S]");
    a.g_allow = g_allow->data_ptr<int>(); a.g_dfa = g_dfa->data_ptr<int16_t>();
    a.tok_off = tok_off->data_ptr<int>(); a.tok_dat = tok_dat->data_ptr<uint8_t>();
    a.g_slot = g_slot->data_ptr<int>(); a.g_in = g_in->data_ptr<int>(); a.g_state = g_state->data_ptr<int>();
    a.g_A = (int)A; a.g_S = (int)g_state->numel();
  }
  const at::DeviceGuard g(logits.device());
  const int64_t nws = lumen::sample_ws_floats((int)R, (int)V);
  at::Tensor ws;
  if (nws > 0) ws = at::empty({nws}, logits.options());
  CHECK_HIP3(lumen::sample_rows(a, nws > 0 ? ws.data_ptr<float>() : nullptr, cur()));
}

// int32 CPU values -> int64 device tensor through the kernel arguments (llm.hip:upload_i64)
void upload_small(const at::Tensor& src, at::Tensor out) {
  TORCH_CHECK(!src.is_cuda() && src.scalar_type() == at::kInt && src.is_contiguous(), "upload_small: src int32 CPU");
  TORCH_CHECK(out.is_cuda() && out.scalar_type() == at::kLong && out.is_contiguous() && out.numel() == src.numel(),
              "upload_small: out int64 like src");
  TORCH_CHECK(src.numel() <= lumen::kUploadMax, "upload_small: at most ", lumen::kUploadMax, " values");
  lumen::UploadArgs a;
  memcpy(a.v, src.data_ptr<int32_t>(), (size_t)src.numel() * sizeof(int32_t));
  const at::DeviceGuard g(out.device());
  CHECK_HIP3(lumen::upload_i64(a, out.data_ptr<int64_t>(), (int)src.numel(), cur()));
}

}  // namespace

TORCH_LIBRARY_FRAGMENT(lumen, m) {
  m.def("upload_small(Tensor src, Tensor(o!) out) -> ()");
  m.def("rope_kv(Tensor(a!) qkv, Tensor pos, Tensor cos_sin, Tensor? slots, Tensor(k!) k_cache, Tensor(v!) v_cache, "
        "int H, int Hkv, int D, Tensor? q_gamma=None, Tensor? k_gamma=None, float qk_eps=0.0, "
        "Tensor? mrope_axes=None) -> ()");
  m.def("paged_decode(Tensor q, Tensor(k!) k_cache, Tensor(v!) v_cache, Tensor block_table, Tensor ctx_len, "
        "Tensor(o!) out, int H, int Hkv, float scale, int nsplit, int blocks_per_split, Tensor(p!)? part_o=None, "
        "Tensor(m!)? part_ml=None, Tensor? pos=None, Tensor? cos_sin=None, Tensor? slots=None, Tensor? pf0=None, "
        "Tensor? pf1=None) -> ()");
  m.def("paged_prefill(Tensor q, Tensor k_cache, Tensor v_cache, Tensor blocks, int start_pos, int H, int Hkv, "
        "float scale, Tensor(a!) out) -> ()");
  m.def("paged_verify(Tensor q, Tensor k_cache, Tensor v_cache, Tensor block_table, Tensor ctx_len, Tensor n_rows, "
        "Tensor(o!) out, int T, int H, int Hkv, float scale, int nsplit, int blocks_per_split, "
        "Tensor(p!)? part_o=None, Tensor(m!)? part_ml=None) -> ()");
  m.def("rep_penalty_(Tensor(a!) logits, Tensor ids, Tensor penalty) -> ()");
  m.def("decode_set_dbg(Tensor dbg) -> ()");
  m.def("sample_rows(Tensor logits, Tensor inv_t, Tensor top_p, Tensor penalty, Tensor u, Tensor greedy, "
        "Tensor seen_slot, Tensor(s!) seen, Tensor in_ids, Tensor(o!) out_ids, Tensor(t!) tok, "
        "Tensor(v!)? out_v=None, Tensor(i!)? out_i=None, Tensor(l!)? out_lse=None, Tensor? g_allow=None, "
        "Tensor? g_dfa=None, Tensor? tok_off=None, Tensor? tok_dat=None, Tensor? g_slot=None, Tensor? g_in=None, "
        "Tensor(g!)? g_state=None) -> ()");
  m.def("sample_verify_rows(Tensor logits, int T, Tensor n_rows, Tensor inv_t, Tensor top_p, Tensor penalty, Tensor u, "
        "Tensor greedy, Tensor seen_slot, Tensor(s!) seen, Tensor in_ids, Tensor(t!) tok, Tensor(n!) n_acc, "
        "Tensor(v!)? out_v=None, Tensor(i!)? out_i=None, Tensor(l!)? out_lse=None, Tensor? g_allow=None, "
        "Tensor? g_dfa=None, Tensor? tok_off=None, Tensor? tok_dat=None, Tensor? g_slot=None, Tensor? g_in=None, "
        "Tensor? g_state=None) -> ()");
}

TORCH_LIBRARY_IMPL(lumen, CUDA, m) {
  m.impl("rope_kv", &rope_kv);
  m.impl("paged_decode", &paged_decode);
  m.impl("paged_prefill", &paged_prefill);
  m.impl("paged_verify", &paged_verify);
  m.impl("rep_penalty_", &rep_penalty_);
  m.impl("upload_small", &upload_small);
  m.impl("decode_set_dbg", &decode_set_dbg);
  m.impl("sample_rows", &sample_rows);
  m.impl("sample_verify_rows", &sample_verify_rows);
}
