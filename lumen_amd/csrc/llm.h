// Decoder-LLM kernels (llm.hip) shared with their torch bindings (ops_llm.cpp).
//
// Paged KV cache layout (block = 64 tokens of one sequence):
//   k_cache [num_blocks, Hkv, 64, D]   token-major rows: the S^T = K Q^T MFMA A-operand
//                                      reads 16-byte pieces of K rows directly from HBM
//   v_cache [num_blocks, Hkv, D, 64]   transposed (d-major): the O^T = V^T P^T A-operand
//                                      needs 8 consecutive tokens of one d -> one 16-byte load
// Either bf16 or OCP e4m3fn (LUMEN_KV_DTYPE=fp8: half the bytes per token; 8-byte loads widened
// to bf16 fragments in registers, unit scale, values saturated to +-448 on write).
// so the decode kernel streams both straight from global memory into MFMA
// fragments with no LDS staging and no transposing reads.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace lumen {

constexpr int KV_BLOCK = 64;

struct RopeKVArgs {
  uint16_t* qkv;          // [T, ld] bf16: q heads | k heads | v heads (rotated in place)
  int64_t ld;
  const int* pos;         // [T] positions ([3, T] with mrope, below)
  const float* cos_sin;   // [max_pos, D/2, 2] (cos, sin)
  const int64_t* slots;   // [T] cache slot = block * 64 + offset, < 0 = do not cache; null = no cache write
  uint16_t* k_cache;
  uint16_t* v_cache;
  int T, H, Hkv, D;
  int kv_fp8;             // caches hold OCP e4m3fn bytes (unit scale, saturated) instead of bf16
  // per-head q / k RMSNorm before the rotation (Qwen3): y = x * rsqrt(mean(x^2) + eps) * gamma over
  // each head's D elements in fp32, one bf16 rounding after the rotation.  D = 32 / 64 / 128.
  const float* q_gamma;   // [D] shared by all q heads (null = no norm; then k_gamma is null too)
  const float* k_gamma;   // [D] shared by all k heads
  float eps;
  // multimodal RoPE (Qwen-VL prefill): pos is [3, T] axis-major (temporal, height, width) and rotary
  // frequency i takes its (cos, sin) from row pos[axis(i)][t] of the table.  axis(i) is the two-bit
  // code i % 32 of mrope_axes[i / 32] (0 = t, 1 = h, 2 = w); D <= 128, so 64 codes cover every i.
  int mrope;              // 0: pos is [T] and the two words below are not read
  uint64_t mrope_axes[2];
};
hipError_t rope_kv(const RopeKVArgs& a, hipStream_t stream);

struct DecodeArgs {
  const uint16_t* q;      // [B, q_sb] rows; head h at h * D
  int64_t q_sb;
  const uint16_t* k_cache;
  const uint16_t* v_cache;
  const int* block_table; // [B, bt_stride]
  int bt_stride;
  const int* ctx_len;     // [B] tokens in cache (including the current one)
  uint16_t* o;            // [B, o_sb] rows; head h at h * D
  int64_t o_sb;
  float* part_o;          // [B, H, nsplit, D]   (nsplit > 1)
  float* part_ml;         // [B, H, nsplit, 2]
  int H, Hkv, nsplit, blocks_per_split;
  float scale_log2;
  // fused RoPE + cache write (decode, D = 64 / 128): q comes unrotated from the QKV projection
  // and is rotated in registers; the split owning the sequence's last block takes the current
  // token's k (rotated) and v from registers for its own attention and writes them to slots[b]
  // after its attention loop (fire-and-forget: the next decode step is the first to read them)
  const int* pos;         // [B] positions (null = q / cache already prepared by rope_kv)
  const float* cos_sin;   // [max_pos, D/2, 2]
  const int64_t* slots;   // [B]
  uint16_t* k_cache_w;    // writable views of the caches
  uint16_t* v_cache_w;
  int kv_fp8;             // caches hold e4m3fn bytes: widened to bf16 on load (cvt_scalef32_pk_bf16_fp8)
  uint32_t* split_cnt;    // [B, Hkv] zeroed tickets of the in-launch split combine (nsplit > 1; nsplit <= 32)
  // Weight prefetch into the Infinity Cache: workgroups beyond the attention grid (grid.z >= B)
  // read these bytes with default-policy loads and drop them, so the GEMV that runs next (the
  // o projection) streams its weights from the 256 MiB MALL instead of HBM while the attention
  // itself occupies only a few dozen CUs.  null / 0 = none.
  const uint8_t* pf[2];
  int64_t pf_bytes[2];
  // profiling only (tools/decode_attn_timeline.py): per-workgroup s_memrealtime stamps [B, Hkv, nsplit, 8]
  int64_t* dbg;
};
hipError_t paged_decode(const DecodeArgs& a, int B, int D, hipStream_t stream);

// Prefill attention of T new rows of ONE sequence over its paged cache (chunked prefill, prefix
// reuse): query row i sits at position start_pos + i and attends cache tokens 0 .. start_pos + i;
// the chunk's own k / v are already in the cache (rope_kv runs first).
struct PrefillArgs {
  const uint16_t* q;      // [T, q_ld] rotated packed QKV rows; head h at h * D
  int64_t q_ld;
  const uint16_t* k_cache;
  const uint16_t* v_cache;
  const int64_t* blocks;  // the sequence's block list, >= ceil((start_pos + T) / 64) entries
  uint16_t* o;            // [T, o_ld] rows; head h at h * D
  int64_t o_ld;
  int start_pos, T, H, Hkv;
  int num_blocks;         // pool size (block ids are clamped to it)
  float scale_log2;
  int kv_fp8;
};
hipError_t paged_prefill(const PrefillArgs& a, int D, hipStream_t stream);

// Verify attention (speculative decoding): up to T new rows for each of B sequences over the
// paged cache in one launch.  Row i of sequence b (q / o row b * T + i) sits at position
// ctx_len[b] - n_rows[b] + i and attends cache tokens 0 .. that position; rows i >= n_rows[b] are
// padding and come out 0.  The rows' own k / v are already in the cache (rope_kv runs first).
// Block table, ctx_len and n_rows are read on the device, so a captured launch serves any step.
// T * (H / Hkv) <= 64.
struct VerifyArgs {
  const uint16_t* q;      // [B * T, q_ld] rotated packed QKV rows; head h at h * D
  int64_t q_ld;
  const uint16_t* k_cache;
  const uint16_t* v_cache;
  const int* block_table; // [B, bt_stride], bt_width entries per row (clamped into the pool)
  int bt_stride, bt_width;
  const int* ctx_len;     // [B] tokens in the cache including this step's n_rows[b] rows
  const int* n_rows;      // [B] live rows, 1 .. T
  uint16_t* o;            // [B * T, o_ld] rows; head h at h * D
  int64_t o_ld;
  float* part_o;          // [B * T, H, nsplit, D]   (nsplit > 1)
  float* part_ml;         // [B * T, H, nsplit, 2]
  uint32_t* split_cnt;    // [B, Hkv] zeroed tickets of the in-launch split combine (nsplit > 1)
  int T, H, Hkv, nsplit, blocks_per_split;   // split policy as DecodeArgs
  int num_blocks;         // pool size
  float scale_log2;
  int kv_fp8;
};
hipError_t paged_verify(const VerifyArgs& a, int B, int D, hipStream_t stream);

hipError_t rep_penalty(float* logits, int64_t ld, const int* ids, int maxn, const float* penalty, int B, int V,
                       hipStream_t stream);

// <= kUploadMax int32 values -> int64 device array, carried in the kernel arguments
constexpr int kUploadMax = 896;
struct UploadArgs {
  int32_t v[kUploadMax];
};
hipError_t upload_i64(const UploadArgs& a, int64_t* out, int n, hipStream_t stream);

}  // namespace lumen
