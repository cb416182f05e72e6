// Row top-k with fused softmax statistics, for zero-shot label-bank
// classification (CLIP / BioCLIP / scene) and vocab sampling candidates.
//
// scores [B, N] fp32 (the MFMA GEMM of query embeddings against the label bank)
// -> top-k values / indices per row (descending) and the row log-sum-exp of
// (scale * scores), so softmax probabilities of the winners are
// exp(scale*s - lse) without a second pass over N.
//
// One workgroup per row (chunk): every thread streams a strided slice keeping a
// sorted register list of its K best (compile-time K, unrolled compare-swap
// insertion) and an online (max, sum-exp); the block then merges by K rounds of a
// block arg-max over the list heads.  Long rows (LLM vocabularies, 128-152 k
// logits, or million-label banks) run in two phases so a single row still fills
// the GPU: phase 1 = one workgroup per (row, 4096-column chunk) writing k
// candidates + the chunk's (max, sum-exp); phase 2 = one workgroup per row merging
// the candidates (original indices carried along) and the partial statistics.
//
// Replaces the numpy `np.dot / softmax / argsort[::-1][:top_k]` of
// packages/lumen-clip/src/lumen_clip/general_clip/clip_model.py:289-315 and the
// raw-cosine top-k of expert_bioclip/bioclip_model.py:313-316.
#include "topk_core.h"

namespace lumen {

// the workgroup body lives in topk_core.h (shared with the vocab sampler, sampler.hip)
template <int K>
__global__ void __launch_bounds__(256)
row_topk_kernel(const float* __restrict__ scores, int64_t ld, int N, int k, float scale, float* __restrict__ out_v,
                int* __restrict__ out_i, float* __restrict__ out_lse, int index_offset, const int* __restrict__ in_idx,
                const float* __restrict__ in_ml, int nparts, int chunk, float* __restrict__ out_ml) {
  TopkStore sink{out_v, out_i, ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * k, index_offset};
  topk_block<K>(scores, ld, N, k, scale, out_lse, in_idx, in_ml, nparts, chunk, out_ml, out_lse != nullptr,
                TopkIdentity{}, sink);
}

template <int K>
static void launch_topk(dim3 grid, hipStream_t stream, const float* scores, int64_t ld, int N, int k, float scale,
                        float* out_v, int* out_i, float* out_lse, int index_offset, const int* in_idx,
                        const float* in_ml, int nparts, int chunk, float* out_ml) {
  hipLaunchKernelGGL(row_topk_kernel<K>, grid, dim3(256), 0, stream, scores, ld, N, k, scale, out_v, out_i, out_lse,
                     index_offset, in_idx, in_ml, nparts, chunk, out_ml);
}

static hipError_t topk_dispatch(dim3 grid, hipStream_t stream, const float* scores, int64_t ld, int N, int k,
                                float scale, float* out_v, int* out_i, float* out_lse, int index_offset,
                                const int* in_idx, const float* in_ml, int nparts, int chunk, float* out_ml) {
  if (k <= 8) launch_topk<8>(grid, stream, scores, ld, N, k, scale, out_v, out_i, out_lse, index_offset, in_idx, in_ml, nparts, chunk, out_ml);
  else if (k <= 16) launch_topk<16>(grid, stream, scores, ld, N, k, scale, out_v, out_i, out_lse, index_offset, in_idx, in_ml, nparts, chunk, out_ml);
  else if (k <= 32) launch_topk<32>(grid, stream, scores, ld, N, k, scale, out_v, out_i, out_lse, index_offset, in_idx, in_ml, nparts, chunk, out_ml);
  else if (k <= 64) launch_topk<64>(grid, stream, scores, ld, N, k, scale, out_v, out_i, out_lse, index_offset, in_idx, in_ml, nparts, chunk, out_ml);
  else return hipErrorInvalidValue;
  return hipGetLastError();
}

int topk_chunks(int N) { return N > 16384 ? (N + TOPK_CHUNK - 1) / TOPK_CHUNK : 1; }

// ws: float [B * nch * (2k + 2)] (candidate values, candidate indices as int bits, partial (m, l))
hipError_t row_topk(const float* scores, int64_t ld, int B, int N, int k, float scale, float* out_v, int* out_i,
                    float* out_lse, int index_offset, float* ws, hipStream_t stream) {
  const int nch = topk_chunks(N);
  if (nch == 1 || ws == nullptr)
    return topk_dispatch(dim3(B, 1), stream, scores, ld, N, k, scale, out_v, out_i, out_lse, index_offset, nullptr,
                         nullptr, 1, N, nullptr);
  float* cv = ws;
  int* ci = reinterpret_cast<int*>(ws + (int64_t)B * nch * k);
  float* pml = ws + (int64_t)B * nch * k * 2;
  hipError_t e = topk_dispatch(dim3(B, nch), stream, scores, ld, N, k, scale, cv, ci, nullptr, 0, nullptr, nullptr, 1,
                               TOPK_CHUNK, pml);
  if (e != hipSuccess) return e;
  return topk_dispatch(dim3(B, 1), stream, cv, (int64_t)nch * k, nch * k, k, 1.f, out_v, out_i, out_lse,
                       index_offset, ci, pml, nch, nch * k, nullptr);
}

}  // namespace lumen
