// Skinny GEMM for decode: C[M, N] = epi(A[M, K] . W[N, K]^T) with M <= 32.
//
// Decode GEMMs are HBM-bound on W (every weight byte is read once per token), so
// the kernel is shaped for bandwidth, not reuse:
//   * a workgroup owns one 16-column N tile and a K range; its 4 waves take
//     interleaved 32-wide k-steps of that range (split-K inside the workgroup,
//     reduced through LDS), and grid.y splits K across workgroups only when the N
//     tiles alone leave CUs idle (skinny_ksplit: N >= 4096 runs unsplit, narrow N such
//     as 896 splits up to ~1024 workgroups; each K-split writes its fp32 partial
//     slab; the last split of a tile to arrive — per-tile atomic counter — sums the
//     slabs in split order — deterministic, so hipGraph replays and eager launches
//     give bitwise-identical logits — and applies the epilogue, with no second
//     kernel launch);
//   * both MFMA operands come straight from global memory in fragment layout:
//     B = W^T (lane: 16 contiguous bytes of weight row n0 + (lane & 15)), A = the
//     activations (L2-resident, shared by every workgroup), 16 rows per MFMA row
//     tile, rows >= M zero;
//   * 4 k-steps are loaded before any MFMA issues (64 B of W in flight per lane).
// The epilogue is the shared GemmEpi (bias / act / residual / SwiGLU / f32 out).
// The kernel is gemm_skinny_kernel<MT, W> of the decode scaffold (gemm_wdec.h) with the bf16
// weight policy below; fp8 weights run the same kernel with their own policy (gemm_w8.hip).
#include "common.h"
#include "gemm_epi.h"
#include "gemm_wdec.h"

namespace lumen {

// 32-wide k blocks: the 16 loaded bytes are the MFMA operand.
struct SkinnyBf16 {
  typedef uint16_t wt;
  static constexpr int KB = 32;
  static constexpr bool SCALED = false;
  static __device__ __forceinline__ void frags(const u32x4_t w, bf16x8_t (&f)[1]) { f[0] = __builtin_bit_cast(bf16x8_t, w); }
};

// K split per shape: when the 16-column N tiles already cover every CU (ntiles >= 256,
// all four Llama-3-8B decode GEMMs) the split only adds slab traffic and is skipped;
// narrower N (FastVLM-0.5B: 896 / 1152 wide) splits K until the grid reaches ~target
// workgroups, each keeping >= 512 of K.
int skinny_ksplit(int N, int K) {
  const int ntiles = (N + 15) / 16;
  constexpr int target = 1024;
  constexpr int full = 256;   // tile count that already fills the chip without a split
  if (ntiles >= full) return 1;
  int ks = (target + ntiles - 1) / ntiles;
  const int kmax = K / 512 > 1 ? K / 512 : 1;
  ks = ks < kmax ? ks : kmax;
  ks = ks > 1 ? ks : 1;
  return ks;
}

hipError_t gemm_skinny(const uint16_t* A, int64_t lda, const uint16_t* W, int64_t ldw, void* C, int64_t ldc, int M,
                       int N, int K, const GemmEpi& ep, float* ws, uint32_t* cnt, int ksplit, hipStream_t stream) {
  if (M <= 0 || M > 32 || K % 32 != 0) return hipErrorInvalidValue;
  // K chunk per workgroup: a multiple of 32 * 4 waves
  int kchunk = (K + ksplit - 1) / ksplit;
  kchunk = (kchunk + 127) / 128 * 128;
  const int gy = (K + kchunk - 1) / kchunk;
  dim3 grid((N + 15) / 16, gy), block(256);
  float* w = gy > 1 ? ws : nullptr;
  if (gy > 1 && ws == nullptr) return hipErrorInvalidValue;
  if (gy > 1 && cnt == nullptr) return hipErrorInvalidValue;
  if (M <= 16)
    hipLaunchKernelGGL((gemm_skinny_kernel<1, SkinnyBf16>), grid, block, 0, stream, A, lda, W, ldw, (const float*)nullptr,
                       C, ldc, w, cnt, M, N, K, kchunk, ep);
  else
    hipLaunchKernelGGL((gemm_skinny_kernel<2, SkinnyBf16>), grid, block, 0, stream, A, lda, W, ldw, (const float*)nullptr,
                       C, ldc, w, cnt, M, N, K, kchunk, ep);
  return hipGetLastError();
}

}  // namespace lumen
