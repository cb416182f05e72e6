// Weight-only FP8 GEMMs for the LLM decoder (BASELINE config 5: "fp8 CDNA4 MFMA").
//
//   C[M, N] = epi( (A[M, K] . W8[N, K]^T) * scale[n] )
//
// W8 is OCP e4m3fn (gfx950's native fp8, NOT the MI300 fnuz encoding) with one fp32
// scale per output row, A stays bf16.  Every e4m3 value is exactly representable in
// bf16, so each fp8 pair is widened with ONE v_cvt_scalef32_pk_bf16_fp8 (scale 1.0)
// and fed to the bf16 MFMA or v_dot2c_f32_bf16; the per-channel scale is applied once in
// fp32 on the summed tile, as the column multiplier of the shared tails.  Decode GEMMs are
// HBM-bound on W, so halving the weight bytes is the whole point there; prefill keeps bf16
// MFMA throughput with half the weight traffic.
//
// What is specific to fp8 lives here; the pipeline driver, row-GEMV prologue / tail, split-K
// hand-offs and the 16-column kernel are the decode scaffold (gemm_wdec.h), the prefill tile
// is gemm_wtile.h.
//  * gemv_w8_rows_kernel (M <= 4): 1024-wide k steps, 16 fp8 per lane and load, non-temporal.
//  * gemv_w8_mfma_kernel (4 < M <= 16): stripes of 16 * TPW columns on MFMA, its own main loop.
//  * SkinnyFp8 (16 < M <= 32): policy of gemm_skinny_kernel; 64-wide k blocks, one 16-byte
//    load of 16 fp8 widened into two MFMA operands.
//  * W8Tile (M > 32, prefill): policy of gemm_wtile_kernel; a chunk is 8 fp8 (two dwords).
#include "common.h"
#include "gemm_epi.h"
#include "gemm_wdec.h"
#include "gemm_wtile.h"
#include "wq_widen.h"

namespace lumen {

typedef unsigned int u32x2_t __attribute__((ext_vector_type(2)));

// row-streaming decode weights (M <= 4): read once per launch by one CU -> non-temporal
// (8B fp8 single-stream decode 428 -> 452 tok/s, r3).  The batched kernels
// (M > 4) keep the default policy: nt measured 5 % slower there (r3_w8_nt_ab_v1.txt).
template <bool NT>
__device__ __forceinline__ u32x4_t wload(const uint8_t* p) {
  if constexpr (NT) return ld_nt16(p);
  else return *(const u32x4_t*)p;
}

// ============================================================================ decode, 16 < M <= 32
// gemm_skinny_kernel<2, SkinnyFp8>: lane group g owns k in [16g, 16g + 16) of a 64-wide block,
// permuted identically for A and W, so one 16-byte W load feeds two MFMAs.
struct SkinnyFp8 {
  typedef uint8_t wt;
  static constexpr int KB = 64;
  static constexpr bool SCALED = true;
  static __device__ __forceinline__ void frags(const u32x4_t w, bf16x8_t (&f)[2]) { fp8x16_to_bf16(w, f[0], f[1]); }
};

// ============================================================================ decode, 4 < M <= 16
// Batched decode GEMV on MFMA: a workgroup owns a stripe of 16 * TPW output columns and a K
// range (grid.y splits K for narrow N); its 4 waves interleave 64-wide k blocks.  Per k block a
// wave loads the A fragment (16 rows x 32 B per lane group) ONCE and TPW weight fragments, and
// issues 2 * TPW MFMAs: the activations cost 1 / (2 TPW) of the weight bytes in load traffic
// (the one-tile kernel paid 2x the weight bytes in L2 reads of A).  k blocks run as a two-slot
// register pipeline of U-block chunks.  Norm sums of squares and the column scales are loaded
// before the weight stream (vmcnt retires in issue order).
template <int TPW, int U>
__global__ void __launch_bounds__(256) gemv_w8_mfma_kernel(const uint16_t* __restrict__ A, int64_t lda,
                                                           const uint8_t* __restrict__ W, int64_t ldw,
                                                           const float* __restrict__ scale, void* __restrict__ C,
                                                           int64_t ldc, float* __restrict__ ws, uint32_t* __restrict__ cnt,
                                                           int M, int N, int K, int kchunk, GemmEpi ep) {
  constexpr int COLS = 16 * TPW;
  __shared__ float red[4][16][COLS + 1];
  __shared__ float sc_s[COLS];
  __shared__ float rstd_s[16];
  __shared__ int last_s;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * COLS;
  const int k_begin = blockIdx.y * kchunk;
  const int k_end = min(K, k_begin + kchunk);

  // ---- epilogue operands first
  const float scv = scale[min(n0 + (tid % COLS), N - 1)];
  const bool rs_pre = ep.norm && ep.ssq_in != nullptr && ep.ssq_tiles <= 16 * 16;   // K <= 4096
  f32x4_t ssq_v[4];
  if (rs_pre) {   // thread (row tid / 16, part tid % 16): float4 s part, part + 16, ...
    const f32x4_t* p = (const f32x4_t*)(ep.ssq_in + (int64_t)min(tid >> 4, M - 1) * ep.ssq_tiles);
    const int n4 = ep.ssq_tiles >> 2;
#pragma unroll
    for (int j = 0; j < 4; ++j) ssq_v[j] = p[min((tid & 15) + 16 * j, n4 - 1)];
  }

  const uint8_t* wr[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) wr[t] = W + (int64_t)min(n0 + t * 16 + col, N - 1) * ldw + g * 16;
  const bool arow = col < M;
  const uint16_t* ar = A + (int64_t)(arow ? col : 0) * lda + g * 16;
  f32x4_t acc[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  u32x4_t wb[2][U][TPW];
  u32x4_t ab[2][U][2];
  const int nblk = (k_end - k_begin) >> 6;
  const int mine = wid < nblk ? (nblk - wid + 3) >> 2 : 0;   // this wave's k blocks: wid, wid + 4, ...
  auto issue = [&](const int slot, const int j0) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t k = k_begin + (int64_t)(wid + 4 * (j0 + u)) * 64;
#pragma unroll
      for (int t = 0; t < TPW; ++t) wb[slot][u][t] = *(const u32x4_t*)(wr[t] + k);
      ab[slot][u][0] = *(const u32x4_t*)(ar + k);
      ab[slot][u][1] = *(const u32x4_t*)(ar + k + 8);
    }
  };
  auto consume = [&](const int slot, const int nu) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u < nu) {
        const u32x4_t a0 = arow ? ab[slot][u][0] : (u32x4_t){0u, 0u, 0u, 0u};
        const u32x4_t a1 = arow ? ab[slot][u][1] : (u32x4_t){0u, 0u, 0u, 0u};
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
          bf16x8_t f0, f1;
          fp8x16_to_bf16(wb[slot][u][t], f0, f1);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a0), f0, acc[t], 0, 0, 0);
          acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a1), f1, acc[t], 0, 0, 0);
        }
      }
    }
  };
  const int nch = mine / U;
  pipeline2<U>(nch, issue, consume);
  for (int j = nch * U; j < mine; ++j) {   // remainder blocks, one at a time
    const int64_t k = k_begin + (int64_t)(wid + 4 * j) * 64;
#pragma unroll
    for (int t = 0; t < TPW; ++t) wb[0][0][t] = *(const u32x4_t*)(wr[t] + k);
    ab[0][0][0] = *(const u32x4_t*)(ar + k);
    ab[0][0][1] = *(const u32x4_t*)(ar + k + 8);
    consume(0, 1);
  }

  // ---- wave partials -> LDS (C fragment: row 4g + r, column t * 16 + col)
#pragma unroll
  for (int t = 0; t < TPW; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wid][4 * g + r][t * 16 + col] = acc[t][r];
  if (tid < COLS) sc_s[tid] = scv;
  if (ep.norm) {
    if (rs_pre) {
      const int n4 = ep.ssq_tiles >> 2;
      float t = 0.f;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((tid & 15) + 16 * j < n4) t += (ssq_v[j][0] + ssq_v[j][1]) + (ssq_v[j][2] + ssq_v[j][3]);
#pragma unroll
      for (int o = 1; o < 16; o <<= 1) t += __shfl_xor(t, o, 64);
      if ((tid & 15) == 0 && (tid >> 4) < 16) rstd_s[tid >> 4] = rsqrtf(t / (float)K + ep.norm_eps);
    } else {
      skinny_rstd<4>(A, lda, M, K, ep, rstd_s);
    }
  }
  __syncthreads();
  if (!splitk_wide<16, COLS>(red, last_s, ws, cnt, M, N, n0)) return;
  stripe_store<TPW>(red, ws != nullptr ? 1 : 0, rstd_s, sc_s, n0, M, N, C, ldc, ep);
}

// ============================================================================ decode, M <= 4
// Row-streaming GEMV.  Every wave streams whole weight rows: one wave instruction reads 1 KiB
// contiguous of ONE row (lane l: bytes [16 l, 16 l + 16) of a 1024-wide k step).  The k steps
// run as a two-slot register pipeline of U-step chunks (chunk c + 1 is issued before chunk c is
// consumed: up to 2 * U * R * 16 B in flight per lane); each 16 fp8 widen to 8 bf16 pairs
// (v_cvt_scalef32_pk_bf16_fp8) and meet the bf16 activations (L1/L2-resident) in
// v_dot2c_f32_bf16; every (row, m) partial is reduced over the 64 lanes once at the end.
// A workgroup = 4 waves x 4 rows = 16 consecutive output columns, so the decode epilogue
// works on whole 16-column tiles.  Prologue (epilogue operands before the weight stream) and
// tail are the scaffold's (RowPre / row_gemv_tail), the column scales ride along.  No MFMA: at
// M <= 4 the dot products use ~20-40 % of the VALU issue budget while HBM streams.
template <int MR, int U, bool NT>
__global__ void __launch_bounds__(256) gemv_w8_rows_kernel(const uint16_t* __restrict__ A, int64_t lda,
                                                           const uint8_t* __restrict__ W, int64_t ldw,
                                                           const float* __restrict__ scale, void* __restrict__ C,
                                                           int64_t ldc, int M, int N, int K, GemmEpi ep) {
  constexpr int R = 4;
  __shared__ float red[16][MR];
  __shared__ float sc_s[16];
  __shared__ float rstd_s[MR];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = blockIdx.x * 16;

  // ---- epilogue operands first (see RowPre)
  const float scv = scale[min(n0 + (lane & 15), N - 1)];
  RowPre<MR> pre;
  pre.load(ep, M, N, K, n0, lane);

  // ---- weight stream
  const int r0 = n0 + wid * R;
  const uint8_t* wp[R];
#pragma unroll
  for (int r = 0; r < R; ++r) wp[r] = W + (int64_t)min(r0 + r, N - 1) * ldw + lane * 16;
  const uint16_t* ap[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) ap[m] = A + (int64_t)(m < M ? m : 0) * lda + lane * 16;
  float acc[R][MR];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int m = 0; m < MR; ++m) acc[r][m] = 0.f;

  u32x4_t wb[2][U][R];
  u32x4_t ab[2][U][MR][2];
  auto issue = [&](const int slot, const int st0) {   // U full 1024-wide steps
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t ko = (int64_t)(st0 + u) << 10;
#pragma unroll
      for (int r = 0; r < R; ++r) wb[slot][u][r] = wload<NT>(wp[r] + ko);
#pragma unroll
      for (int m = 0; m < MR; ++m) {
        ab[slot][u][m][0] = *(const u32x4_t*)(ap[m] + ko);
        ab[slot][u][m][1] = *(const u32x4_t*)(ap[m] + ko + 8);
      }
    }
  };
  auto consume = [&](const int slot, const int nu) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u < nu) {
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const u32x4_t b0 = fp8x8_to_bf16(wb[slot][u][r][0], wb[slot][u][r][1]);
          const u32x4_t b1 = fp8x8_to_bf16(wb[slot][u][r][2], wb[slot][u][r][3]);
#pragma unroll
          for (int m = 0; m < MR; ++m)
            acc[r][m] = dot8_bf16(b1, ab[slot][u][m][1], dot8_bf16(b0, ab[slot][u][m][0], acc[r][m]));
        }
      }
    }
  };
  const int nfull = K >> 10;
  const int nch = nfull / U;
  pipeline2<U>(nch, issue, consume);
  // remainder: full steps past the last chunk, then the partial step (K % 1024; Qwen2: 896,
  // 4864), whose lanes past K load a clamped in-row address and zero their activations
  for (int st = nch * U; st < nfull; ++st) {
    const int64_t ko = (int64_t)st << 10;
#pragma unroll
    for (int r = 0; r < R; ++r) wb[0][0][r] = wload<NT>(wp[r] + ko);
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      ab[0][0][m][0] = *(const u32x4_t*)(ap[m] + ko);
      ab[0][0][m][1] = *(const u32x4_t*)(ap[m] + ko + 8);
    }
    consume(0, 1);
  }
  if ((K & 1023) != 0) {
    const int k = (nfull << 10) + lane * 16;
    const bool ok = k < K;
    const int64_t ko = ok ? k - lane * 16 : K - 16 - lane * 16;
#pragma unroll
    for (int r = 0; r < R; ++r) wb[0][0][r] = wload<NT>(wp[r] + ko);
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      const u32x4_t a0 = *(const u32x4_t*)(ap[m] + ko), a1 = *(const u32x4_t*)(ap[m] + ko + 8);
      ab[0][0][m][0] = ok ? a0 : (u32x4_t){0u, 0u, 0u, 0u};
      ab[0][0][m][1] = ok ? a1 : (u32x4_t){0u, 0u, 0u, 0u};
    }
    consume(0, 1);
  }

  if (tid < 16) sc_s[tid] = scv;
  row_gemv_tail<MR>(acc, pre, red, rstd_s, (const float*)sc_s, A, lda, C, ldc, M, N, K, n0, ep);
}

// ============================================================================ prefill
// gemm_wtile_kernel with an fp8 W tile: 8 fp8 per chunk, K % 64 == 0.
struct W8Tile {
  typedef float param_t;
  typedef u32x2_t chunk_t;
  typedef const uint8_t* src_t;
  static constexpr bool KTAIL = false, COLSCALE = true;
  const uint8_t* W;
  int64_t ldw;
  const float* scale;
  __device__ __forceinline__ W8Tile(const uint8_t* W_, int64_t ldw_, const float* scale_, int64_t, int)
      : W(W_), ldw(ldw_), scale(scale_) {}
  __device__ __forceinline__ src_t src(const int64_t n, const int c) const { return W + n * ldw + c * 8; }
  __device__ __forceinline__ chunk_t load(const src_t s, const int koff) const { return *(const u32x2_t*)(s + koff); }
  static __device__ __forceinline__ u32x4_t widen(const chunk_t w) { return fp8x8_to_bf16(w[0], w[1]); }
  __device__ __forceinline__ float colscale(const int n) const { return scale[n]; }
};

int skinny_ksplit(int N, int K);

// Decode plan for fp8 weights, 4 < M <= 32 (M <= 4 runs the unsplit row-streaming GEMV):
// M <= 16: column stripes of 64 / 32 / 16 (N divisibility), K split so that stripes x splits
// reach ~512 workgroups (2 per CU), every split >= 4 k blocks (one per wave);
// 16 < M <= 32: 16-column tiles, the skinny split heuristic.
DecPlan w8_dec_plan(int M, int N, int K) {
  if (M <= 4) return DecPlan{1, 1, K};
  if (M <= 16) return dec_plan_stripes(N, K, N % 64 == 0 ? 4 : (N % 32 == 0 ? 2 : 1), 64, 256);
  DecPlan p{1, 1, K};
  const int ks = skinny_ksplit(N, K);
  int kchunk = (K + ks - 1) / ks;
  kchunk = (kchunk + 255) / 256 * 256;   // whole 64-wide blocks for every wave
  p.ks = (K + kchunk - 1) / kchunk;
  if (p.ks > 1) p.kchunk = kchunk;
  return p;
}

hipError_t gemm_w8(const uint16_t* A, int64_t lda, const uint8_t* W, int64_t ldw, const float* scale, void* C,
                   int64_t ldc, int M, int N, int K, const GemmEpi& ep, float* ws, uint32_t* cnt, int ksplit,
                   hipStream_t stream) {
  if (K % 64 != 0 || M <= 0) return hipErrorInvalidValue;
  if (M <= 4) {   // row-streaming GEMV, non-temporal weight loads
    const dim3 grid((N + 15) / 16);
#define ROWS_LAUNCH(MR_, U_)                                                                                      \
  hipLaunchKernelGGL((gemv_w8_rows_kernel<MR_, U_, true>), grid, dim3(256), 0, stream, A, lda, W, ldw, scale, C, \
                     ldc, M, N, K, ep)
    if (M == 1) ROWS_LAUNCH(1, 2);
    else if (M == 2) ROWS_LAUNCH(2, 2);
    else ROWS_LAUNCH(4, 1);
#undef ROWS_LAUNCH
    return hipGetLastError();
  }
  if (M <= 32) {
    const DecPlan pl = w8_dec_plan(M, N, K);
    if (pl.ks > 1 && pl.ks != ksplit) return hipErrorInvalidValue;   // host sized ws / counters for its plan
    const int gy = pl.ks;
    if (gy > 1 && (ws == nullptr || cnt == nullptr)) return hipErrorInvalidValue;
    float* w = gy > 1 ? ws : nullptr;
    if (M <= 16) {
      const dim3 grid((N + 16 * pl.tpw - 1) / (16 * pl.tpw), gy);
#define MFMA_LAUNCH(T_)                                                                                          \
  hipLaunchKernelGGL((gemv_w8_mfma_kernel<T_, 2>), grid, dim3(256), 0, stream, A, lda, W, ldw, scale, C, ldc, w, cnt, \
                     M, N, K, pl.kchunk, ep)
      if (pl.tpw == 4) MFMA_LAUNCH(4);
      else if (pl.tpw == 2) MFMA_LAUNCH(2);
      else MFMA_LAUNCH(1);
#undef MFMA_LAUNCH
    } else {
      hipLaunchKernelGGL((gemm_skinny_kernel<2, SkinnyFp8>), dim3((N + 15) / 16, gy), dim3(256), 0, stream, A, lda, W,
                         ldw, scale, C, ldc, w, cnt, M, N, K, pl.kchunk, ep);
    }
    return hipGetLastError();
  }
  const int64_t t128 = (int64_t)((M + 127) / 128) * ((N + 127) / 128);
  if (t128 >= 256)
    return launch_wtile<128, 128, 2, 2, W8Tile>(A, lda, W, ldw, scale, 0, 0, C, ldc, M, N, K, ep, stream);
  return launch_wtile<64, 64, 2, 2, W8Tile>(A, lda, W, ldw, scale, 0, 0, C, ldc, M, N, K, ep, stream);
}

}  // namespace lumen
