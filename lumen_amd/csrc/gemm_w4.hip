// Weight-only 4-bit group-quantised GEMMs for the LLM decoder.
//
//   C[M, N] = epi( A[M, K] . dq(W4)[N, K]^T ),   dq(W4)[n, k] = code[n, k] * scale[n, k / G] + wmin[n, k / G]
//
// A stays bf16, accumulation is fp32.  W4 is uint8 [N, K / 2] with two codes (0..15) per byte;
// the physical nibble order IS the logical (MatMulNBits) one -- byte j of a row holds k = 2 j in
// its low nibble and k = 2 j + 1 in its high nibble -- so the packer / unpacker of
// lumen_amd.ops permute nothing.  The group parameters are fp16 [N, K / G, 2] = (scale, wmin),
// one 4-byte load per group, G in {32, 128}.  Decode GEMMs are HBM-bound on the weight bytes:
// 4 bits + 32 / G bits of parameters per weight instead of fp8's 8.
//
// What is specific to 4-bit groups lives here; the pipeline driver, row-GEMV prologue / tail and
// split-K hand-off are the decode scaffold (gemm_wdec.h), the prefill tile is gemm_wtile.h.
//  * gemv_w4_rows_kernel (M <= 4): 2048-wide k steps.  A lane's 16-byte load carries 32 k
//    values = (a quarter of) one group; its (scale, wmin) dword is loaded with it.  The codes
//    never become weights: a dword's nibbles i and i + 4 are masked into one bf16 pair
//    (0x4300 | c = 128 + c exactly), the activations are paired the same way,
//    and with d = sum a_k (128 + c_k), sa = sum a_k over the lane's 32 k
//        sum a_k (c_k scale + wmin) = scale * d + (wmin - 128 scale) * sa      (fp32).
//  * gemm_skinny_w4_kernel (4 < M <= 32): split-K MFMA kernel; lane group g owns k in
//    [32 g, 32 g + 32) of a 128-wide block (identically for A and W), so one 16-byte W load
//    feeds four 16x16x32 MFMAs.  G = 128: the exact codes go into the MFMA and the group
//    parameters scale the block's partial sums; G = 32: codes are widened in registers,
//    bf16(code * scale + wmin), one fp32 fma per weight.
//  * W4Tile (M > 32, prefill): policy of gemm_wtile_kernel; a chunk of 8 codes (one dword) and
//    its group's parameter dword; K % 64 == 32 (G = 32 shards) runs as a zero-filled K tail.
#include "common.h"
#include "gemm_w4.h"
#include "gemm_wdec.h"
#include "gemm_wtile.h"
#include "wq_widen.h"

namespace lumen {

// ============================================================================ decode, M <= 4
// Every wave streams whole weight rows: one wave instruction reads 1 KiB contiguous of ONE row
// (lane l: bytes [16 l, 16 l + 16) = k in [32 l, 32 l + 32) of a 2048-wide k step).  Rows
// shorter than a step (K = 896: 448 bytes) and K tails run in the partial step, whose lanes
// past K load a clamped in-row address and zero their activations.  Epilogue operands are
// loaded before the weight stream (vmcnt retires in issue order).
template <int MR, int U>
__global__ void __launch_bounds__(256) gemv_w4_rows_kernel(const uint16_t* __restrict__ A, int64_t lda,
                                                           const uint8_t* __restrict__ W, int64_t ldw,
                                                           const uint32_t* __restrict__ P, int64_t ldp, int gshift,
                                                           void* __restrict__ C, int64_t ldc, int M, int N, int K,
                                                           GemmEpi ep) {
  constexpr int R = 4;
  __shared__ float red[16][MR];
  __shared__ float rstd_s[MR];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int n0 = blockIdx.x * 16;

  RowPre<MR> pre;   // epilogue operands first
  pre.load(ep, M, N, K, n0, lane);

  // ---- weight stream
  const int r0 = n0 + wid * R;
  const uint8_t* wp[R];
  const uint32_t* pp[R];
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int64_t row = min(r0 + r, N - 1);
    wp[r] = W + row * ldw + lane * 16;
    pp[r] = P + row * ldp;
  }
  const uint16_t* ap[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) ap[m] = A + (int64_t)(m < M ? m : 0) * lda + lane * 32;
  float acc[R][MR];
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int m = 0; m < MR; ++m) acc[r][m] = 0.f;

  u32x4_t wb[2][U][R];
  uint32_t pb[2][U][R];
  u32x4_t ab[2][U][MR][4];
  auto issue = [&](const int slot, const int st0) {   // U full 2048-wide steps
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int64_t kb = (int64_t)(st0 + u) << 10;           // byte offset in the W row
      const int kg = (((st0 + u) << 11) + lane * 32) >> gshift;
#pragma unroll
      for (int r = 0; r < R; ++r) {
        wb[slot][u][r] = ld_nt16(wp[r] + kb);
        pb[slot][u][r] = pp[r][kg];
      }
#pragma unroll
      for (int m = 0; m < MR; ++m)
#pragma unroll
        for (int j = 0; j < 4; ++j) ab[slot][u][m][j] = *(const u32x4_t*)(ap[m] + 2 * kb + 8 * j);
    }
  };
  auto consume = [&](const int slot, const int nu) {
    const u32x4_t ones = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (u < nu) {
        // activation side, shared by the R rows: pairs (a_i, a_i+4) of every 8, and the sum
        u32x4_t q[MR][4];
        float sa[MR];
#pragma unroll
        for (int m = 0; m < MR; ++m) {
          sa[m] = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const u32x4_t a = ab[slot][u][m][j];
            q[m][j] = (u32x4_t){(a[0] & 0xffffu) | (a[2] << 16), (a[0] >> 16) | (a[2] & 0xffff0000u),
                                (a[1] & 0xffffu) | (a[3] << 16), (a[1] >> 16) | (a[3] & 0xffff0000u)};
            sa[m] = dot8_bf16(a, ones, sa[m]);
          }
        }
#pragma unroll
        for (int r = 0; r < R; ++r) {
          const float s = h2f_lo(pb[slot][u][r]), off = h2f_hi(pb[slot][u][r]) - 128.f * s;
          float d[MR];
#pragma unroll
          for (int m = 0; m < MR; ++m) d[m] = 0.f;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t w = wb[slot][u][r][j];
            const u32x4_t e = {(w & 0x000f000fu) | 0x43004300u, ((w >> 4) & 0x000f000fu) | 0x43004300u,
                               ((w >> 8) & 0x000f000fu) | 0x43004300u, ((w >> 12) & 0x000f000fu) | 0x43004300u};
#pragma unroll
            for (int m = 0; m < MR; ++m) d[m] = dot8_bf16(e, q[m][j], d[m]);
          }
#pragma unroll
          for (int m = 0; m < MR; ++m) acc[r][m] += fmaf(s, d[m], off * sa[m]);
        }
      }
    }
  };
  const int nfull = K >> 11;
  const int nch = nfull / U;
  pipeline2<U>(nch, issue, consume);
  // remainder: full steps past the last chunk, then the partial step (K % 2048)
  for (int st = nch * U; st < nfull; ++st) {
    const int64_t kb = (int64_t)st << 10;
    const int kg = ((st << 11) + lane * 32) >> gshift;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      wb[0][0][r] = ld_nt16(wp[r] + kb);
      pb[0][0][r] = pp[r][kg];
    }
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
      for (int j = 0; j < 4; ++j) ab[0][0][m][j] = *(const u32x4_t*)(ap[m] + 2 * kb + 8 * j);
    consume(0, 1);
  }
  if ((K & 2047) != 0) {
    const int k = (nfull << 11) + lane * 32;
    const bool ok = k < K;
    const int kc = ok ? k : K - 32;                  // this lane's (clamped) first k
    const int64_t kb = (kc >> 1) - lane * 16;        // relative to wp (row + 16 lane)
    const int64_t ka = kc - lane * 32;               // relative to ap (row + 32 lane)
    const int kg = kc >> gshift;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      wb[0][0][r] = ld_nt16(wp[r] + kb);
      pb[0][0][r] = pp[r][kg];
    }
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const u32x4_t a = *(const u32x4_t*)(ap[m] + ka + 8 * j);
        ab[0][0][m][j] = ok ? a : (u32x4_t){0u, 0u, 0u, 0u};
      }
    consume(0, 1);
  }

  row_gemv_tail<MR>(acc, pre, red, rstd_s, NoColScale{}, A, lda, C, ldc, M, N, K, n0, ep);
}

// ============================================================================ decode, 4 < M <= 32
// MT 16-row MFMA tiles x TPW 16-column tiles per wave: a workgroup owns a stripe of 16 * TPW
// output columns and a K range (grid.y splits K for narrow N, in-launch reduction); its 4 waves
// interleave 128-wide k blocks, UNR in flight per wave.  Lane (col, g) owns k in
// [32 g, 32 g + 32) of a block for A row col and W rows n0 + 16 t + col: per block the A
// fragment (64 B per lane and row tile) is loaded ONCE for the TPW weight fragments, each one
// 16-byte W load + one parameter dword feeding four MFMAs.
//   G = 128 (G128): a block is exactly one group for every lane of a column, so the codes go
//   into the MFMA as exact bf16 (0x4300 | c = 128 + c; pairs (k i, k i + 4) of a dword, the A
//   pairs permuted identically) and the group parameters scale the block's partial sums:
//       acc += scale * (A . (128 + c)) + (wmin - 128 scale) * rowsum(A)      (lane-local: a
//   lane's accumulator column is its own W row), rowsum(A) from one more MFMA against ones.
//   G = 32: the four lane groups of an MFMA meet four different groups; codes are widened to
//   bf16(code * scale + wmin) in registers (one fp32 fma per weight).
// A block past the K range loads a clamped address and zeroes A.
template <int MT, int TPW, bool G128>
__global__ void __launch_bounds__(256) gemm_skinny_w4_kernel(const uint16_t* __restrict__ A, int64_t lda,
                                                             const uint8_t* __restrict__ W, int64_t ldw,
                                                             const uint32_t* __restrict__ P, int64_t ldp, int gshift,
                                                             void* __restrict__ C, int64_t ldc, float* __restrict__ ws,
                                                             uint32_t* __restrict__ cnt, int M, int N, int K, int kchunk,
                                                             GemmEpi ep) {
  constexpr int NWV = 4, UNR = 2, COLS = 16 * TPW, ROWS = 16 * MT;
  __shared__ float red[NWV][ROWS][COLS + 1];
  __shared__ float rstd_s[ROWS];
  __shared__ int last_s;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * COLS;
  const int k_begin = blockIdx.y * kchunk;
  const int k_end = min(K, k_begin + kchunk);
  const uint8_t* wr[TPW];
  const uint32_t* pr[TPW];
#pragma unroll
  for (int t = 0; t < TPW; ++t) {
    const int64_t nrow = min(n0 + t * 16 + col, N - 1);
    wr[t] = W + nrow * ldw;
    pr[t] = P + nrow * ldp;
  }
  const uint16_t* ar[MT];
  bool av[MT];
#pragma unroll
  for (int i = 0; i < MT; ++i) {
    const int m = i * 16 + col;
    av[i] = m < M;
    ar[i] = A + (int64_t)(av[i] ? m : 0) * lda;
  }
  f32x4_t acc[MT][TPW];
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int t = 0; t < TPW; ++t) acc[i][t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  const int nblk = (k_end - k_begin + 127) >> 7;
  for (int s = wid; s < nblk; s += NWV * UNR) {
    u32x4_t wf[UNR][TPW];
    uint32_t pf[UNR][TPW];
    u32x4_t af[UNR][MT][4];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int k = k_begin + (s + NWV * u) * 128 + 32 * g;
      const bool ok = k < k_end;
      const int kc = ok ? k : k_begin;
#pragma unroll
      for (int t = 0; t < TPW; ++t) {
        wf[u][t] = *(const u32x4_t*)(wr[t] + (kc >> 1));
        pf[u][t] = pr[t][kc >> gshift];
      }
#pragma unroll
      for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const u32x4_t a = *(const u32x4_t*)(ar[i] + kc + 8 * j);
          af[u][i][j] = (ok && av[i]) ? a : (u32x4_t){0u, 0u, 0u, 0u};
        }
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      if constexpr (G128) {
        const u32x4_t ones = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
        bf16x8_t aq[MT][4];
        f32x4_t sa[MT];
#pragma unroll
        for (int i = 0; i < MT; ++i) {
          sa[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const u32x4_t a = af[u][i][j];
            sa[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a),
                                                            __builtin_bit_cast(bf16x8_t, ones), sa[i], 0, 0, 0);
            aq[i][j] = __builtin_bit_cast(
                bf16x8_t, (u32x4_t){(a[0] & 0xffffu) | (a[2] << 16), (a[0] >> 16) | (a[2] & 0xffff0000u),
                                    (a[1] & 0xffffu) | (a[3] << 16), (a[1] >> 16) | (a[3] & 0xffff0000u)});
          }
        }
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
          const float sc = h2f_lo(pf[u][t]), off = h2f_hi(pf[u][t]) - 128.f * sc;
          f32x4_t d[MT];
#pragma unroll
          for (int i = 0; i < MT; ++i) d[i] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const uint32_t w = wf[u][t][j];
            const bf16x8_t e = __builtin_bit_cast(
                bf16x8_t, (u32x4_t){(w & 0x000f000fu) | 0x43004300u, ((w >> 4) & 0x000f000fu) | 0x43004300u,
                                    ((w >> 8) & 0x000f000fu) | 0x43004300u, ((w >> 12) & 0x000f000fu) | 0x43004300u});
#pragma unroll
            for (int i = 0; i < MT; ++i) d[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(aq[i][j], e, d[i], 0, 0, 0);
          }
#pragma unroll
          for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[i][t][r] += fmaf(sc, d[i][r], off * sa[i][r]);
        }
      } else {
#pragma unroll
        for (int t = 0; t < TPW; ++t) {
          const float sc = h2f_lo(pf[u][t]), mn = h2f_hi(pf[u][t]);
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const bf16x8_t f = __builtin_bit_cast(bf16x8_t, w4x8_to_bf16(wf[u][t][j], sc, mn));
#pragma unroll
            for (int i = 0; i < MT; ++i)
              acc[i][t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[u][i][j]), f,
                                                                  acc[i][t], 0, 0, 0);
          }
        }
      }
    }
  }
  // ---- wave partials -> LDS (C fragment: row 16 i + 4 g + r, column 16 t + col)
#pragma unroll
  for (int i = 0; i < MT; ++i)
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wid][i * 16 + 4 * g + r][t * 16 + col] = acc[i][t][r];
  if (ep.norm) skinny_rstd<NWV>(A, lda, M, K, ep, rstd_s);
  __syncthreads();
  if (!splitk_wide<ROWS, COLS>(red, last_s, ws, cnt, M, N, n0)) return;
  stripe_store<TPW>(red, ws != nullptr ? 1 : 0, rstd_s, NoColScale{}, n0, M, N, C, ldc, ep);
}

// ============================================================================ prefill
// gemm_wtile_kernel with a 4-bit W tile: per 64-wide k tile a thread loads its W chunks as one
// dword of 8 codes plus the chunk's parameter dword, and widens them to 8 bf16 into the
// swizzled LDS image.  K % 64 == 32 (G = 32 shards): the last tile's upper chunks are zeros.
struct W4Tile {
  typedef uint32_t param_t;
  struct chunk_t {
    uint32_t w, p;
  };
  struct src_t {
    const uint8_t* w;
    const uint32_t* p;
    int cc8;   // the chunk's first k inside a tile
  };
  static constexpr bool KTAIL = true, COLSCALE = false;
  const uint8_t* W;
  int64_t ldw;
  const uint32_t* P;
  int64_t ldp;
  int gshift;
  __device__ __forceinline__ W4Tile(const uint8_t* W_, int64_t ldw_, const uint32_t* P_, int64_t ldp_, int gshift_)
      : W(W_), ldw(ldw_), P(P_), ldp(ldp_), gshift(gshift_) {}
  __device__ __forceinline__ src_t src(const int64_t n, const int c) const {
    return src_t{W + n * ldw + c * 4, P + n * ldp, c * 8};
  }
  __device__ __forceinline__ chunk_t load(const src_t& s, const int koff) const {
    return chunk_t{*(const uint32_t*)(s.w + (koff >> 1)), s.p[(koff + s.cc8) >> gshift]};
  }
  static __device__ __forceinline__ u32x4_t widen(const chunk_t c) { return w4x8_to_bf16(c.w, h2f_lo(c.p), h2f_hi(c.p)); }
};

// Decode plan for 4-bit weights, 4 < M <= 32 (M <= 4 runs the unsplit row-streaming GEMV):
// column stripes of 64 / 32 / 16 (N divisibility; at most 32 for two row tiles), K split so that
// stripes x splits reach ~512 workgroups (2 per CU), every split >= 4 k blocks of 128 (one per
// wave), chunks whole 128-wide blocks.
DecPlan w4_dec_plan(int M, int N, int K) {
  if (M <= 4 || M > 32) return DecPlan{1, 1, K};
  return dec_plan_stripes(N, K, N % 64 == 0 && M <= 16 ? 4 : (N % 32 == 0 ? 2 : 1), 128, 512);
}

hipError_t gemm_w4(const uint16_t* A, int64_t lda, const uint8_t* W4, int64_t ldw, const uint32_t* params, int G,
                   void* C, int64_t ldc, int M, int N, int K, const GemmEpi& ep, float* ws, uint32_t* cnt, int ksplit,
                   hipStream_t stream) {
  if ((G != 32 && G != 128) || K <= 0 || K % G != 0 || M <= 0 || N <= 0) return hipErrorInvalidValue;
  const int gshift = G == 32 ? 5 : 7;
  const int64_t ldp = K / G;
  if (M <= 4) {   // row-streaming GEMV, non-temporal weight loads
    const dim3 grid((N + 15) / 16);
#define ROWS_LAUNCH(MR_, U_)                                                                                     \
  hipLaunchKernelGGL((gemv_w4_rows_kernel<MR_, U_>), grid, dim3(256), 0, stream, A, lda, W4, ldw, params, ldp, \
                     gshift, C, ldc, M, N, K, ep)
    if (M == 1) ROWS_LAUNCH(1, 2);
    else if (M == 2) ROWS_LAUNCH(2, 1);
    else ROWS_LAUNCH(4, 1);
#undef ROWS_LAUNCH
    return hipGetLastError();
  }
  if (M <= 32) {
    const DecPlan pl = w4_dec_plan(M, N, K);
    if (pl.ks > 1 && pl.ks != ksplit) return hipErrorInvalidValue;   // host sized ws / counters for its plan
    const int gy = pl.ks;
    if (gy > 1 && (ws == nullptr || cnt == nullptr)) return hipErrorInvalidValue;
    float* w = gy > 1 ? ws : nullptr;
    const dim3 grid((N + 16 * pl.tpw - 1) / (16 * pl.tpw), gy);
#define SKINNY_LAUNCH(MT_, T_, G_)                                                                              \
  hipLaunchKernelGGL((gemm_skinny_w4_kernel<MT_, T_, G_>), grid, dim3(256), 0, stream, A, lda, W4, ldw, params, ldp, \
                     gshift, C, ldc, w, cnt, M, N, K, pl.kchunk, ep)
#define SKINNY_G(MT_, T_)                 \
  do {                                    \
    if (G == 128) SKINNY_LAUNCH(MT_, T_, true); \
    else SKINNY_LAUNCH(MT_, T_, false);   \
  } while (0)
    if (M <= 16) {
      if (pl.tpw == 4) SKINNY_G(1, 4);
      else if (pl.tpw == 2) SKINNY_G(1, 2);
      else SKINNY_G(1, 1);
    } else {
      if (pl.tpw == 2) SKINNY_G(2, 2);
      else SKINNY_G(2, 1);
    }
#undef SKINNY_G
#undef SKINNY_LAUNCH
    return hipGetLastError();
  }
  const int64_t t128 = (int64_t)((M + 127) / 128) * ((N + 127) / 128);
  if (t128 >= 256)
    return launch_wtile<128, 128, 2, 2, W4Tile>(A, lda, W4, ldw, params, ldp, gshift, C, ldc, M, N, K, ep, stream);
  return launch_wtile<64, 64, 2, 2, W4Tile>(A, lda, W4, ldw, params, ldp, gshift, C, ldc, M, N, K, ep, stream);
}

}  // namespace lumen
