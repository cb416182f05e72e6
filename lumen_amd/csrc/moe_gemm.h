// The grouped GEMM of the sparse mixture-of-experts MLP: moe_gemm_kernel<MT, MODE, W>, included by
// moe.hip (bf16 weights: router logits, gate|up, down) and moe_wq.hip (fp8 and 4-bit experts).
//
// A sibling of gemm_skinny_kernel (gemm_wdec.h): a workgroup owns one 16-column stripe of ONE expert,
// both MFMA operands come straight from global memory in fragment layout and its 4 waves split K,
// reduced through LDS.  What it adds is the row indirection (activation rows are gathered through
// `rowmap`) and the expert stride on the weights and on their scales / group parameters.  grid.y
// indexes the list of NON-EMPTY experts the group kernel compacts (at most min(E, T k) of them);
// workgroups past the list's end leave at once.  The expert's rows are walked MT * 16 at a time.
// No floating-point atomics and no cross-workgroup reduction: every output element is summed in one
// fixed order, so results are bit-identical from run to run.
//
// W is the weight policy:
//   MoeBf16      [E, N, K] bf16; 32-wide k blocks, wave wid takes blocks wid, wid + 4, ..., 4 in flight
//   MoeFp8       [E, N, K] e4m3fn + fp32 scale [E, N]; 64-wide k blocks, one 16-byte load feeds two
//                MFMAs (as SkinnyFp8), the scale of column n0 + c multiplies the summed tile after the
//                LDS reduction -- before the SwiGLU pairing, gate and up columns carry different scales
//   MoeW4<G128>  [E, N, K / 2] codes + fp16 (scale, wmin) [E, N, K / G, 2]; 128-wide k blocks, lane
//                group g owns k in [32 g, 32 g + 32) (as gemm_skinny_w4_kernel).  G = 128: the exact
//                codes go into the MFMA as 0x4300 | c with the A pairs permuted identically, the row sum
//                comes from an MFMA against ones and the group parameters scale the block's partial
//                sums; G = 32: codes are widened in registers to bf16(code * scale + wmin).  A lane
//                group whose k range lies past K loads a clamped in-row address and zeroes A.
#pragma once
#include "common.h"
#include "moe.h"
#include "wq_widen.h"

namespace lumen {

enum MoeMode : int { MOE_LOGITS = 0, MOE_GATE_UP = 1, MOE_DOWN = 2 };

struct MoeGemmArgs {
  const uint16_t* A;      // activation rows [*, K] bf16
  int64_t lda;
  const void* W;          // [E, N, K] in the policy's format (MOE_LOGITS: [N, K])
  int64_t w_stride;       // policy elements (bf16 / fp8 code / byte of two 4-bit codes) between experts
  const void* S;          // fp8: fp32 scale [E, N]; 4-bit: (scale, wmin) dwords [E, N, K / G]; bf16: unused
  int gshift;             // 4-bit: log2 G
  void* C;                // MOE_LOGITS f32 [M, N]; MOE_GATE_UP bf16 [P, N / 2]; MOE_DOWN f32 [P, N]
  int64_t ldc;
  const int* rowmap;      // sorted position -> row of A (nullptr: the sorted position itself)
  const int* cnt;
  const int* off;
  const int* active;      // [E + 1]
  int M, N, K, E;
};

struct MoeBf16 {
  typedef uint16_t wt;
  static constexpr int KB = 32;
  static constexpr bool SCALED = false, W4 = false, G128 = false;
  static __device__ __forceinline__ void frags(const u32x4_t w, bf16x8_t (&f)[1]) { f[0] = __builtin_bit_cast(bf16x8_t, w); }
};

struct MoeFp8 {
  typedef uint8_t wt;
  static constexpr int KB = 64;
  static constexpr bool SCALED = true, W4 = false, G128 = false;
  static __device__ __forceinline__ void frags(const u32x4_t w, bf16x8_t (&f)[2]) { fp8x16_to_bf16(w, f[0], f[1]); }
};

template <bool G128_>
struct MoeW4 {
  typedef uint8_t wt;
  static constexpr int KB = 128;
  static constexpr bool SCALED = false, W4 = true, G128 = G128_;
};

template <int MT, int MODE, class W>
__global__ void __launch_bounds__(256) moe_gemm_kernel(const MoeGemmArgs a) {
  constexpr int NWV = 4, KB = W::KB, ROWS = MT * 16;
  __shared__ float red[NWV][ROWS][17];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int N = a.N, K = a.K;
  int e = 0, base = 0, row_begin = 0, row_end;
  if constexpr (MODE == MOE_LOGITS) {
    row_begin = blockIdx.y * ROWS;
    row_end = min(a.M, row_begin + ROWS);
  } else {
    if ((int)blockIdx.y >= a.active[a.E]) return;   // past the non-empty experts (workgroup-uniform)
    e = a.active[blockIdx.y];
    base = a.off[e];
    row_end = a.cnt[e];
  }
  const int64_t nrow = min(n0 + col, N - 1);
  // lane (col, g): its k offset inside a block, identically for A row col and W row n0 + col
  // (4-bit: added per block, where the lane group's range is clamped into K)
  constexpr int KG = W::W4 ? 0 : KB / 4;

  for (int rb = row_begin; rb < row_end; rb += ROWS) {
    const uint16_t* ar[MT];
    bool av[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) {
      const int m = rb + t * 16 + col;
      av[t] = m < row_end;
      int64_t row = 0;
      if (av[t]) row = a.rowmap != nullptr ? a.rowmap[base + m] : base + m;
      ar[t] = a.A + row * a.lda + g * KG;
    }
    f32x4_t acc[MT];
#pragma unroll
    for (int t = 0; t < MT; ++t) acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

    if constexpr (!W::W4) {
      constexpr int UNR = 4, NF = KB / 32;
      const typename W::wt* wr = (const typename W::wt*)a.W + (int64_t)e * a.w_stride + nrow * K + g * KG;
      const int nblk = K / KB;
      auto load_a = [&](const int kk, u32x4_t (&af)[MT][NF]) {
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
          for (int j = 0; j < NF; ++j) {
            af[t][j] = *(const u32x4_t*)(ar[t] + kk + 8 * j);
            if (!av[t]) af[t][j] = (u32x4_t){0u, 0u, 0u, 0u};
          }
      };
      auto mma_block = [&](const u32x4_t w, const u32x4_t (&af)[MT][NF]) {
        bf16x8_t f[NF];
        W::frags(w, f);
#pragma unroll
        for (int t = 0; t < MT; ++t)
#pragma unroll
          for (int j = 0; j < NF; ++j)
            acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[t][j]), f[j], acc[t], 0, 0, 0);
      };
      // wave wid takes k blocks wid, wid + 4, ... (UNR at a time)
      int s = wid;
      for (; s + NWV * (UNR - 1) < nblk; s += NWV * UNR) {
        u32x4_t wf[UNR];
        u32x4_t af[UNR][MT][NF];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          const int kk = (s + NWV * u) * KB;
          wf[u] = *(const u32x4_t*)(wr + kk);
          load_a(kk, af[u]);
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) mma_block(wf[u], af[u]);
      }
      if constexpr (W::SCALED) {
        // fp8: the 1 .. UNR - 1 blocks left go out together (the down projection's K = 768 is 12 blocks,
        // 3 per wave and no unrolled pass at all); a slot past the end loads block 0 and zeroes A
        if (s < nblk) {
          u32x4_t wf[UNR - 1];
          u32x4_t af[UNR - 1][MT][NF];
#pragma unroll
          for (int u = 0; u < UNR - 1; ++u) {
            const bool ok = s + NWV * u < nblk;
            const int kk = ok ? (s + NWV * u) * KB : 0;
            wf[u] = *(const u32x4_t*)(wr + kk);
            load_a(kk, af[u]);
            if (!ok) {
#pragma unroll
              for (int t = 0; t < MT; ++t)
#pragma unroll
                for (int j = 0; j < NF; ++j) af[u][t][j] = (u32x4_t){0u, 0u, 0u, 0u};
            }
          }
#pragma unroll
          for (int u = 0; u < UNR - 1; ++u) mma_block(wf[u], af[u]);
        }
        s = nblk;
      }
      for (; s < nblk; s += NWV) {
        const int kk = s * KB;
        const u32x4_t wf = *(const u32x4_t*)(wr + kk);
        u32x4_t af[MT][NF];
        load_a(kk, af);
        mma_block(wf, af);
      }
    } else {
      // 16 rows: 2 blocks in flight per wave; 64 rows: 1 (the A fragments of a block are 16 VGPRs per row tile)
      constexpr int UNR = MT == 1 ? 2 : 1;
      const uint8_t* wr = (const uint8_t*)a.W + (int64_t)e * a.w_stride + nrow * (K >> 1);
      const uint32_t* pr = (const uint32_t*)a.S + ((int64_t)e * N + nrow) * (K >> a.gshift);
      const int nblk = (K + 127) >> 7;
      for (int s = wid; s < nblk; s += NWV * UNR) {
        u32x4_t wf[UNR];
        uint32_t pf[UNR];
        u32x4_t af[UNR][MT][4];
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          const int k = (s + NWV * u) * 128 + 32 * g;
          const bool ok = k < K;
          const int kc = ok ? k : 0;
          wf[u] = *(const u32x4_t*)(wr + (kc >> 1));
          pf[u] = pr[kc >> a.gshift];
#pragma unroll
          for (int t = 0; t < MT; ++t)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const u32x4_t x = *(const u32x4_t*)(ar[t] + kc + 8 * j);
              af[u][t][j] = (ok && av[t]) ? x : (u32x4_t){0u, 0u, 0u, 0u};
            }
        }
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          if constexpr (W::G128) {
            // acc += scale * (A . (128 + c)) + (wmin - 128 scale) * rowsum(A): lane-local, a lane's
            // accumulator column is its own W row
            const u32x4_t ones = {0x3f803f80u, 0x3f803f80u, 0x3f803f80u, 0x3f803f80u};
            const float sc = h2f_lo(pf[u]), off = h2f_hi(pf[u]) - 128.f * sc;
#pragma unroll
            for (int t = 0; t < MT; ++t) {
              f32x4_t sa = (f32x4_t){0.f, 0.f, 0.f, 0.f}, d = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
              for (int j = 0; j < 4; ++j) {
                sa = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[u][t][j]),
                                                             __builtin_bit_cast(bf16x8_t, ones), sa, 0, 0, 0);
                d = __builtin_amdgcn_mfma_f32_16x16x32_bf16(pair_i_i4(af[u][t][j]), w4x8_exact(wf[u][j]), d, 0, 0, 0);
              }
#pragma unroll
              for (int r = 0; r < 4; ++r) acc[t][r] += fmaf(sc, d[r], off * sa[r]);
            }
          } else {
            const float sc = h2f_lo(pf[u]), mn = h2f_hi(pf[u]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const bf16x8_t f = __builtin_bit_cast(bf16x8_t, w4x8_to_bf16(wf[u][j], sc, mn));
#pragma unroll
              for (int t = 0; t < MT; ++t)
                acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, af[u][t][j]), f, acc[t], 0, 0, 0);
            }
          }
        }
      }
    }
    // C fragment: row t * 16 + 4 g + r, column n0 + col
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wid][t * 16 + 4 * g + r][col] = acc[t][r];
    __syncthreads();
    const int m = rb + tid;
    if (tid < ROWS && m < row_end) {
      float v[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) v[c] = ((red[0][tid][c] + red[1][tid][c]) + red[2][tid][c]) + red[3][tid][c];
      if constexpr (W::SCALED) {   // N % 16 == 0 in the expert modes
        const float* sc = (const float*)a.S + (int64_t)e * N + n0;
#pragma unroll
        for (int c = 0; c < 16; ++c) v[c] *= sc[c];
      }
      if constexpr (MODE == MOE_LOGITS) {
        float* o = (float*)a.C + (int64_t)m * a.ldc + n0;
#pragma unroll
        for (int c = 0; c < 16; ++c)
          if (n0 + c < N) o[c] = v[c];
      } else if constexpr (MODE == MOE_GATE_UP) {   // [gate 8 | up 8] -> 8 columns of silu(gate) * up
        float o[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) o[q] = v[q] * fast_rcp(1.f + __expf(-v[q])) * v[8 + q];
        *(u32x4_t*)((uint16_t*)a.C + (int64_t)(base + m) * a.ldc + (n0 >> 1)) = pack8(o);
      } else {
        f32x4_t* o = (f32x4_t*)((float*)a.C + (int64_t)(base + m) * a.ldc + n0);
#pragma unroll
        for (int q = 0; q < 4; ++q) o[q] = (f32x4_t){v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
      }
    }
    __syncthreads();   // red is rewritten by the next row block
  }
}

// The two grouped GEMMs of the expert MLP (after moe_group); WG / WD are the policies of gate|up and
// down (they differ only for 4-bit experts whose H and I give different group sizes).
template <class WG, class WD = WG>
inline hipError_t moe_launch_experts(const uint16_t* x, int64_t ldx, const void* gu_w, const void* gu_s,
                                     const void* down_w, const void* down_s, int64_t gu_stride, int64_t down_stride,
                                     int gshift_gu, int gshift_down, int T, int E, int k, int H, int I,
                                     const MoeWork& work, hipStream_t stream) {
  const int P = T * k;
  const int ny = E < P ? E : P;   // at most this many experts hold a row
  MoeGemmArgs a{};
  a.cnt = work.cnt; a.off = work.off; a.active = work.active;
  a.M = P; a.E = E;
  const dim3 block(256);
  const bool tall = P > MOE_DECODE_PAIRS;
  // gate | up: rows gathered from x through the sorted order
  a.A = x; a.lda = ldx; a.rowmap = work.src_tok;
  a.W = gu_w; a.w_stride = gu_stride; a.S = gu_s; a.gshift = gshift_gu;
  a.C = work.g; a.ldc = I;
  a.N = 2 * I; a.K = H;
  if (tall) hipLaunchKernelGGL((moe_gemm_kernel<4, MOE_GATE_UP, WG>), dim3(2 * I / 16, ny), block, 0, stream, a);
  else hipLaunchKernelGGL((moe_gemm_kernel<1, MOE_GATE_UP, WG>), dim3(2 * I / 16, ny), block, 0, stream, a);
  // down: rows of g are already in sorted order
  a.A = work.g; a.lda = I; a.rowmap = nullptr;
  a.W = down_w; a.w_stride = down_stride; a.S = down_s; a.gshift = gshift_down;
  a.C = work.y; a.ldc = H;
  a.N = H; a.K = I;
  if (tall) hipLaunchKernelGGL((moe_gemm_kernel<4, MOE_DOWN, WD>), dim3(H / 16, ny), block, 0, stream, a);
  else hipLaunchKernelGGL((moe_gemm_kernel<1, MOE_DOWN, WD>), dim3(H / 16, ny), block, 0, stream, a);
  return hipGetLastError();
}

// One grouped GEMM without an epilogue: work.y [P, N] fp32 (sorted order) = rows of x gathered through
// work.src_tok times expert weights [E, N, K] -- the MOE_DOWN mode with a row map (after moe_group).
template <class W>
inline hipError_t moe_launch_grouped(const uint16_t* x, int64_t ldx, const void* w, const void* s, int64_t w_stride,
                                     int gshift, int T, int E, int k, int N, int K, const MoeWork& work,
                                     hipStream_t stream) {
  const int P = T * k;
  const int ny = E < P ? E : P;
  MoeGemmArgs a{};
  a.cnt = work.cnt; a.off = work.off; a.active = work.active;
  a.M = P; a.E = E;
  a.A = x; a.lda = ldx; a.rowmap = work.src_tok;
  a.W = w; a.w_stride = w_stride; a.S = s; a.gshift = gshift;
  a.C = work.y; a.ldc = N;
  a.N = N; a.K = K;
  if (P > MOE_DECODE_PAIRS) hipLaunchKernelGGL((moe_gemm_kernel<4, MOE_DOWN, W>), dim3(N / 16, ny), dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((moe_gemm_kernel<1, MOE_DOWN, W>), dim3(N / 16, ny), dim3(256), 0, stream, a);
  return hipGetLastError();
}

}  // namespace lumen
