// Prefill tile of the weight-only GEMMs (M > 32): C[M, N] = epi(A[M, K] . dq(Wq)[N, K]^T), A bf16.
// Register-staged 2-stage BM x BN x 64 tile: while the MFMAs run on one swizzled LDS image, the
// next k tile's A chunks and quantised W chunks wait in registers; a W chunk (8 weights) is
// widened to 8 bf16 on its way into the LDS image, after which the MFMA loop is the bf16 one.
// The epilogue goes through LDS in 16-row slabs to the shared epi_store16.
//
// W is the weight policy, constructed in the kernel from (Wq, ldw, P, ldp, gshift):
//   param_t            element type of the parameter tensor P (fp8: fp32 column scales; 4-bit:
//                      one (scale, wmin) dword per group)
//   chunk_t            registers of a staged chunk of 8 weights (4-bit: codes + parameter dword)
//   src_t, src(n, c)   a thread's source pointers for chunk column c of W row n
//   load(src, koff)    stage the chunk at element offset koff from src
//   widen(chunk)       -> u32x4_t, 8 bf16
//   KTAIL              K % 64 != 0 is allowed: chunks past K are zeros (loaded from a clamped
//                      in-row address).  false: the k loop carries no tail predicate
//   COLSCALE, colscale(n)   per-column fp32 multiplier of the accumulator
#pragma once
#include "common.h"
#include "gemm_epi.h"

namespace lumen {

template <int BM, int BN, int WM, int WN, class W>
__global__ void __launch_bounds__(WM* WN * 64)
gemm_wtile_kernel(const uint16_t* __restrict__ A, int64_t lda, const uint8_t* __restrict__ Wq, int64_t ldw,
                  const typename W::param_t* __restrict__ P, int64_t ldp, int gshift, void* __restrict__ C, int64_t ldc,
                  int M, int N, int K, GemmEpi ep) {
  constexpr int NT = WM * WN * 64;
  constexpr int TM = BM / WM, TN = BN / WN;
  constexpr int MR = TM / 16, NR = TN / 16;
  constexpr int CA = BM * 8 / NT;  // 8-element chunks per thread
  constexpr int CB = BN * 8 / NT;
  static_assert(CA >= 1 && CB >= 1 && BM * 8 % NT == 0 && BN * 8 % NT == 0, "bad tiling");

  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* sA = smem;                 // [2][BM][128 B] bf16
  char* sB = smem + 2 * BM * 128;  // [2][BN][128 B] bf16 (widened)
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int wm = wid / WN, wn = wid % WN;
  const int tiles_n = (N + BN - 1) / BN, tiles_m = (M + BM - 1) / BM;
  const int bid = xcd_remap(blockIdx.x, tiles_n * tiles_m);
  const int m0 = (bid / tiles_n) * BM, n0 = (bid % tiles_n) * BN;

  const W w(Wq, ldw, P, ldp, gshift);
  const uint16_t* pa[CA];
  typename W::src_t pb[CB];
  int la[CA], lb[CB];
  // chunk column (the same for every chunk of a thread: NT % 8 == 0)
  const int cc8 = (tid & 7) * 8;
#pragma unroll
  for (int i = 0; i < CA; ++i) {
    const int id = tid + i * NT, r = id >> 3, c = id & 7;
    pa[i] = A + (int64_t)min(m0 + r, M - 1) * lda + c * 8;
    la[i] = swz(r, c);
  }
#pragma unroll
  for (int i = 0; i < CB; ++i) {
    const int id = tid + i * NT, r = id >> 3, c = id & 7;
    pb[i] = w.src(min(n0 + r, N - 1), c);
    lb[i] = swz(r, c);
  }
  f32x4_t acc[MR][NR];
#pragma unroll
  for (int i = 0; i < MR; ++i)
#pragma unroll
    for (int j = 0; j < NR; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  u32x4_t ra[CA];
  typename W::chunk_t rb[CB];
  const int nk = W::KTAIL ? (K + 63) / 64 : K / 64;
  auto load_tile = [&](const int kt) {
    int koff = kt * 64;   // relative to the chunk pointers
    bool ok = true;
    if constexpr (W::KTAIL) {
      ok = koff + cc8 < K;
      koff = ok ? koff : -cc8;   // clamped (in-row) address, values zeroed
    }
#pragma unroll
    for (int i = 0; i < CA; ++i) {
      const u32x4_t a = *(const u32x4_t*)(pa[i] + koff);
      ra[i] = ok ? a : (u32x4_t){0u, 0u, 0u, 0u};
    }
#pragma unroll
    for (int i = 0; i < CB; ++i) rb[i] = w.load(pb[i], koff);
  };
  auto store_tile = [&](char* dA, char* dB) {
#pragma unroll
    for (int i = 0; i < CA; ++i) *(u32x4_t*)(dA + la[i]) = ra[i];
#pragma unroll
    for (int i = 0; i < CB; ++i) *(u32x4_t*)(dB + lb[i]) = W::widen(rb[i]);
  };
  load_tile(0);
  store_tile(sA, sB);
  __syncthreads();
  const int frow = lane & 15, fq = lane >> 4;
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load_tile(kt + 1);
    const char* tA = sA + cur * BM * 128;
    const char* tB = sB + cur * BN * 128;
#pragma unroll
    for (int s = 0; s < 2; ++s) {
      bf16x8_t fa[MR], fb[NR];
#pragma unroll
      for (int i = 0; i < MR; ++i) fa[i] = *(const bf16x8_t*)(tA + swz(wm * TM + i * 16 + frow, s * 4 + fq));
#pragma unroll
      for (int j = 0; j < NR; ++j) fb[j] = *(const bf16x8_t*)(tB + swz(wn * TN + j * 16 + frow, s * 4 + fq));
#pragma unroll
      for (int i = 0; i < MR; ++i)
#pragma unroll
        for (int j = 0; j < NR; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    if (kt + 1 < nk) store_tile(sA + (cur ^ 1) * BM * 128, sB + (cur ^ 1) * BN * 128);
    __syncthreads();
  }
  // epilogue through LDS, 16-row slabs; a column scale is applied in fp32
  constexpr int LDSTR = TN + 4;
  float* es = (float*)smem + wid * 16 * LDSTR;
  constexpr int LPR = TN / 16;
  constexpr int RPP = 64 / LPR;
  constexpr int NPASS = RPP >= 16 ? 1 : 16 / RPP;
  Unroll<0, MR>::run([&](const int i) {
#pragma unroll
    for (int j = 0; j < NR; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) es[(fq * 4 + r) * LDSTR + j * 16 + frow] = acc[i][j][r];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
      const int rr = p * RPP + lane / LPR;
      const int cc = (lane % LPR) * 16;
      if (rr < 16) {
        const int n = n0 + wn * TN + cc;
        float v[16];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x4_t t = *(const f32x4_t*)(es + rr * LDSTR + cc + q * 4);
          v[q * 4 + 0] = t[0]; v[q * 4 + 1] = t[1]; v[q * 4 + 2] = t[2]; v[q * 4 + 3] = t[3];
        }
        if constexpr (W::COLSCALE) {
#pragma unroll
          for (int q = 0; q < 16; ++q) v[q] *= n + q < N ? w.colscale(n + q) : 0.f;
        }
        epi_store16(v, m0 + wm * TM + i * 16 + rr, n, M, N, C, ldc, ep);
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  });
}

template <int BM, int BN, int WM, int WN, class W>
static hipError_t launch_wtile(const uint16_t* A, int64_t lda, const uint8_t* Wq, int64_t ldw,
                               const typename W::param_t* P, int64_t ldp, int gshift, void* C, int64_t ldc, int M, int N,
                               int K, const GemmEpi& ep, hipStream_t stream) {
  const int tiles = ((M + BM - 1) / BM) * ((N + BN - 1) / BN);
  size_t lds = 2 * (size_t)(BM + BN) * 128;
  const size_t epi = (size_t)WM * WN * 16 * (BN / WN + 4) * 4;
  if (epi > lds) lds = epi;
  auto kern = gemm_wtile_kernel<BM, BN, WM, WN, W>;
  static bool attr_set = false;
  if (!attr_set) {
    (void)hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    attr_set = true;
  }
  hipLaunchKernelGGL(kern, dim3(tiles), dim3(WM * WN * 64), lds, stream, A, lda, Wq, ldw, P, ldp, gshift, C, ldc, M, N,
                     K, ep);
  return hipGetLastError();
}

}  // namespace lumen
