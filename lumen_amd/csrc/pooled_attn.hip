// Pooled-query attention over the residual stream (gfx950): the attention of a pre-LN block whose
// output is only needed at ONE query row per sequence (CLIP: the CLS row of the last vision block,
// the EOT row of the last text block).  K and V are never formed: with the query pushed through the
// LayerNorm-folded K weights (g) the scores are dot products with the raw residual rows x_j, and the
// softmax-weighted sum of the raw rows (z, c) goes through the folded V weights afterwards as one
// small GEMM.  Per sequence b and head h, over the keys j < kv_len[b]:
//
//   score[h, j] = st[j, 0] * (x_j . g[b, h, :]) + st[j, 1] * s[b, h]
//   p[h, :]     = softmax_j(score[h, :])
//   z[b, h, :]  = sum_j p[h, j] * st[j, 0] * x_j          c[b, h] = sum_j p[h, j] * st[j, 1]
//
// One workgroup = one sequence x 16 heads, one pass over x (flash style, running max).  The heads are
// the MFMA N dimension.  Wave w owns the CW columns [w * CW, (w + 1) * CW) of x: it DMA-loads its own
// [16 tokens, CW] tile of every 16-token chunk into LDS (double-buffered, XOR-swizzled on the source
// address), and uses that one tile twice:
//
//   S^T[tok][head] partial over its columns:  A = x rows (ds_read_b128), B = g fragment (registers)
//   Z^T[col][head] += X^T . P^T            :  A = x^T (ds_read_b64_tr_b16), B = P^T packed from S^T
//
// The partial scores of the waves are summed through LDS in a fixed order, so every wave holds the
// same full scores and runs the same online softmax; the lane layout is that of attention.hip (lane:
// head lane & 15, tokens 4 * (lane >> 4) + r).
#include "common.h"
#include "pooled_attn.h"

namespace lumen {

typedef short s16x4v __attribute__((ext_vector_type(4)));

// tile image: rows of CW bf16; 16-byte chunk XOR so that a 32-lane half of ds_read_b64_tr_b16
// (8 rows x 32 bytes) covers all 64 banks (the ds_read_b128 score reads then conflict two ways)
template <int CW>
__device__ __forceinline__ int px_phys(int row, int chunk) {
  if constexpr (CW == 128) return chunk ^ ((row & 7) << 1);
  else return chunk ^ (((row >> 1) & 3) << 1);
}

__device__ __forceinline__ s16x4v px_read_tr16(const char* p) {
  typedef __attribute__((address_space(3))) s16x4v* lp;
  return __builtin_amdgcn_ds_read_tr16_b64_v4i16((lp)(p));
}

template <int CW>
__global__ void __launch_bounds__(1024) pooled_attn_x_kernel(PooledAttnArgs a) {
  constexpr int KC = 16;                // tokens per chunk
  constexpr int NCH = CW / 8;           // 16-byte chunks per tile row
  constexpr int KS = CW / 32;           // MFMA k-steps of the score product
  constexpr int NB = CW / 16;           // 16-column blocks of z
  constexpr int TILE = KC * CW * 2;     // bytes per wave tile
  constexpr int RPI = 1024 / (CW * 2);  // tile rows per 1 KiB DMA wave-instruction
  constexpr int NI = KC / RPI;          // DMA instructions per tile
  constexpr float LOG2E = 1.4426950408889634f;
  extern __shared__ __attribute__((aligned(16))) char smem[];   // [2][nw][TILE] x tiles, [nw][64] float4 partials

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int nw = blockDim.x >> 6;
  const int col = lane & 15, g = lane >> 4;
  const int b = blockIdx.x;
  const int h = blockIdx.y * 16 + col;
  const bool hok = h < a.H;
  const int wcol0 = wid * CW;
  const int kvl = a.kv_len ? min(max(a.kv_len[b], 0), a.S) : a.S;
  const int nkc = (kvl + KC - 1) / KC;
  const int64_t row0 = (int64_t)b * a.S;
  char* xs = smem;
  f32x4_t* ex = (f32x4_t*)(smem + 2 * nw * TILE);

  // ---- g fragments (B operand of the score product): head h, columns wcol0 + 32 t + 8 g .. + 8
  bf16x8_t gf[KS];
#pragma unroll
  for (int t = 0; t < KS; ++t) {
    u32x4_t v = (u32x4_t){0u, 0u, 0u, 0u};
    if (hok) v = *(const u32x4_t*)(a.g + ((int64_t)b * a.H + h) * a.W + wcol0 + t * 32 + g * 8);
    gf[t] = __builtin_bit_cast(bf16x8_t, v);
  }
  const float sh = hok ? a.s[(int64_t)b * a.H + h] : 0.f;

  typedef __attribute__((address_space(3))) void* lds_ptr_t;
  typedef const __attribute__((address_space(1))) void* g_ptr_t;
  // tokens past the sequence end are clamped to its last row: finite copies, masked below
  auto stage = [&](int chunk, int buf) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int r = i * RPI + lane / NCH;
      const int tok = min(chunk * KC + r, a.S - 1);
      char* dst = xs + (buf * nw + wid) * TILE + i * 1024;
      __builtin_amdgcn_global_load_lds(
          (g_ptr_t)(a.x + (row0 + tok) * a.ldx + wcol0 + px_phys<CW>(r, lane % NCH) * 8), (lds_ptr_t)dst, 16, 0, 0);
    }
  };
  float2 stn[4];                        // (rstd, -mean * rstd) of tokens 4 g + r of the next chunk
  auto load_st = [&](int chunk) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int tok = min(chunk * KC + 4 * g + r, a.S - 1);
      stn[r] = *(const float2*)(a.st + (row0 + tok) * 2);
    }
  };

  f32x4_t acc[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) acc[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f, cs = 0.f;   // running max (all g groups equal), this lane's parts of sum p, sum p st1

  // per-lane byte offsets inside a tile: score rows (token col) and transposed rows (token 4 g + col / 4)
  int kofs[KS], vofs[NB];
#pragma unroll
  for (int t = 0; t < KS; ++t) kofs[t] = col * CW * 2 + (px_phys<CW>(col, t * 4 + g) << 4);
#pragma unroll
  for (int j = 0; j < NB; ++j) {
    const int r0 = 4 * g + (col >> 2), c0 = j * 16 + 4 * (col & 3);
    vofs[j] = r0 * CW * 2 + (px_phys<CW>(r0, c0 >> 3) << 4) + (c0 & 7) * 2;
  }

  if (nkc > 0) {
    stage(0, 0);
    load_st(0);
  }
  for (int kc = 0; kc < nkc; ++kc) {
    const int buf = kc & 1;
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();                    // tile kc landed; every wave has read the partials of chunk kc - 1
    float2 stc[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) stc[r] = stn[r];
    if (kc + 1 < nkc) {
      stage(kc + 1, buf ^ 1);
      load_st(kc + 1);
    }
    const char* tile = xs + (buf * nw + wid) * TILE;

    // partial S^T over this wave's columns
    f32x4_t sc = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      const bf16x8_t xf = *(const bf16x8_t*)(tile + kofs[t]);
      sc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(xf, gf[t], sc, 0, 0, 0);
    }
    ex[wid * 64 + lane] = sc;
    __syncthreads();
    f32x4_t tot = ex[lane];
    for (int w = 1; w < nw; ++w) tot += ex[w * 64 + lane];

    // online softmax: lane = head col, tokens k0 + 4 g + r
    const int k0 = kc * KC;
    float sv[4], mx = -INFINITY;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const bool ok = k0 + 4 * g + r < kvl;
      sv[r] = ok ? __builtin_fmaf(stc[r].x, tot[r], stc[r].y * sh) : -INFINITY;
      mx = fmaxf(mx, sv[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float mn = fmaxf(m, mx);      // finite: token k0 of every chunk is a live key
    const float alpha = __builtin_amdgcn_exp2f((m - mn) * LOG2E);
    m = mn;
    float ps = 0.f, pc = 0.f;
    s16x4v pf;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = __builtin_amdgcn_exp2f((sv[r] - mn) * LOG2E);
      ps += p;
      pc = __builtin_fmaf(p, stc[r].y, pc);
      pf[r] = (short)f2bf(p * stc[r].x);
    }
    l = __builtin_fmaf(l, alpha, ps);
    cs = __builtin_fmaf(cs, alpha, pc);

    // Z^T += X^T P^T: lane = head col, columns 16 j + 4 g + r
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      const s16x4v xt = px_read_tr16(tile + vofs[j]);
      acc[j] = __builtin_amdgcn_mfma_f32_16x16x16bf16_1k(xt, pf, acc[j] * alpha, 0, 0, 0);
    }
  }

  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  cs += __shfl_xor(cs, 16, 64);
  cs += __shfl_xor(cs, 32, 64);
  const float inv = l > 0.f ? 1.f / l : 0.f;
  if (hok) {
    uint16_t* zr = a.z + ((int64_t)b * a.H + h) * a.W + wcol0 + 4 * g;
#pragma unroll
    for (int j = 0; j < NB; ++j) {
      uint2 w;
      w.x = pack2bf(acc[j][0] * inv, acc[j][1] * inv);
      w.y = pack2bf(acc[j][2] * inv, acc[j][3] * inv);
      *(uint2*)(zr + j * 16) = w;
    }
    if (wid == 0 && g == 0) a.c[(int64_t)b * a.H + h] = cs * inv;
  }
}

template <int CW>
static hipError_t launch_pooled(const PooledAttnArgs& a, int B, hipStream_t stream) {
  const int nw = a.W / CW;
  const size_t lds = (size_t)2 * nw * 16 * CW * 2 + (size_t)nw * 1024;
  // set on every launch (cheap): the attribute is per device, and a process may drive several
  if (lds > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute((const void*)pooled_attn_x_kernel<CW>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
  }
  hipLaunchKernelGGL((pooled_attn_x_kernel<CW>), dim3(B, (a.H + 15) / 16), dim3(64 * nw), lds, stream, a);
  return hipGetLastError();
}

// W % 64 == 0; 64-column waves up to W = 512 (and for the odd multiples of 64 up to 1024), 128-column
// waves above: at most 16 waves per workgroup
hipError_t pooled_attn_x(const PooledAttnArgs& a, int B, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  if (a.W % 64 != 0 || a.S < 1 || a.H < 1) return hipErrorInvalidValue;
  if (a.W > 512 && a.W % 128 == 0) {
    if (a.W > 2048) return hipErrorInvalidValue;
    return launch_pooled<128>(a, B, stream);
  }
  if (a.W > 1024) return hipErrorInvalidValue;
  return launch_pooled<64>(a, B, stream);
}

}  // namespace lumen
