// Decode scaffold of the weight-only GEMMs (bf16 gemm_skinny.hip, fp8 gemm_w8.hip, 4-bit
// gemm_w4.hip): everything around a kernel's weight stream that does not depend on the weight
// format -- the launch plan, the two-slot register pipeline, the row-GEMV prologue and tail, the
// in-launch split-K hand-offs and the 16-column split-K MFMA kernel.  A format keeps only how a
// weight chunk is loaded, widened and scaled.
#pragma once
#include <type_traits>

#include "common.h"
#include "gemm_epi.h"

namespace lumen {

typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));

// ============================================================================ launch plan (host)
// Launch plan of a weight-only decode GEMM, 4 < M <= 32: 16-column tiles per wave, K splits and
// the K chunk per split.  The host sizes the split-K slabs / counters from the same plan.
struct DecPlan {
  int tpw;
  int ks;
  int kchunk;
};
DecPlan w8_dec_plan(int M, int N, int K);
DecPlan w4_dec_plan(int M, int N, int K);

// Column stripes of 16 * tpw, K split so that stripes x splits reach ~512 workgroups (2 per CU),
// every split >= kmin of K (4 k blocks, one per wave), chunks whole kblk-wide blocks.
inline DecPlan dec_plan_stripes(int N, int K, int tpw, int kblk, int kmin) {
  DecPlan p{tpw, 1, K};
  const int stripes = (N + 16 * tpw - 1) / (16 * tpw);
  int ks = (512 + stripes - 1) / stripes;
  const int kmax = K / kmin > 1 ? K / kmin : 1;
  ks = ks < kmax ? ks : kmax;
  int kchunk = (K + ks - 1) / ks;
  kchunk = (kchunk + kblk - 1) / kblk * kblk;
  p.ks = (K + kchunk - 1) / kchunk;
  if (p.ks > 1) p.kchunk = kchunk;
  return p;
}

// ============================================================================ device pieces
// t + <8 bf16 of x, 8 bf16 of y> on v_dot2c_f32_bf16.  The pairs are taken by shuffling a
// bf16x8 view: bit-casting a u32 vector ELEMENT to bf16x2 miscompiles on ROCm 7.2 (every
// element reads lane 0's dword).
__device__ __forceinline__ float dot8_bf16(const u32x4_t x, const u32x4_t y, float t) {
  const bf16x8_t xv = __builtin_bit_cast(bf16x8_t, x), yv = __builtin_bit_cast(bf16x8_t, y);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const bf16x2_t p = {xv[2 * j], xv[2 * j + 1]}, q = {yv[2 * j], yv[2 * j + 1]};
    t = __builtin_amdgcn_fdot2_f32_bf16(p, q, t, false);
  }
  return t;
}

// Two-slot register pipeline over nch chunks of U steps: issue(slot, first step) loads a chunk
// into a register slot, consume(slot, U) uses it; chunk c + 1 is issued before chunk c is
// consumed.  Straight-line steady state (a conditional issue inside the loop makes the waitcnt
// pass merge both paths and drain everything), and a sched_barrier after every issue: the machine
// scheduler otherwise sinks part of chunk c's loads below chunk c + 1's.  The lambdas come by
// value (closures of references): taken by reference, the 4-bit <2, 1> row kernel allocates 5
// more VGPRs.
template <int U, class Issue, class Consume>
__device__ __forceinline__ void pipeline2(const int nch, const Issue issue, const Consume consume) {
  if (nch > 0) {
    issue(0, 0);
    __builtin_amdgcn_sched_barrier(0);
    int c = 0;
    for (; c + 2 < nch; c += 2) {
      issue(1, (c + 1) * U);
      __builtin_amdgcn_sched_barrier(0);
      consume(0, U);
      __builtin_amdgcn_sched_barrier(0);
      issue(0, (c + 2) * U);
      __builtin_amdgcn_sched_barrier(0);
      consume(1, U);
      __builtin_amdgcn_sched_barrier(0);
    }
    if (c + 1 < nch) {
      issue(1, (c + 1) * U);
      __builtin_amdgcn_sched_barrier(0);
      consume(0, U);
      __builtin_amdgcn_sched_barrier(0);
      consume(1, U);
    } else {
      consume(0, U);
    }
  }
}

// No per-column multiplier (4-bit: the group scales are applied in the weight stream).
struct NoColScale {};

// ---------------------------------------------------------------------------- row GEMV (M <= 4)
// A workgroup = 4 waves x 4 rows = 16 consecutive output columns, so the decode epilogue works on
// whole 16-column tiles (SwiGLU [gate 8 | up 8] pairing, ssq tiles).  Everything the epilogue
// reads -- the folded-norm sums of squares, bias and residual -- is loaded BEFORE the weight
// stream, so the tail after the last weight byte is only the reductions and the store (vmcnt
// retires in issue order: a load issued after the stream would wait behind it).  Straight-line
// loads at clamped addresses, so no exec-masked branch makes the compiler drain vmcnt before the
// weight stream is issued.
template <int MR>
struct RowPre {
  static constexpr int SSQ4 = 4;   // float4 ssq loads per lane and row: K <= 4 * 4 * 64 * 16 = 16384
  static constexpr int NM = MR <= 2 ? MR : 1;
  bool rs_pre, full16, pre_bias, pre_res;
  f32x4_t ssq_v[NM][SSQ4];
  u32x4_t pre_b[2], pre_r[2];

  __device__ __forceinline__ void load(const GemmEpi& ep, const int M, const int N, const int K, const int n0,
                                       const int lane) {
    const bool rs = MR <= 2 && ep.norm && ep.ssq_in != nullptr && K <= SSQ4 * 4 * 64 * 16;
    f32x4_t sv[NM][SSQ4];
    if (rs) {   // wave-uniform
      const int n4 = ep.ssq_tiles >> 2;
#pragma unroll
      for (int m = 0; m < NM; ++m) {
        const f32x4_t* p = (const f32x4_t*)(ep.ssq_in + (int64_t)min(m, M - 1) * ep.ssq_tiles);
#pragma unroll
        for (int j = 0; j < SSQ4; ++j) sv[m][j] = p[min(lane + j * 64, n4 - 1)];
      }
    }
    const int prow = min(lane, M - 1);
    const bool f16 = n0 + 16 <= N;
    const bool pb = ep.bias && !ep.bias_f32 && f16;
    const bool pr = ep.residual && f16;
    u32x4_t b[2] = {(u32x4_t){0u, 0u, 0u, 0u}, (u32x4_t){0u, 0u, 0u, 0u}};
    u32x4_t r[2] = {(u32x4_t){0u, 0u, 0u, 0u}, (u32x4_t){0u, 0u, 0u, 0u}};
    if (pb) {
      b[0] = *(const u32x4_t*)((const uint16_t*)ep.bias + n0);
      b[1] = *(const u32x4_t*)((const uint16_t*)ep.bias + n0 + 8);
    }
    if (pr) {
      r[0] = *(const u32x4_t*)(ep.residual + (int64_t)prow * ep.ldr + n0);
      r[1] = *(const u32x4_t*)(ep.residual + (int64_t)prow * ep.ldr + n0 + 8);
    }
    // members are filled from locals: loaded in place, the 4-bit <1, 2> row kernel allocates 83 more VGPRs
    rs_pre = rs, full16 = f16, pre_bias = pb, pre_res = pr;
#pragma unroll
    for (int m = 0; m < NM; ++m)
#pragma unroll
      for (int j = 0; j < SSQ4; ++j) ssq_v[m][j] = sv[m][j];
    pre_b[0] = b[0], pre_b[1] = b[1], pre_r[0] = r[0], pre_r[1] = r[1];
  }
};

// Tail of a row GEMV: every (row, m) partial is reduced over the 64 lanes, rstd comes from the
// preloaded sums of squares (or skinny_rstd), then thread m < M finishes row m of the 16-column
// tile: the fast bf16 bias / SwiGLU / residual / ssq_out store from the prologue registers, or
// the generic epilogue.  sc: per-column multipliers in LDS (16 floats, written by the caller
// before this call) or NoColScale.
template <int MR, class SC>
__device__ __forceinline__ void row_gemv_tail(const float (&acc)[4][MR], const RowPre<MR>& pre, float (&red)[16][MR],
                                              float (&rstd_s)[MR], const SC sc, const uint16_t* __restrict__ A,
                                              const int64_t lda, void* __restrict__ C, const int64_t ldc, const int M,
                                              const int N, const int K, const int n0, const GemmEpi& ep) {
  constexpr int R = 4;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
#pragma unroll
  for (int r = 0; r < R; ++r)
#pragma unroll
    for (int m = 0; m < MR; ++m) {
      const float v = wave_sum(acc[r][m]);
      if (lane == 0) red[wid * R + r][m] = v;
    }
  if (ep.norm) {
    if (pre.rs_pre) {
      if (wid == 0) {
        const int n4 = ep.ssq_tiles >> 2;
#pragma unroll
        for (int m = 0; m < RowPre<MR>::NM; ++m) {
          float t = 0.f;
#pragma unroll
          for (int j = 0; j < RowPre<MR>::SSQ4; ++j)
            if (lane + j * 64 < n4)
              t += (pre.ssq_v[m][j][0] + pre.ssq_v[m][j][1]) + (pre.ssq_v[m][j][2] + pre.ssq_v[m][j][3]);
          t = wave_sum(t);
          if (lane == 0 && m < M) rstd_s[m] = rsqrtf(t / (float)K + ep.norm_eps);
        }
      }
    } else {
      skinny_rstd<4>(A, lda, M, K, ep, rstd_s);
    }
  }
  __syncthreads();
  if (tid < M) {
    float v[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      if constexpr (std::is_same<SC, NoColScale>::value) v[c] = red[c][tid];
      else v[c] = red[c][tid] * sc[c];
    }
    if (ep.norm) {
      const float rs = rstd_s[tid];
#pragma unroll
      for (int c = 0; c < 16; ++c) v[c] *= rs;
    }
    const bool fast = pre.full16 && !ep.bias_f32 && !ep.act && !ep.out_f32 && ep.out_group == 0 && !ep.table &&
                      !ep.prelu && !ep.post_act && ep.alpha == 1.f;
    if (fast) {   // bias / residual from the prologue registers (lane tid < M loaded row tid)
      if (pre.pre_bias) {
        float f[8];
        unpack8(pre.pre_b[0], f);
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] += f[q];
        unpack8(pre.pre_b[1], f);
#pragma unroll
        for (int q = 0; q < 8; ++q) v[8 + q] += f[q];
      }
      if (ep.glu) {
        float g[8];
#pragma unroll
        for (int q = 0; q < 8; ++q) g[q] = v[q] * fast_rcp(1.f + __expf(-v[q])) * v[8 + q];
        *(u32x4_t*)((uint16_t*)C + (int64_t)tid * ldc + (n0 >> 1)) = pack8(g);
        return;
      }
      if (pre.pre_res) {
        float f[8];
        unpack8(pre.pre_r[0], f);
#pragma unroll
        for (int q = 0; q < 8; ++q) v[q] += f[q];
        unpack8(pre.pre_r[1], f);
#pragma unroll
        for (int q = 0; q < 8; ++q) v[8 + q] += f[q];
      }
      const u32x4_t o0 = pack8(v), o1 = pack8(v + 8);
      uint16_t* o = (uint16_t*)C + (int64_t)tid * ldc + n0;
      *(u32x4_t*)o = o0;
      *(u32x4_t*)(o + 8) = o1;
      if (ep.ssq_out) {
        float f[16], t = 0.f;
        unpack8(o0, f);
        unpack8(o1, f + 8);
#pragma unroll
        for (int q = 0; q < 16; ++q) t += f[q] * f[q];
        ep.ssq_out[(int64_t)tid * ep.ssq_tiles + (n0 >> 4)] = t;
      }
    } else {
      GemmEpi e2 = ep;
      e2.norm = 0;   // rstd applied above
      epi_store16_dec(v, 1.f, tid, n0, M, N, C, ldc, e2);
    }
  }
}

// ---------------------------------------------------------------------------- split-K, 16-column tiles
// In-launch split-K reduction of the skinny decode GEMMs (the counter form of the
// write-through hand-off, cdna_hip_programming.md §6 G16 / MI355X_MICROARCH.md: per-XCD
// L2s are not coherent, and a __threadfence() per block costs ~4x the whole GEMM).
// Called by every thread once `red` ([4 waves][rows][17] LDS partials) is complete:
//   1. the workgroup's summed partial tile goes to its fp32 slab with agent-scope
//      (sc1, write-through) stores, drained by every wave before the barrier;
//   2. lane 0 draws a ticket from the tile's counter (relaxed agent fetch_add); the
//      workgroup that draws nsplit-1 arrived last, resets the counter (buffer is
//      all-zero between kernels) and tells its waves through red's padding column;
//   3. the last arriver reads every slab with sc1 loads and sums them in split order
//      (deterministic, independent of arrival order) into red[1][m][c].
// No release/acquire fences: sc1 stores leave L2 before the ticket, sc1 loads bypass L1.
template <int NWV, int ROWS>
__device__ __forceinline__ bool splitk_reduce_last(float (&red)[NWV][ROWS][17], float* ws, uint32_t* cnt, int M, int N,
                                                   int n0) {
  const int tid = threadIdx.x;
  const int64_t slab = (int64_t)M * N;
  float* mine = ws + (int64_t)blockIdx.y * slab;
  for (int idx = tid; idx < ROWS * 16; idx += blockDim.x) {
    const int m = idx >> 4, c = idx & 15;
    if (m < M && n0 + c < N) {
      float v = 0.f;
#pragma unroll
      for (int w = 0; w < NWV; ++w) v += red[w][m][c];
      __hip_atomic_store(mine + (int64_t)m * N + n0 + c, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    const uint32_t prev = __hip_atomic_fetch_add(cnt + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const bool last = prev == gridDim.y - 1;
    if (last) __hip_atomic_store(cnt + blockIdx.x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    red[0][0][16] = last ? 1.f : 0.f;
  }
  __syncthreads();
  if (red[0][0][16] == 0.f) return false;
  for (int idx = tid; idx < ROWS * 16; idx += blockDim.x) {
    const int m = idx >> 4, c = idx & 15;
    float v = 0.f;
    if (m < M && n0 + c < N) {
      const float* p = ws + (int64_t)m * N + n0 + c;
      for (int s = 0; s < (int)gridDim.y; ++s)
        v += __hip_atomic_load(p + s * slab, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    red[1][m][c] = v;
  }
  __syncthreads();
  return true;
}

// ---------------------------------------------------------------------------- split-K, wide stripes
// Wave sum and in-launch split-K of a [4 waves][ROWS][COLS + 1] stripe of partials (same hand-off
// as splitk_reduce_last; the wave sum here is (w0 + w1) + (w2 + w3), the 17-column form sums the
// waves left to right, so the two stay apart).  Called by every thread after the barrier that
// publishes `red`.  The wave sum is kept in red[0] (thread-owned elements only: no race); with a
// K split (ws != nullptr) it goes to the write-through slab, and the last split to arrive sums
// the slabs in split order, 8 loads in flight, into red[1].  Returns false in a workgroup that did
// not arrive last; otherwise plane ws != nullptr of `red` holds the result, published by a barrier.
template <int ROWS, int COLS>
__device__ __forceinline__ bool splitk_wide(float (&red)[4][ROWS][COLS + 1], int& last_s, float* ws, uint32_t* cnt,
                                           const int M, const int N, const int n0) {
  const int tid = threadIdx.x;
  for (int i = tid; i < ROWS * COLS; i += 256) {
    const int m = i / COLS, c = i - m * COLS;
    red[0][m][c] = (red[0][m][c] + red[1][m][c]) + (red[2][m][c] + red[3][m][c]);
  }
  if (ws != nullptr) {
    const int64_t slab = (int64_t)M * N;
    for (int i = tid; i < M * COLS; i += 256) {
      const int m = i / COLS, c = i - m * COLS;
      if (n0 + c < N)
        __hip_atomic_store(ws + blockIdx.y * slab + (int64_t)m * N + n0 + c, red[0][m][c], __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
      const uint32_t prev = __hip_atomic_fetch_add(cnt + blockIdx.x, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      const bool last = prev == gridDim.y - 1;
      if (last) __hip_atomic_store(cnt + blockIdx.x, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      last_s = last ? 1 : 0;
    }
    __syncthreads();
    if (!last_s) return false;
    const int S = gridDim.y;
    for (int i = tid; i < M * COLS; i += 256) {
      const int m = i / COLS, c = i - m * COLS;
      const float* p = ws + (int64_t)m * N + min(n0 + c, N - 1);
      float v = 0.f;
      for (int s0 = 0; s0 < S; s0 += 8) {   // 8 slab loads in flight; summed in split order
        float pv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j)
          pv[j] = __hip_atomic_load(p + min(s0 + j, S - 1) * slab, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
        for (int j = 0; j < 8; ++j) v += s0 + j < S ? pv[j] : 0.f;
      }
      red[1][m][c] = v;
    }
  }
  __syncthreads();
  return true;
}

// Epilogue of a wide stripe: thread (row m, 16-column tile t) of the TPW tiles finishes 16 columns
// of plane `src` of red.  sc: per-column multipliers in LDS (16 * TPW floats) or NoColScale.
template <int TPW, int ROWS, class SC>
__device__ __forceinline__ void stripe_store(const float (&red)[4][ROWS][16 * TPW + 1], const int src,
                                             const float* rstd_s, const SC sc, const int n0, const int M, const int N,
                                             void* __restrict__ C, const int64_t ldc, const GemmEpi& ep) {
  const int tid = threadIdx.x;
  if (tid < M * TPW) {
    const int m = tid / TPW, t = tid - m * TPW;
    float v[16];
#pragma unroll
    for (int c = 0; c < 16; ++c) {
      if constexpr (std::is_same<SC, NoColScale>::value) v[c] = red[src][m][t * 16 + c];
      else v[c] = red[src][m][t * 16 + c] * sc[t * 16 + c];
    }
    epi_store16_dec(v, rstd_s[m], m, n0 + t * 16, M, N, C, ldc, ep);
  }
}

// ============================================================================ 16-column skinny kernel
// Split-K MFMA kernel for M <= 32: a workgroup owns one 16-column N tile and a K range; its 4
// waves take interleaved KB-wide k blocks of that range, UNR in flight per wave (split-K inside
// the workgroup, reduced through LDS), and grid.y splits K across workgroups with the in-launch
// reduction above.  Both MFMA operands come straight from global memory in fragment layout: lane
// (col, g) owns k in [g KB / 4, (g + 1) KB / 4) of a block, identically for A row col (rows >= M
// zero) and W row n0 + col, so one 16-byte W load feeds KB / 32 MFMAs.
// W is the weight policy:
//   wt                 element type of a W row
//   KB                 k block width (32: bf16, one MFMA per load; 64: fp8, two)
//   SCALED             a per-column fp32 scale multiplies the summed tile
//   frags(w, f)        16 loaded bytes -> KB / 32 bf16x8 MFMA operands
template <int MT, class W>
__global__ void __launch_bounds__(256) gemm_skinny_kernel(const uint16_t* __restrict__ A, int64_t lda,
                                                          const typename W::wt* __restrict__ Wp, int64_t ldw,
                                                          const float* __restrict__ scale, void* __restrict__ C,
                                                          int64_t ldc, float* __restrict__ ws, uint32_t* __restrict__ cnt,
                                                          int M, int N, int K, int kchunk, GemmEpi ep) {
  constexpr int NWV = 4, UNR = 4, KB = W::KB, NF = KB / 32;
  __shared__ float red[NWV][MT * 16][17];
  __shared__ float rstd_s[MT * 16];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, g = lane >> 4;
  const int n0 = blockIdx.x * 16;
  const int k_begin = blockIdx.y * kchunk;
  const int k_end = min(K, k_begin + kchunk);
  const typename W::wt* wr = Wp + (int64_t)min(n0 + col, N - 1) * ldw + g * (KB / 4);
  const uint16_t* ar[MT];
  bool av[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) {
    const int m = t * 16 + col;
    av[t] = m < M;
    ar[t] = A + (int64_t)(av[t] ? m : 0) * lda + g * (KB / 4);
  }
  f32x4_t acc[MT];
#pragma unroll
  for (int t = 0; t < MT; ++t) acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  auto load_a = [&](const int k, u32x4_t (&a)[MT][NF]) {
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int j = 0; j < NF; ++j) {
        a[t][j] = *(const u32x4_t*)(ar[t] + k + 8 * j);
        if (!av[t]) a[t][j] = (u32x4_t){0u, 0u, 0u, 0u};
      }
  };
  auto mma_block = [&](const u32x4_t w, const u32x4_t (&a)[MT][NF]) {
    bf16x8_t f[NF];
    W::frags(w, f);
#pragma unroll
    for (int t = 0; t < MT; ++t)
#pragma unroll
      for (int j = 0; j < NF; ++j)
        acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a[t][j]), f[j], acc[t], 0, 0, 0);
  };
  // wave wid takes blocks wid, wid + 4, ... (UNR at a time)
  const int nblk = (k_end - k_begin) / KB;
  int s = wid;
  for (; s + NWV * (UNR - 1) < nblk; s += NWV * UNR) {
    u32x4_t wf[UNR];
    u32x4_t af[UNR][MT][NF];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      const int k = k_begin + (s + NWV * u) * KB;
      wf[u] = *(const u32x4_t*)(wr + k);
      load_a(k, af[u]);
    }
#pragma unroll
    for (int u = 0; u < UNR; ++u) mma_block(wf[u], af[u]);
  }
  for (; s < nblk; s += NWV) {
    const int k = k_begin + s * KB;
    const u32x4_t wf = *(const u32x4_t*)(wr + k);
    u32x4_t af[MT][NF];
    load_a(k, af);
    mma_block(wf, af);
  }
  // C fragment: row (m) = t*16 + 4g + r, column n0 + col
#pragma unroll
  for (int t = 0; t < MT; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) red[wid][t * 16 + 4 * g + r][col] = acc[t][r];
  if (ep.norm) skinny_rstd<NWV>(A, lda, M, K, ep, rstd_s);
  __syncthreads();
  // Two copies of the epilogue, one per path: in the unsplit one no store or atomic of the hand-off
  // precedes the column-scale loads, so they stay scalar loads (shared, they turn into 16 vector
  // loads per thread: fp8 M = 32 measured 4 - 7 % slower).
  auto finish = [&](auto&& val) {
    if (tid < M) {
      float v[16];
#pragma unroll
      for (int c = 0; c < 16; ++c) {
        v[c] = val(c);
        if constexpr (W::SCALED) v[c] *= n0 + c < N ? scale[n0 + c] : 0.f;
      }
      epi_store16_dec(v, rstd_s[tid], tid, n0, M, N, C, ldc, ep);
    }
  };
  if (ws != nullptr) {   // K split over grid.y: the last split to arrive reduces + runs the epilogue
    if (!splitk_reduce_last(red, ws, cnt, M, N, n0)) return;
    finish([&](const int c) { return red[1][tid][c]; });
    return;
  }
  finish([&](const int c) { return red[0][tid][c] + red[1][tid][c] + red[2][tid][c] + red[3][tid][c]; });
}

}  // namespace lumen
