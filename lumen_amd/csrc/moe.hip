// Sparse mixture-of-experts MLP for the Qwen3-MoE decoders: route -> group -> expert GEMMs -> combine.
//
//   moe_gemm_kernel<MT, MOE_LOGITS>   router logits x . gate_w^T in fp32     grid (ceil(E / 16), ceil(T / 16 MT))
//   moe_topk_kernel                   top-k of a row + its weights, 1 wave   grid (ceil(T / 4))
//   moe_group_kernel                  stable counting sort by expert         grid (1), 1024 threads
//   moe_gemm_kernel<MT, MOE_GATE_UP>  g = silu(x Wg^T) * (x Wu^T) per expert grid (2I / 16, min(E, T k))
//   moe_gemm_kernel<MT, MOE_DOWN>     y = g Wd^T per expert, fp32            grid (H / 16, min(E, T k))
//   moe_combine_kernel                out = residual + sum_j w_j y_j         grid (T, ceil(H / 2048))
//
// Every grid is a function of (T, E, k, H, I) only and nothing is read back on the host, so a
// captured graph replays for any routing.  The GEMM is a sibling of gemm_skinny_kernel
// (gemm_wdec.h): a workgroup owns one 16-column stripe of ONE expert, both MFMA operands come
// straight from global memory in fragment layout and its 4 waves split K, reduced through LDS.
// What it adds is the row indirection (activation rows are gathered through the sorted order) and
// the expert stride on the weights.  grid.y indexes the list of NON-EMPTY experts the group kernel
// compacts (at most min(E, T k) of them), so a decode step launches no workgroup for the ~120 idle
// experts; workgroups past the list's end leave at once.  The expert's rows are walked MT * 16 at a
// time: MT = 1 for decode / verify (an expert holds 0 - 4 rows, the kernel is bound by the weight
// stream), MT = 4 for prefill so the stripe's weights are re-read once per 64 rows.
// No floating-point atomics and no cross-workgroup reduction anywhere: every output element is
// summed in one fixed order, so results are bit-identical from run to run.
// The GEMM kernel itself is moe_gemm.h; this file instantiates it for bf16 weights (MoeBf16), the
// fp8 and 4-bit expert instantiations are moe_wq.hip.
#include "common.h"
#include "moe.h"
#include "moe_gemm.h"

namespace lumen {

// ---------------------------------------------------------------------------------------- top-k
// One wave per token: k rounds of a wave-wide arg-max over the row's E <= 256 logits (4 per lane),
// ties to the lower expert id, then the weights: the softmax over the k chosen logits, or
// exp(l_j - logsumexp(l over all E)).  NaN logits count as -inf.  (A rank-counting top-k through
// LDS, alone and fused with the grouping into one launch, measured slower: profiles/moe_v1.txt.)
__global__ void __launch_bounds__(256) moe_topk_kernel(const float* __restrict__ logits, const int T, const int E,
                                                       const int k, const int norm_topk, int* __restrict__ ids,
                                                       float* __restrict__ w) {
  constexpr int NONE = 0x7fffffff;
  const int lane = threadIdx.x & 63;
  const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (t >= T) return;
  float v[4];
  unsigned taken = 0;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int e = lane + 64 * j;
    float x = -INFINITY;
    if (e < E) x = logits[(int64_t)t * E + e];
    else taken |= 1u << j;
    v[j] = x != x ? -INFINITY : x;
  }
  float selv[MOE_MAX_TOPK];
  int seli[MOE_MAX_TOPK];
#pragma unroll
  for (int s = 0; s < MOE_MAX_TOPK; ++s) {
    selv[s] = -INFINITY;
    seli[s] = NONE;
    if (s < k) {
      float bv = -INFINITY;
      int bi = NONE;
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (!((taken >> j) & 1u) && (bi == NONE || v[j] > bv)) {
          bv = v[j];
          bi = lane + 64 * j;
        }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const float ov = __shfl_xor(bv, o, 64);
        const int oi = __shfl_xor(bi, o, 64);
        if (ov > bv || (ov == bv && oi < bi)) {
          bv = ov;
          bi = oi;
        }
      }
      selv[s] = bv;
      seli[s] = bi;
      if (bi != NONE && (bi & 63) == lane) taken |= 1u << (bi >> 6);
    }
  }
  const float mx = selv[0];
  float den = 0.f;
  if (norm_topk) {
#pragma unroll
    for (int s = 0; s < MOE_MAX_TOPK; ++s)
      if (s < k) den += expf(selv[s] - mx);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (lane + 64 * j < E) den += expf(v[j] - mx);
    den = wave_sum(den);
  }
#pragma unroll
  for (int s = 0; s < MOE_MAX_TOPK; ++s)
    if (s < k && lane == s) {
      ids[(int64_t)t * k + s] = seli[s];
      w[(int64_t)t * k + s] = expf(selv[s] - mx) / den;
    }
}

// ---------------------------------------------------------------------------------------- group
// Stable counting sort of the P = T k pairs by expert, one workgroup of 16 waves.  Every wave walks
// the pairs in order, 256 per step (4 independent loads in flight), and for each of the <= 16
// experts it owns (wave v: v, v + 16, ...) a ballot gives every matching pair its rank within the
// expert (stable: pair order is kept).  Wave 0 then scans the counts (offsets, list of non-empty
// experts) and a last pass turns ranks into sorted positions.  An id outside [0, E) matches no
// expert: its pair gets position -1 and is never used as an index.
// Cost: P / 64 x E / 16 ballot rounds per wave in ONE workgroup, i.e. linear in the prefill length
// on one CU (measured in profiles/moe_v1.txt); the ops admit T k <= 2^20.  A multi-workgroup
// histogram sort is the step after this one.
__global__ void __launch_bounds__(1024) moe_group_kernel(const int* ids, const int P, const int E, const int k,
                                                         int* __restrict__ cnt, int* __restrict__ off,
                                                         int* __restrict__ active, int* pos, int* __restrict__ src_tok) {
  constexpr int EPW = MOE_MAX_EXPERTS / 16;   // experts per wave
  __shared__ int s_cnt[MOE_MAX_EXPERTS], s_off[MOE_MAX_EXPERTS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const unsigned long long below = (1ull << lane) - 1ull;
  int run[EPW];
#pragma unroll
  for (int q = 0; q < EPW; ++q) run[q] = 0;
  for (int p0 = 0; p0 < P; p0 += 256) {
    int id[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int p = p0 + 64 * u + lane;
      id[u] = p < P ? ids[p] : -1;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int q = 0; q < EPW; ++q) {
        const int e = wid + 16 * q;
        if (e < E) {   // wave-uniform
          const bool hit = id[u] == e;
          const unsigned long long m = __ballot(hit);
          if (hit) pos[p0 + 64 * u + lane] = run[q] + __popcll(m & below);
          run[q] += __popcll(m);
        }
      }
  }
#pragma unroll
  for (int q = 0; q < EPW; ++q)
    if (wid + 16 * q < E && lane == 0) s_cnt[wid + 16 * q] = run[q];
  __syncthreads();
  if (wid == 0) {   // lane l: experts 4 l .. 4 l + 3
    int c[4], tot = 0, nz = 0;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = 4 * lane + q;
      c[q] = e < E ? s_cnt[e] : 0;
      tot += c[q];
      nz += c[q] > 0;
    }
    int itot = tot, inz = nz;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int a = __shfl_up(itot, o, 64), b = __shfl_up(inz, o, 64);
      if (lane >= o) {
        itot += a;
        inz += b;
      }
    }
    int o_run = itot - tot, a_run = inz - nz;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int e = 4 * lane + q;
      if (e < E) {
        s_off[e] = o_run;
        off[e] = o_run;
        cnt[e] = c[q];
        if (c[q] > 0) active[a_run++] = e;
        o_run += c[q];
      }
    }
    if (lane == 63) active[E] = inz;
  }
  __syncthreads();   // also orders the rank stores to pos (global) before the reads below
  for (int p = tid; p < P; p += 1024) {
    const int id = ids[p];
    if (id >= 0 && id < E) {
      const int sp = s_off[id] + pos[p];
      pos[p] = sp;
      src_tok[sp] = p / k;
    } else {
      pos[p] = -1;
    }
  }
}

// out[t, c0 .. c0 + 8) = residual + sum_j w[t, j] * y[pos[t k + j]]; the thread reads its residual
// elements before it writes them, so residual may alias out.
__global__ void __launch_bounds__(256) moe_combine_kernel(const float* __restrict__ y, const int* __restrict__ pos,
                                                          const float* __restrict__ w, const uint16_t* residual,
                                                          const int64_t ldr, uint16_t* out, const int64_t ldo,
                                                          const int k, const int H) {
  const int t = blockIdx.x;
  const int c0 = (blockIdx.y * 256 + threadIdx.x) * 8;
  if (c0 >= H) return;
  float acc[8];
#pragma unroll
  for (int q = 0; q < 8; ++q) acc[q] = 0.f;
  for (int j = 0; j < k; ++j) {
    const int p = pos[(int64_t)t * k + j];
    if (p < 0) continue;
    const float wj = w[(int64_t)t * k + j];
    const f32x4_t* yp = (const f32x4_t*)(y + (int64_t)p * H + c0);
    const f32x4_t y0 = yp[0], y1 = yp[1];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      acc[q] = fmaf(wj, y0[q], acc[q]);
      acc[4 + q] = fmaf(wj, y1[q], acc[4 + q]);
    }
  }
  if (residual != nullptr) {
    float r[8];
    unpack8(*(const u32x4_t*)(residual + (int64_t)t * ldr + c0), r);
#pragma unroll
    for (int q = 0; q < 8; ++q) acc[q] += r[q];
  }
  *(u32x4_t*)(out + (int64_t)t * ldo + c0) = pack8(acc);
}

// ---------------------------------------------------------------------------------------- host
hipError_t moe_route(const uint16_t* x, int64_t ldx, const uint16_t* gate_w, int T, int E, int k, int H, int norm_topk,
                     float* logits, int* ids, float* w, hipStream_t stream) {
  MoeGemmArgs a{};
  a.A = x; a.lda = ldx;
  a.W = gate_w; a.w_stride = 0;
  a.C = logits; a.ldc = E;
  a.M = T; a.N = E; a.K = H; a.E = E;
  const dim3 block(256);
  if (T <= 32) {
    const dim3 grid((E + 15) / 16, (T + 15) / 16);
    hipLaunchKernelGGL((moe_gemm_kernel<1, MOE_LOGITS, MoeBf16>), grid, block, 0, stream, a);
  } else {
    const dim3 grid((E + 15) / 16, (T + 63) / 64);
    hipLaunchKernelGGL((moe_gemm_kernel<4, MOE_LOGITS, MoeBf16>), grid, block, 0, stream, a);
  }
  hipLaunchKernelGGL(moe_topk_kernel, dim3((T + 3) / 4), block, 0, stream, logits, T, E, k, norm_topk, ids, w);
  return hipGetLastError();
}

hipError_t moe_group(const int* ids, int T, int E, int k, const MoeWork& work, hipStream_t stream) {
  hipLaunchKernelGGL(moe_group_kernel, dim3(1), dim3(1024), 0, stream, ids, T * k, E, k, work.cnt, work.off, work.active,
                     work.pos, work.src_tok);
  return hipGetLastError();
}

hipError_t moe_expert_gemms(const uint16_t* x, int64_t ldx, const uint16_t* gu_w, const uint16_t* down_w, int T, int E,
                            int k, int H, int I, const MoeWork& work, hipStream_t stream) {
  return moe_launch_experts<MoeBf16>(x, ldx, gu_w, nullptr, down_w, nullptr, (int64_t)2 * I * H, (int64_t)H * I, 0, 0, T, E,
                                     k, H, I, work, stream);
}

hipError_t moe_grouped_gemm(const uint16_t* x, int64_t ldx, const uint16_t* w, int T, int E, int k, int N, int K,
                            const MoeWork& work, hipStream_t stream) {
  return moe_launch_grouped<MoeBf16>(x, ldx, w, nullptr, (int64_t)N * K, 0, T, E, k, N, K, work, stream);
}

hipError_t moe_combine(const float* w, const uint16_t* residual, int64_t ldr, uint16_t* out, int64_t ldo, int T, int k,
                       int H, const MoeWork& work, hipStream_t stream) {
  hipLaunchKernelGGL(moe_combine_kernel, dim3(T, (H / 8 + 255) / 256), dim3(256), 0, stream, work.y, work.pos, w,
                     residual, ldr, out, ldo, k, H);
  return hipGetLastError();
}

}  // namespace lumen
