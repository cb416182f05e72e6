// The block step shared by the attention kernels over the paged KV pools (llm.hip:
// paged_decode_kernel, paged_prefill_kernel, paged_verify_kernel).  A wave takes one 64-token block
// of one kv head and 16 query columns at a time:
//
//   load_kv_block    every K and V fragment of the block, straight from HBM (layouts in llm.h)
//   zero_v_tail      V lanes past the sequence end -> 0 (any time before pv_step)
//   qk_scores        S^T = K Q^T        four 16-token x 16-column tiles
//   softmax_step     mask, online softmax: scores -> P, running (m, l, o) rescaled
//   pv_step          O^T += V^T P^T
//
// and the workgroup's PA_NW wave states (m, l, o) of a column tile meet in LDS (WaveMerge).
// The kernels keep what differs: which columns, which blocks, what a column may see, where the
// result goes.
//
// Token order.  S^T tile kb16 = (s = kb16 >> 1, hf = kb16 & 1) has MFMA row i <-> token
// 32s + 8(i >> 2) + 4hf + (i & 3) of the block, so its C row 4g + r (lane group g, register r)
// holds token 32s + 8g + 4hf + r: a lane's 8 P values of the two tiles of step s are the 8
// consecutive tokens 32s + 8g .., which the transposed V pool serves with one 16-byte load per
// PV MFMA.  pa_token is that mapping; the K load, the mask and decode's current-token override
// all go through it.
#pragma once
#include <type_traits>

#include "common.h"
#include "llm.h"

namespace lumen {

constexpr int PA_NW = 4;   // waves per workgroup = 1 per SIMD: the 512-VGPR budget holds a whole block's K and V fragments

// token (within its block) of S^T tile kb16, C row 4g + r
__device__ __forceinline__ constexpr int pa_token(int kb16, int g, int r) {
  return 32 * (kb16 >> 1) + 8 * g + 4 * (kb16 & 1) + r;
}

// 8 consecutive elements of pool p from element off as a bf16 fragment.  The pools are typed
// bf16; an fp8 pool holds one byte per element: an 8-byte load, widened.
template <bool F8KV>
__device__ __forceinline__ bf16x8_t pa_load8(const uint16_t* p, int64_t off) {
  if constexpr (F8KV) {
    const uint2 w = *(const uint2*)(reinterpret_cast<const uint8_t*>(p) + off);
    return __builtin_bit_cast(bf16x8_t, fp8x8_to_bf16(w.x, w.y));
  } else {
    return *(const bf16x8_t*)(p + off);
  }
}

// Every K and V fragment of the block at element offset kvo (= bytes for fp8) of the pools, all
// loads back to back: kf[kb16][t] = A operand of S^T tile kb16, k-step t (lane: row col, d range
// 32t + 8g ..); vf[s][j] = A operand of O^T d-block j, token step s (lane: d 16j + col, tokens
// 32s + 8g ..).
template <int D, bool F8KV>
__device__ __forceinline__ void load_kv_block(const uint16_t* k_cache, const uint16_t* v_cache, int64_t kvo, int col,
                                              int g, bf16x8_t (&kf)[4][D / 32], bf16x8_t (&vf)[2][D / 16]) {
#pragma unroll
  for (int kb16 = 0; kb16 < 4; ++kb16) {
    const int tok = pa_token(kb16, col >> 2, col & 3);
#pragma unroll
    for (int t = 0; t < D / 32; ++t) kf[kb16][t] = pa_load8<F8KV>(k_cache, kvo + (int64_t)tok * D + g * 8 + t * 32);
  }
  const int64_t vro = (int64_t)col * KV_BLOCK + 8 * g;
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int j = 0; j < D / 16; ++j) vf[s][j] = pa_load8<F8KV>(v_cache, kvo + vro + 32 * s + (int64_t)j * 16 * KV_BLOCK);
}

// A partial block: V columns past the sequence end get p = 0, but a never-written slot may hold
// a NaN, and 0 * NaN would reach O through the PV MFMA: zero them.
template <int NB>
__device__ __forceinline__ void zero_v_tail(bf16x8_t (&vf)[2][NB], int valid, int g) {
  if (valid < KV_BLOCK) {
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int e = 0; e < 8; ++e)
        if (32 * s + 8 * g + e >= valid) {
#pragma unroll
          for (int j = 0; j < NB; ++j) vf[s][j][e] = (__bf16)0.f;
        }
  }
}

// S^T = K Q^T of the block for one 16-column tile (unscaled)
template <int KS>
__device__ __forceinline__ void qk_scores(const bf16x8_t (&kf)[4][KS], const bf16x8_t (&qf)[KS], f32x4_t (&sc)[4]) {
#pragma unroll
  for (int kb16 = 0; kb16 < 4; ++kb16) {
    sc[kb16] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int t = 0; t < KS; ++t) sc[kb16] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf[kb16][t], qf[t], sc[kb16], 0, 0, 0);
  }
}

// One online-softmax step of a 16-column tile over the block: the column sees the block's first
// `seen` tokens (<= 0: none), the rest go to -inf before the max; (mrow, lrow, o) is the tile's
// running state in the exp2 domain.  Scores in, P out (sc); o is rescaled, pv_step adds the block.
// Needs K only: decode runs it before zero_v_tail, while the V loads are still in flight (zeroing
// first cost 0.15 - 0.45 us per launch at 650 tokens, profiles/paged_attn_refactor_v1.txt).
template <int NB>
__device__ __forceinline__ void softmax_step(f32x4_t (&sc)[4], int seen, float scale_log2, int g, float& mrow, float& lrow,
                                             f32x4_t (&o)[NB]) {
  float mx = mrow;
#pragma unroll
  for (int kb16 = 0; kb16 < 4; ++kb16)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float sv = pa_token(kb16, g, r) < seen ? sc[kb16][r] * scale_log2 : -INFINITY;
      sc[kb16][r] = sv;
      mx = fmaxf(mx, sv);
    }
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));   // over the 4 lane groups (token ranges) of the column
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
  const float mbase = mx == -INFINITY ? 0.f : mx;   // nothing seen yet: exp2(-inf - 0) = 0, not NaN
  const float alpha = __builtin_amdgcn_exp2f(mrow - mbase);
  float rs = 0.f;
#pragma unroll
  for (int kb16 = 0; kb16 < 4; ++kb16)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float p = __builtin_amdgcn_exp2f(sc[kb16][r] - mbase);
      sc[kb16][r] = p;
      rs += p;
    }
  rs += __shfl_xor(rs, 16, 64);
  rs += __shfl_xor(rs, 32, 64);
  lrow = lrow * alpha + rs;
  mrow = mx;
#pragma unroll
  for (int j = 0; j < NB; ++j) o[j] *= alpha;
}

// O^T += V^T P^T over two 32-token steps; lane's P k-slots 8g + j = tokens 32s + 8g + j
template <int NB>
__device__ __forceinline__ void pv_step(const f32x4_t (&sc)[4], const bf16x8_t (&vf)[2][NB], f32x4_t (&o)[NB]) {
#pragma unroll
  for (int s = 0; s < 2; ++s) {
    bf16x8_t pf;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      pf[r] = (__bf16)sc[2 * s][r];
      pf[4 + r] = (__bf16)sc[2 * s + 1][r];
    }
#pragma unroll
    for (int j = 0; j < NB; ++j) o[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf[s][j], pf, o[j], 0, 0, 0);
  }
}

// LDS meeting point of the workgroup's PA_NW wave states of one 16-column tile
template <int D>
struct WaveMerge {
  float ml[PA_NW][2][16];
  float o[PA_NW][D][17];

  // wave wid's state; __syncthreads() before reduce
  __device__ __forceinline__ void store(int wid, int col, int g, float mrow, float lrow, const f32x4_t (&acc)[D / 16]) {
    if (g == 0) {
      ml[wid][0][col] = mrow;
      ml[wid][1][col] = lrow;
    }
#pragma unroll
    for (int j = 0; j < D / 16; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) o[wid][j * 16 + 4 * g + r][col] = acc[j][r];
  }

  // (max, sum, unnormalised output) of column q, element d over all waves; all -inf: (-inf, 0, 0)
  __device__ __forceinline__ void reduce(int q, int d, float& M, float& L, float& O) const {
    M = -INFINITY;
#pragma unroll
    for (int w = 0; w < PA_NW; ++w) M = fmaxf(M, ml[w][0][q]);
    L = 0.f;
    O = 0.f;
    if (M != -INFINITY) {
#pragma unroll
      for (int w = 0; w < PA_NW; ++w) {
        const float e = __builtin_amdgcn_exp2f(ml[w][0][q] - M);
        L += ml[w][1][q] * e;
        O += o[w][d][q] * e;
      }
    }
  }
};

// ---- in-launch combine of a context split over several workgroups (decode, verify): every split
// publishes its (m, l, o) partials with write-through stores (publish_split), waits for them
// (s_waitcnt vmcnt(0) + __syncthreads()), draws a ticket (split_ticket), and the last to arrive
// merges all of them (merge_splits).  part_o [.., nsplit, D], part_ml [.., nsplit, 2]; pi = index
// of the (row, head, split) record.

template <int D>
__device__ __forceinline__ void publish_split(float* part_o, float* part_ml, int64_t pi, int d, float M, float L, float O) {
  __hip_atomic_store(part_o + pi * D + d, O, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (d == 0) {
    __hip_atomic_store(part_ml + pi * 2, M, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_store(part_ml + pi * 2 + 1, L, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

// one thread per workgroup: true for the last of the ns splits to arrive, which also re-zeroes the
// counter for the next launch
__device__ __forceinline__ bool split_ticket(uint32_t* c, int ns) {
  const uint32_t prev = __hip_atomic_fetch_add(c, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const bool last = prev == (uint32_t)ns - 1;
  if (last) __hip_atomic_store(c, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return last;
}

// element d of the normalised output over the ns split records from pi0.  One round trip per 8
// splits: every (m, l) and o partial of a chunk is loaded before any is used (the chunk's max
// rescales the running sums, online-softmax style); split order: deterministic
template <int D>
__device__ __forceinline__ float merge_splits(const float* part_o, const float* part_ml, int64_t pi0, int ns, int d) {
  float M = -INFINITY, L = 0.f, O = 0.f;
  for (int s0 = 0; s0 < ns; s0 += 8) {
    float pm[8], pl[8], pv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const int64_t pi = pi0 + min(s0 + j, ns - 1);
      pm[j] = __hip_atomic_load(part_ml + pi * 2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      pl[j] = __hip_atomic_load(part_ml + pi * 2 + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      pv[j] = __hip_atomic_load(part_o + pi * D + d, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    float mc = M;
#pragma unroll
    for (int j = 0; j < 8; ++j) mc = s0 + j < ns ? fmaxf(mc, pm[j]) : mc;
    if (mc == -INFINITY) continue;
    const float r = __builtin_amdgcn_exp2f(M - mc);   // M = -inf: 0 (L, O still 0)
    L *= r;
    O *= r;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      if (s0 + j < ns) {
        const float e = __builtin_amdgcn_exp2f(pm[j] - mc);
        L += pl[j] * e;
        O += pv[j] * e;
      }
    }
    M = mc;
  }
  return L > 0.f ? O / L : 0.f;
}

// Host: f(integral_constant<int, D>, bool_constant<fp8 cache>) for the head dims the paged kernels
// are built for; false = unsupported head dim, f not called.
template <class F>
inline bool pa_dispatch(int D, bool kv_fp8, F&& f) {
  auto with_d = [&](auto d) {
    if (kv_fp8) f(d, std::true_type{});
    else f(d, std::false_type{});
  };
  if (D == 64) with_d(std::integral_constant<int, 64>{});
  else if (D == 128) with_d(std::integral_constant<int, 128>{});
  else if (D == 32) with_d(std::integral_constant<int, 32>{});
  else return false;
  return true;
}

}  // namespace lumen
