// Decoder-LLM kernels for the VLM (Qwen2 / Qwen3 / Llama family):
//
//  * rope_kv: rotary embedding (rotate-half, HF convention) applied in place to
//    the q and k heads of the packed QKV projection, fused with the paged KV
//    cache write (k token-major, v transposed; layouts in llm.h).  Prefill
//    attention then reads q/k/v straight from the rotated QKV buffer.  Qwen3:
//    every q / k head first passes through an RMSNorm over the head dim
//    (template flag NORM of both kernel forms).  Qwen-VL prefill: multimodal RoPE, three
//    positions per token and an axis per rotary frequency (template flag MROPE of both forms).
//  * paged_decode: flash-decoding over the paged cache.  One workgroup per
//    (split, kv-head, sequence); the G = H / Hkv query heads sharing a kv head
//    are the 16 MFMA columns, each wave walks its own 64-token blocks with an
//    online softmax, the 4 wave states are merged through LDS and — when the
//    context is split across workgroups — the last split to finish merges them
//    (in-launch, ticket counter; no combine kernel).
//  * paged_prefill: attention of a chunk of new query rows over the paged cache (chunked
//    prefill, prefix reuse) with (query row, head) pairs as the MFMA columns and a causal
//    mask per column.
//  * paged_verify: up to T new query rows for each of B sequences in one launch (speculative
//    decoding): prefill's column mapping on decode's (split, kv-head, sequence) grid and
//    in-launch split combine, every per-step quantity read from device memory.
//    All three paged kernels are bookkeeping around ONE block step, paged_attn.h: the K / V
//    fragment loads straight from HBM (S^T = K Q^T reads K rows in a permuted token order
//    chosen so that each lane's 8 P values are 8 consecutive tokens, which the transposed
//    V cache serves with one 16-byte load per MFMA of O^T = V^T P^T), the online-softmax /
//    PV step, and the LDS merge of the wave states.
//  * rep_penalty: repetition penalty on the logits of previously generated
//    tokens (the reference accepts and ignores it, SURVEY V-7).
#include "common.h"
#include "llm.h"
#include "paged_attn.h"

namespace lumen {

// ------------------------------------------------------------------------------ RoPE + KV write
// grid (T, nrot_blocks + v_blocks): one (token, 256-element chunk) per workgroup and ONE
// rotation pair / V element per thread, so a decode step (T = 1..16) spreads over 14+
// workgroups per token instead of looping 10x inside one (each pass of that loop paid a
// dependent global round trip: 8 us per layer per token, measured)
//
// NORM (per-head q / k RMSNorm, llm.h): a head's D/2 pairs are 16, 32 or 64 consecutive threads,
// a segment aligned inside one wave (256 is a multiple of D/2), so the head's sum of squares is a
// xor-butterfly over the segment.  The bound below cuts at a head boundary: a segment is wholly
// in or wholly out, and the threads past it leave only after the butterfly.
__device__ __forceinline__ float qk_rstd(float ssq, int D, float eps) { return rsqrtf(ssq / (float)D + eps); }

// MROPE (llm.h): pos is [3, T] and frequency i reads the table row of the axis its two-bit code names.
// The codes are kernel arguments, so the per-element form adds one pos load of a computed row and the
// tile form three pos loads per thread; neither adds a load that another depends on.
__device__ __forceinline__ int mrope_axis(const RopeKVArgs& a, int i) {
  return (int)((i < 32 ? a.mrope_axes[0] : a.mrope_axes[1]) >> ((i & 31) * 2)) & 3;
}

template <bool NORM, bool MROPE>
__global__ void __launch_bounds__(256) rope_kv_kernel(RopeKVArgs a, int nrot_blocks) {
  const int t = blockIdx.x;
  const int half = a.D >> 1;
  uint16_t* row = a.qkv + (int64_t)t * a.ld;
  const int64_t slot = a.slots ? a.slots[t] : -1;
  const int64_t blk = slot >= 0 ? (slot >> 6) : 0;
  const int off = (int)(slot & 63);
  if ((int)blockIdx.y < nrot_blocks) {
    int idx = blockIdx.y * 256 + threadIdx.x;
    const bool live = idx < (a.H + a.Hkv) * half;
    if constexpr (NORM) {
      if (!live) idx = 0;   // reads head 0 again, stores nothing
    } else {
      if (!live) return;
    }
    const int p = MROPE ? 0 : a.pos[t];
    const float2* cs = reinterpret_cast<const float2*>(a.cos_sin) + (int64_t)p * half;
    const int hh = idx / half, i = idx - hh * half;
    if constexpr (MROPE) cs += (int64_t)a.pos[(int64_t)mrope_axis(a, i) * a.T + t] * half;   // the row of i's axis
    uint16_t* hp = row + hh * a.D;
    float x1 = bf2f(hp[i]), x2 = bf2f(hp[i + half]);
    if constexpr (NORM) {
      float ssq = x1 * x1 + x2 * x2;
      for (int m = 1; m < half; m <<= 1) ssq += __shfl_xor(ssq, m, 64);
      const float rstd = qk_rstd(ssq, a.D, a.eps);
      const float* gm = hh < a.H ? a.q_gamma : a.k_gamma;
      x1 = x1 * rstd * gm[i];
      x2 = x2 * rstd * gm[i + half];
      if (!live) return;
    }
    const float2 c = cs[i];
    const float y1 = x1 * c.x - x2 * c.y, y2 = x2 * c.x + x1 * c.y;
    const uint16_t b1 = f2bf(y1), b2 = f2bf(y2);
    hp[i] = b1;
    hp[i + half] = b2;
    if (hh >= a.H && slot >= 0) {
      const int64_t ko = ((blk * a.Hkv + (hh - a.H)) * KV_BLOCK + off) * a.D;
      if (a.kv_fp8) {
        uint8_t* kr = reinterpret_cast<uint8_t*>(a.k_cache) + ko;
        kr[i] = f2fp8(bf2f(b1));
        kr[i + half] = f2fp8(bf2f(b2));
      } else {
        uint16_t* kr = a.k_cache + ko;
        kr[i] = b1;
        kr[i + half] = b2;
      }
    }
    return;
  }
  if (slot < 0) return;
  const int idx = (blockIdx.y - nrot_blocks) * 256 + threadIdx.x;
  if (idx >= a.Hkv * a.D) return;
  const uint16_t* vr = row + (a.H + a.Hkv) * a.D;
  const int kh = idx / a.D, d = idx - kh * a.D;
  const int64_t vo = ((blk * a.Hkv + kh) * a.D + d) * KV_BLOCK + off;
  if (a.kv_fp8) reinterpret_cast<uint8_t*>(a.v_cache)[vo] = f2fp8(bf2f(vr[idx]));
  else a.v_cache[vo] = vr[idx];
}

// Prefill form (T >= 64): one workgroup per (64-token tile, head) with 16-byte accesses.  q / k
// heads: each thread rotates D/8 pairs of one token (4 threads per token) in place and writes the
// k cache rows; v heads: the [64 x D] tile goes through LDS and leaves d-major, 8 tokens (16 or
// 8 bytes) per store when their slots are consecutive in one block.  The per-element kernel above
// wrote V with 2-byte stores 128 bytes apart (11 us per 8B-prefill layer at 624 tokens).
// NORM: the 4 adjacent threads of a (token, head) each sum the D/4 squares of the values they hold;
// two xor steps over the quad give the head's sum (a quad leaves together at the ragged last tile).
// MROPE: a thread's PPT consecutive frequencies are PPT two-bit codes of one argument word, shifted
// down once; each unrolled pair picks one of the token's three table rows by a constant-shift code, so
// only the 8-byte (cos, sin) loads become gathers (the interleaved layout changes row on every pair).
template <int D, bool NORM, bool MROPE>
__global__ void __launch_bounds__(256) rope_kv_tile_kernel(RopeKVArgs a) {
  constexpr int HALF = D / 2, PPT = D / 8;       // rotation pairs per thread
  __shared__ __attribute__((aligned(16))) uint16_t vt[64][D + 8];
  __shared__ int64_t sl[64];
  const int t0 = blockIdx.x * 64, hh = blockIdx.y, tid = threadIdx.x;
  if (hh < a.H + a.Hkv) {
    const int tt = tid >> 2, c0 = (tid & 3) * PPT, t = t0 + tt;
    if (t >= a.T) return;
    uint16_t* hp = a.qkv + (int64_t)t * a.ld + hh * D;
    // (MROPE: cs is row 0 of the table and each pair adds the row of its axis)
    const float2* cs = reinterpret_cast<const float2*>(a.cos_sin) + (int64_t)(MROPE ? 0 : a.pos[t]) * HALF + c0;
    int row_t = 0, row_h = 0, row_w = 0;      // MROPE: first table element of the token's three rows (< 2^31)
    uint32_t codes = 0;                       // MROPE: the axis codes of pairs c0 .. c0 + PPT - 1
    if constexpr (MROPE) {
      row_t = a.pos[t] * HALF;
      row_h = a.pos[(int64_t)a.T + t] * HALF;
      row_w = a.pos[2 * (int64_t)a.T + t] * HALF;
      codes = (uint32_t)((c0 < 32 ? a.mrope_axes[0] : a.mrope_axes[1]) >> ((c0 & 31) * 2));
    }
    u32x4_t raw1[PPT / 8], raw2[PPT / 8];   // NORM: the thread's values, held across the reduction
    float g1[PPT], g2[PPT];                 // NORM: gamma of each element, 16-byte loads
    float rstd = 1.f;
    if constexpr (NORM) {
      float ssq = 0.f;
#pragma unroll
      for (int u = 0; u < PPT; u += 8) {
        float x1[8], x2[8];
        raw1[u / 8] = *(const u32x4_t*)(hp + c0 + u);
        raw2[u / 8] = *(const u32x4_t*)(hp + HALF + c0 + u);
        unpack8(raw1[u / 8], x1);
        unpack8(raw2[u / 8], x2);
#pragma unroll
        for (int q = 0; q < 8; ++q) ssq += x1[q] * x1[q] + x2[q] * x2[q];
      }
      const float* gm = (hh < a.H ? a.q_gamma : a.k_gamma) + c0;
#pragma unroll
      for (int u = 0; u < PPT; u += 4) {
        const float4 ga = *(const float4*)(gm + u), gb = *(const float4*)(gm + HALF + u);
        g1[u] = ga.x; g1[u + 1] = ga.y; g1[u + 2] = ga.z; g1[u + 3] = ga.w;
        g2[u] = gb.x; g2[u + 1] = gb.y; g2[u + 2] = gb.z; g2[u + 3] = gb.w;
      }
      ssq += __shfl_xor(ssq, 1, 64);
      ssq += __shfl_xor(ssq, 2, 64);
      rstd = qk_rstd(ssq, D, a.eps);
    }
    float y1[PPT], y2[PPT];
#pragma unroll
    for (int u = 0; u < PPT; u += 8) {
      float x1[8], x2[8];
      if constexpr (NORM) {
        unpack8(raw1[u / 8], x1);
        unpack8(raw2[u / 8], x2);
#pragma unroll
        for (int q = 0; q < 8; ++q) {
          x1[q] = x1[q] * rstd * g1[u + q];
          x2[q] = x2[q] * rstd * g2[u + q];
        }
      } else {
        unpack8(*(const u32x4_t*)(hp + c0 + u), x1);
        unpack8(*(const u32x4_t*)(hp + HALF + c0 + u), x2);
      }
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        float2 c;
        if constexpr (MROPE) {
          const uint32_t ax = (codes >> (2 * (u + q))) & 3u;
          c = cs[(ax == 1u ? row_h : ax == 2u ? row_w : row_t) + u + q];
        } else {
          c = cs[u + q];
        }
        y1[u + q] = x1[q] * c.x - x2[q] * c.y;
        y2[u + q] = x2[q] * c.x + x1[q] * c.y;
      }
      *(u32x4_t*)(hp + c0 + u) = pack8(y1 + u);
      *(u32x4_t*)(hp + HALF + c0 + u) = pack8(y2 + u);
    }
    const int64_t slot = a.slots && hh >= a.H ? a.slots[t] : -1;
    if (slot >= 0) {
      const int64_t ko = (((slot >> 6) * a.Hkv + (hh - a.H)) * KV_BLOCK + (slot & 63)) * D;
#pragma unroll
      for (int u = 0; u < PPT; u += 8) {
        float r1[8], r2[8];   // the stored (bf16-rounded) values, as the per-element kernel caches them
        unpack8(pack8(y1 + u), r1);
        unpack8(pack8(y2 + u), r2);
        if (a.kv_fp8) {
          uint8_t* kr = reinterpret_cast<uint8_t*>(a.k_cache) + ko;
          *(uint2*)(kr + c0 + u) = fp8x8_scaled(r1, 1.f);
          *(uint2*)(kr + HALF + c0 + u) = fp8x8_scaled(r2, 1.f);
        } else {
          *(u32x4_t*)(a.k_cache + ko + c0 + u) = pack8(r1);
          *(u32x4_t*)(a.k_cache + ko + HALF + c0 + u) = pack8(r2);
        }
      }
    }
    return;
  }
  if (a.slots == nullptr) return;
  const int kh = hh - a.H - a.Hkv;
  if (tid < 64) sl[tid] = t0 + tid < a.T ? a.slots[t0 + tid] : -1;
  constexpr int CPR = D / 8;                       // 16-byte chunks per token row
  for (int c = tid; c < 64 * CPR; c += 256) {
    const int tt = c / CPR, ch = c % CPR;
    if (t0 + tt < a.T)
      *(u32x4_t*)&vt[tt][ch * 8] = *(const u32x4_t*)(a.qkv + (int64_t)(t0 + tt) * a.ld + (a.H + a.Hkv + kh) * D + ch * 8);
  }
  __syncthreads();
  // thread -> (d, run of 8 tokens)
  for (int w = tid; w < D * 8; w += 256) {
    const int d = w % D, g8 = w / D;
    const int64_t s0 = sl[g8 * 8];
    bool run = s0 >= 0 && (s0 & 7) == 0;
#pragma unroll
    for (int q = 1; q < 8; ++q) run = run && sl[g8 * 8 + q] == s0 + q;
    if (run) {
      const int64_t vo = (((s0 >> 6) * a.Hkv + kh) * D + d) * KV_BLOCK + (s0 & 63);
      float f[8];
#pragma unroll
      for (int q = 0; q < 8; ++q) f[q] = bf2f(vt[g8 * 8 + q][d]);
      if (a.kv_fp8) *(uint2*)(reinterpret_cast<uint8_t*>(a.v_cache) + vo) = fp8x8_scaled(f, 1.f);
      else *(u32x4_t*)(a.v_cache + vo) = pack8(f);
    } else {
#pragma unroll
      for (int q = 0; q < 8; ++q) {
        const int64_t s = sl[g8 * 8 + q];
        if (s < 0) continue;
        const int64_t vo = (((s >> 6) * a.Hkv + kh) * D + d) * KV_BLOCK + (s & 63);
        if (a.kv_fp8) reinterpret_cast<uint8_t*>(a.v_cache)[vo] = f2fp8(bf2f(vt[g8 * 8 + q][d]));
        else a.v_cache[vo] = vt[g8 * 8 + q][d];
      }
    }
  }
}

hipError_t rope_kv(const RopeKVArgs& a, hipStream_t stream) {
  if (a.T == 0) return hipSuccess;
  const bool norm = a.q_gamma != nullptr;
  // the norm's segmented butterfly needs a power-of-two D/2 that divides the wave
  if (norm && (a.k_gamma == nullptr || !(a.D == 32 || a.D == 64 || a.D == 128))) return hipErrorInvalidValue;
  const bool mrope = a.mrope != 0;
  if (mrope && a.D > 128) return hipErrorInvalidValue;   // two words hold 64 axis codes
  if (a.T >= 64 && (a.D == 64 || a.D == 128) && a.ld % 8 == 0) {
    const dim3 grid((a.T + 63) / 64, a.H + 2 * a.Hkv);
    auto tile = a.D == 128
        ? (norm ? (mrope ? rope_kv_tile_kernel<128, true, true> : rope_kv_tile_kernel<128, true, false>)
                : (mrope ? rope_kv_tile_kernel<128, false, true> : rope_kv_tile_kernel<128, false, false>))
        : (norm ? (mrope ? rope_kv_tile_kernel<64, true, true> : rope_kv_tile_kernel<64, true, false>)
                : (mrope ? rope_kv_tile_kernel<64, false, true> : rope_kv_tile_kernel<64, false, false>));
    hipLaunchKernelGGL(tile, grid, dim3(256), 0, stream, a);
    return hipGetLastError();
  }
  const int nrot_blocks = ((a.H + a.Hkv) * (a.D / 2) + 255) / 256;
  const int v_blocks = a.slots ? (a.Hkv * a.D + 255) / 256 : 0;
  const dim3 grid(a.T, nrot_blocks + v_blocks);
  auto elem = norm ? (mrope ? rope_kv_kernel<true, true> : rope_kv_kernel<true, false>)
                   : (mrope ? rope_kv_kernel<false, true> : rope_kv_kernel<false, false>);
  hipLaunchKernelGGL(elem, grid, dim3(256), 0, stream, a, nrot_blocks);
  return hipGetLastError();
}

// ------------------------------------------------------------------------------ paged decode attention
// One workgroup of PA_NW = 4 waves per (split, kv head, sequence); wave w takes the split's
// 64-token blocks w, w + 4, ...  The launch has at most 32 splits (ops/llm.py decode_splits):
// batched decode gives a split >= 4 blocks, so a context of <= 256 tokens is ONE workgroup per kv
// head; a few sequences get no minimum, so their blocks spread over all launched splits.  Either
// way a wave has one block up to 8k tokens (32 splits x 4 waves); past that the waves loop over
// their blocks with an online softmax.  The latency chain per wave is:
// block-table entry -> every K and V fragment of the block in flight at once -> S^T = K Q^T,
// online softmax, O^T += V^T P^T (the block step of paged_attn.h); the 4 wave states merge
// through LDS.  Fused RoPE mode (decode): q and the current token's k are rotated in
// registers, and the current token enters the wave that owns its block straight from registers
// (its score q . k_cur as a lane-group dot product, its v into the V fragment) -- the cache
// write of that token is fire-and-forget (the next step reads it), so no workgroup waits for a
// store round trip.  A context split over several workgroups is
// combined IN the launch: every split publishes its (m, l, o) partials with write-through (sc1)
// stores, draws a ticket from the (sequence, kv head) counter, and the last to arrive merges
// all splits (sc1 loads, 8 in flight) -- no combine launch, no fences (MI355X_MICROARCH.md
// hand-off rules); the last arriver re-zeroes the counter for the next launch.
// The launch fixes the number of splits (grid.x); blocks per split = max(a.blocks_per_split,
// ceil(blocks / grid.x)) is derived from each sequence's own ctx_len on the device, so a graph
// captured for the longest context spreads every shorter one over all its splits as well.
// (One-wave workgroups with one block each measured 2x slower: their single-wave split combine is
// latency-serial, profiles/r3_decode_attn_splits_v1.txt.)

// Prefetch workgroups (blockIdx.z >= B): stream a.pf[] once through the memory-side cache.
__device__ __forceinline__ void pd_prefetch(const DecodeArgs& a, int wg, int nwg) {
  uint32_t x = 0;
#pragma unroll 1
  for (int r = 0; r < 2; ++r) {
    if (a.pf[r] == nullptr || a.pf_bytes[r] <= 0) continue;
    const int64_t n16 = a.pf_bytes[r] >> 4;                     // whole 16-byte chunks
    const int64_t per = (n16 + nwg - 1) / nwg;
    const int64_t c0 = (int64_t)wg * per, c1 = min(n16, c0 + per);
    const u32x4_t* p = reinterpret_cast<const u32x4_t*>(a.pf[r]);
    int64_t c = c0 + threadIdx.x;
    for (; c + 7 * (int64_t)blockDim.x < c1; c += 8 * (int64_t)blockDim.x) {   // 8 loads in flight per lane
      u32x4_t v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = p[c + u * (int64_t)blockDim.x];
#pragma unroll
      for (int u = 0; u < 8; ++u) x ^= v[u][0] ^ v[u][3];
    }
    for (; c < c1; c += blockDim.x) x ^= p[c][0];
  }
  if (x == 0x9e3779b9u && a.pf_bytes[0] < 0) a.o[threadIdx.x] = 0;   // never true: keeps the loads
}

template <int D>
__device__ __forceinline__ void rope_chunks(u32x4_t (&w)[D / 32], const float2* cs, int g) {
  constexpr int KS = D / 32;
#pragma unroll
  for (int t = 0; t < KS / 2; ++t) {   // element e pairs with e + D/2: chunk t with t + KS/2
    float x1[8], x2[8];
    unpack8(w[t], x1);
    unpack8(w[t + KS / 2], x2);
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float2 c = cs[t * 32 + g * 8 + j];
      const float y1 = x1[j] * c.x - x2[j] * c.y, y2 = x2[j] * c.x + x1[j] * c.y;
      x1[j] = y1;
      x2[j] = y2;
    }
    w[t] = pack8(x1);
    w[t + KS / 2] = pack8(x2);
  }
}

// bf16 values as the cache stores them (fp8 cache: rounded through e4m3fn)
template <bool F8KV>
__device__ __forceinline__ __bf16 as_cached(__bf16 v) {
  if constexpr (F8KV) {
    const uint32_t b = f2fp8((float)v);
    return __builtin_bit_cast(bf16x8_t, fp8x8_to_bf16(b, 0u))[0];
  } else {
    return v;
  }
}

template <int D, bool F8KV>
__global__ void __launch_bounds__(64 * PA_NW) paged_decode_kernel(DecodeArgs a, int B) {
  constexpr int NW = PA_NW;
  if ((int)blockIdx.z >= B) {   // MALL prefetch workgroups
    pd_prefetch(a, ((blockIdx.z - B) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x,
                (gridDim.z - B) * gridDim.y * gridDim.x);
    return;
  }
  const int64_t t_start = a.dbg ? (int64_t)__builtin_amdgcn_s_memrealtime() : 0;
  constexpr int KS = D / 32;   // k-steps of S^T over the head dim
  constexpr int NB = D / 16;   // 16-wide d blocks of O^T
  __shared__ WaveMerge<D> sm;
  __shared__ int sm_last;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, g = lane >> 4;
  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int G = a.H / a.Hkv;
  const int ctx = a.ctx_len[b];
  const int nblk = (ctx + KV_BLOCK - 1) / KV_BLOCK;
  const int bps = max(a.blocks_per_split, (nblk + (int)gridDim.x - 1) / (int)gridDim.x);
  const int blk0 = split * bps;
  const int blk1 = min(blk0 + bps, nblk);
  const int ns = max(1, (nblk + bps - 1) / bps);   // splits holding blocks
  if (split >= ns) return;
  // this wave's blocks: blk0 + wid, + NW, ... (one block per wave up to 512 tokens per split)
  int phys = blk0 + wid < blk1 ? a.block_table[(int64_t)b * a.bt_stride + blk0 + wid] : 0;   // first load of the chain

  // Q^T fragment (B operand): column = query head hk*G + col (zero beyond G).  Loaded here, rotated
  // (fused RoPE) only after the first block's K / V loads are in flight: its VALU then overlaps
  // that round trip instead of delaying the issue.
  bf16x8_t qf[KS];
  const bool fused = a.pos != nullptr;
  const float2* cs = fused ? reinterpret_cast<const float2*>(a.cos_sin) + (int64_t)a.pos[b] * (D / 2) : nullptr;
  const bool qv = col < G;
  u32x4_t qraw[KS];
  {
    const uint16_t* qp = a.q + (int64_t)b * a.q_sb + (int64_t)(hk * G + (qv ? col : 0)) * D;
#pragma unroll
    for (int t = 0; t < KS; ++t) qraw[t] = *(const u32x4_t*)(qp + t * 32 + g * 8);
  }
  bool q_ready = false;
  auto prep_q = [&]() {
#pragma unroll
    for (int t = 0; t < KS; ++t)
      if (!qv) qraw[t] = (u32x4_t){0u, 0u, 0u, 0u};
    if constexpr (KS >= 2) {
      if (fused) rope_chunks<D>(qraw, cs, g);
    }
#pragma unroll
    for (int t = 0; t < KS; ++t) qf[t] = __builtin_bit_cast(bf16x8_t, qraw[t]);
    q_ready = true;
  };
  // current token (position ctx - 1) in fused mode: the wave owning its block takes it from
  // registers; the owning split's workgroup also writes it to the cache AFTER its attention
  // (fire-and-forget: only the next decode step reads it)
  const int cur = ctx - 1;
  const bool owns_cur = fused && blk0 <= cur / KV_BLOCK && cur / KV_BLOCK < blk1;
  // the current token's k (rotated) and v as this lane's fragments need them, loaded BEFORE the
  // K / V stream (vmcnt retires in issue order; a load issued after it would wait behind it)
  u32x4_t kcur[KS];
  uint16_t vcur[NB];
  if (owns_cur) {
    const uint16_t* kp = a.q + (int64_t)b * a.q_sb + (int64_t)(a.H + hk) * D;
    const uint16_t* vp = a.q + (int64_t)b * a.q_sb + (int64_t)(a.H + a.Hkv + hk) * D;
#pragma unroll
    for (int t = 0; t < KS; ++t) kcur[t] = *(const u32x4_t*)(kp + t * 32 + g * 8);
#pragma unroll
    for (int j = 0; j < NB; ++j) vcur[j] = vp[j * 16 + col];
  }

  f32x4_t o[NB];
#pragma unroll
  for (int j = 0; j < NB; ++j) o[j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  float mrow = -INFINITY, lrow = 0.f;

  for (int bi = blk0 + wid; bi < blk1; bi += NW) {
    if (bi != blk0 + wid) phys = a.block_table[(int64_t)b * a.bt_stride + bi];
    const int valid = min(KV_BLOCK, ctx - bi * KV_BLOCK);
    bf16x8_t kf[4][KS];
    bf16x8_t vf[2][NB];
    load_kv_block<D, F8KV>(a.k_cache, a.v_cache, ((int64_t)phys * a.Hkv + hk) * KV_BLOCK * D, col, g, kf, vf);
    // the current token's v from registers (its cache write comes after the loop)
    const bool cur_here = owns_cur && bi == cur / KV_BLOCK;
    const int coff = cur - bi * KV_BLOCK;
    if (cur_here) {
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        const int e = coff - 32 * s - 8 * g;   // lane-dependent: a select per element, no branch
#pragma unroll
        for (int j = 0; j < NB; ++j) {
          const __bf16 v = as_cached<F8KV>(__builtin_bit_cast(__bf16, vcur[j]));
#pragma unroll
          for (int ee = 0; ee < 8; ++ee) vf[s][j][ee] = ee == e ? v : vf[s][j][ee];
        }
      }
    }

    if (!q_ready) prep_q();
    f32x4_t sc[4];
    qk_scores(kf, qf, sc);
    if (cur_here) {   // the current token's score q . k_cur from registers (rotated, rounded as cached)
      u32x4_t kw[KS];
#pragma unroll
      for (int t = 0; t < KS; ++t) kw[t] = kcur[t];
      if constexpr (KS >= 2) rope_chunks<D>(kw, cs, g);
      float dot = 0.f;
#pragma unroll
      for (int t = 0; t < KS; ++t) {
        const bf16x8_t kv8 = __builtin_bit_cast(bf16x8_t, kw[t]);
#pragma unroll
        for (int e = 0; e < 8; ++e) dot += (float)as_cached<F8KV>(kv8[e]) * (float)qf[t][e];
      }
      dot += __shfl_xor(dot, 16, 64);   // sum over the 4 lane groups (d ranges) of query col
      dot += __shfl_xor(dot, 32, 64);
#pragma unroll
      for (int kb16 = 0; kb16 < 4; ++kb16)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (pa_token(kb16, g, r) == coff) sc[kb16][r] = dot;
    }
    softmax_step(sc, valid, a.scale_log2, g, mrow, lrow, o);
    zero_v_tail(vf, valid, g);   // after the softmax (K only): the V loads, issued last, stay in flight under it
    pv_step(sc, vf, o);
  }

  if (owns_cur) {   // the current token's k (rotated) / v into the cache for the next step
    const int64_t slot = a.slots[b];
    if (slot >= 0) {
      const int64_t cblk = slot >> 6;
      const int coff = (int)(slot & 63);
      const uint16_t* kv = a.q + (int64_t)b * a.q_sb + (int64_t)(a.H + hk) * D;   // unrotated k head
      const int half = D / 2;
      for (int i = tid; i < half + D; i += 64 * NW) {   // k rotation pairs, then v elements
      if (i < half) {
        const float2 c = reinterpret_cast<const float2*>(a.cos_sin)[(int64_t)a.pos[b] * half + i];
        const float x1 = bf2f(kv[i]), x2 = bf2f(kv[i + half]);
        const uint16_t y1 = f2bf(x1 * c.x - x2 * c.y), y2 = f2bf(x2 * c.x + x1 * c.y);
        const int64_t ko = ((cblk * a.Hkv + hk) * KV_BLOCK + coff) * D;
        if constexpr (F8KV) {
          uint8_t* kr = reinterpret_cast<uint8_t*>(a.k_cache_w) + ko;
          kr[i] = f2fp8(bf2f(y1));
          kr[i + half] = f2fp8(bf2f(y2));
        } else {
          a.k_cache_w[ko + i] = y1;
          a.k_cache_w[ko + i + half] = y2;
        }
      } else {
        const int d = i - half;
        const uint16_t* vr = a.q + (int64_t)b * a.q_sb + (int64_t)(a.H + a.Hkv + hk) * D;
        const int64_t vo = ((cblk * a.Hkv + hk) * D + d) * KV_BLOCK + coff;
        if constexpr (F8KV) reinterpret_cast<uint8_t*>(a.v_cache_w)[vo] = f2fp8(bf2f(vr[d]));
        else a.v_cache_w[vo] = vr[d];
      }
      }
    }
  }

  int64_t* dbg = a.dbg ? a.dbg + ((((int64_t)b * a.Hkv + hk) * gridDim.x + split) << 3) : nullptr;
  if (dbg && lane == 0) {   // per wave: when its block loop ended (stamp 1 + wave)
    dbg[1 + wid] = (int64_t)__builtin_amdgcn_s_memrealtime();
    if (wid == 0) dbg[0] = t_start;
  }
  // ---- merge the NW wave states through LDS
  sm.store(wid, col, g, mrow, lrow, o);
  __syncthreads();
  for (int idx = tid; idx < G * D; idx += 64 * NW) {
    const int q = idx / D, d = idx - q * D;
    float M, L, O;
    sm.reduce(q, d, M, L, O);
    const int h = hk * G + q;
    if (ns == 1) {
      a.o[(int64_t)b * a.o_sb + (int64_t)h * D + d] = f2bf(L > 0.f ? O / L : 0.f);
    } else {
      const int64_t pi = ((int64_t)b * a.H + h) * a.nsplit + split;
      publish_split<D>(a.part_o, a.part_ml, pi, d, M, L, O);
    }
  }
  if (ns == 1) {
    if (dbg && tid == 0) dbg[5] = (int64_t)__builtin_amdgcn_s_memrealtime();
    return;
  }

  // ---- in-launch combine: the last split of (b, hk) to arrive merges all ns splits
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (dbg && tid == 0) dbg[5] = (int64_t)__builtin_amdgcn_s_memrealtime();   // partials published
  if (tid == 0) sm_last = split_ticket(a.split_cnt + (int64_t)b * a.Hkv + hk, ns) ? 1 : 0;
  __syncthreads();
  if (dbg && tid == 0) dbg[6] = (int64_t)__builtin_amdgcn_s_memrealtime();   // ticket back
  if (!sm_last) return;
  for (int idx = tid; idx < G * D; idx += 64 * NW) {
    const int q = idx / D, d = idx - q * D;
    const int h = hk * G + q;
    const int64_t pi0 = ((int64_t)b * a.H + h) * a.nsplit;
    a.o[(int64_t)b * a.o_sb + (int64_t)h * D + d] = f2bf(merge_splits<D>(a.part_o, a.part_ml, pi0, ns, d));
  }
  if (dbg && tid == 0) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    dbg[7] = (int64_t)__builtin_amdgcn_s_memrealtime();   // combine done (last split only)
  }
}

hipError_t paged_decode(const DecodeArgs& a, int B, int D, hipStream_t stream) {
  if (a.nsplit > 32 || (a.nsplit > 1 && a.split_cnt == nullptr)) return hipErrorInvalidValue;
  // prefetch slices: enough z-slices of (nsplit x Hkv) workgroups for >= 192 prefetching CUs
  const bool pf = (a.pf[0] != nullptr && a.pf_bytes[0] > 0) || (a.pf[1] != nullptr && a.pf_bytes[1] > 0);
  const int per_z = a.nsplit * a.Hkv;
  const int pfz = pf ? (192 + per_z - 1) / per_z : 0;
  dim3 grid(a.nsplit, a.Hkv, B + pfz), block(64 * PA_NW);
  const bool ok = pa_dispatch(D, a.kv_fp8, [&](auto d, auto f8) {
    hipLaunchKernelGGL((paged_decode_kernel<decltype(d)::value, decltype(f8)::value>), grid, block, 0, stream, a, B);
  });
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

// ------------------------------------------------------------------------------ paged prefill attention
// Queries are T new rows of one sequence at positions start_pos.., keys / values are the paged
// pools read through the sequence's block list (the chunk's own k / v were written by rope_kv
// before this launch): chunked prefill and prefix reuse without a contiguous copy of the prefix.
// The block step is paged_decode's (paged_attn.h), but the 16 MFMA columns are (query row, head in
// group) pairs: column c of a workgroup <-> row c / G, head hk * G + c % G, so a G that does not
// divide 16 wastes at most G - 1 columns per workgroup.  One workgroup of 4 waves per (tile of
// 64 / G query rows, kv head); every wave carries all PP_NCT = 4 column tiles and walks blocks
// wid, wid + 4, ... up to the tile's last position, so each block's K / V fragments are loaded
// once per workgroup and reused by 64 columns; the 4 wave states merge through LDS, one column
// tile at a time.  Causal: column at position p sees tokens <= p.
constexpr int PP_NCT = 4;

template <int D, bool F8KV>
__global__ void __launch_bounds__(64 * PA_NW) paged_prefill_kernel(PrefillArgs a) {
  constexpr int NW = PA_NW, NCT = PP_NCT;
  constexpr int KS = D / 32;   // k-steps of S^T over the head dim
  constexpr int NB = D / 16;   // 16-wide d blocks of O^T
  __shared__ WaveMerge<D> sm;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, g = lane >> 4;
  const int hk = blockIdx.y;
  const int G = a.H / a.Hkv;
  const int QT = (16 * NCT) / G;                       // query rows per workgroup
  const int row0 = blockIdx.x * QT;
  const int rows = min(QT, a.T - row0);
  const int S = a.start_pos + a.T;                     // tokens of the sequence in the cache
  const int nblk = (a.start_pos + row0 + rows - 1) / KV_BLOCK + 1;   // blocks up to the tile's last position

  int64_t phys = wid < nblk ? a.blocks[wid] : 0;       // first load of the chain

  // Q^T fragments (B operand) of the NCT column tiles; lim = tokens the column may see (0: unused column)
  bf16x8_t qf[NCT][KS];
  int lim[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    const int c = ct * 16 + col;
    const int rl = c / G, hg = c - rl * G;
    const bool ok = rl < rows;
    lim[ct] = ok ? a.start_pos + row0 + rl + 1 : 0;
    const uint16_t* qp = a.q + (int64_t)(row0 + (ok ? rl : 0)) * a.q_ld + (int64_t)(hk * G + hg) * D;
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      u32x4_t w = *(const u32x4_t*)(qp + t * 32 + g * 8);
      if (!ok) w = (u32x4_t){0u, 0u, 0u, 0u};
      qf[ct][t] = __builtin_bit_cast(bf16x8_t, w);
    }
  }

  f32x4_t o[NCT][NB];
  float mrow[NCT], lrow[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    mrow[ct] = -INFINITY;
    lrow[ct] = 0.f;
#pragma unroll
    for (int j = 0; j < NB; ++j) o[ct][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }

  for (int bi = wid; bi < nblk; bi += NW) {
    if (bi != wid) phys = a.blocks[bi];
    phys = min(max(phys, (int64_t)0), (int64_t)a.num_blocks - 1);   // a bad list entry must not leave the pool
    const int tok0 = bi * KV_BLOCK;
    bf16x8_t kf[4][KS];
    bf16x8_t vf[2][NB];
    load_kv_block<D, F8KV>(a.k_cache, a.v_cache, (phys * a.Hkv + hk) * KV_BLOCK * D, col, g, kf, vf);
    zero_v_tail(vf, min(KV_BLOCK, S - tok0), g);
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      f32x4_t sc[4];
      qk_scores(kf, qf[ct], sc);
      // the column sees lim[ct] - tok0 tokens of this block
      softmax_step(sc, lim[ct] - tok0, a.scale_log2, g, mrow[ct], lrow[ct], o[ct]);
      pv_step(sc, vf, o[ct]);
    }
  }

  // ---- merge the NW wave states through LDS, one column tile at a time
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    if (ct > 0) __syncthreads();
    sm.store(wid, col, g, mrow[ct], lrow[ct], o[ct]);
    __syncthreads();
    for (int idx = tid; idx < 16 * D; idx += 64 * NW) {
      const int qc = idx / D, d = idx - qc * D;
      const int c = ct * 16 + qc;
      const int rl = c / G, hg = c - rl * G;
      if (rl >= rows) continue;
      float M, L, O;
      sm.reduce(qc, d, M, L, O);
      a.o[(int64_t)(row0 + rl) * a.o_ld + (int64_t)(hk * G + hg) * D + d] = f2bf(L > 0.f ? O / L : 0.f);
    }
  }
}

hipError_t paged_prefill(const PrefillArgs& a, int D, hipStream_t stream) {
  if (a.T <= 0) return hipSuccess;
  if (a.Hkv <= 0 || a.H % a.Hkv != 0 || a.H / a.Hkv > 16 || a.num_blocks <= 0 || a.start_pos < 0) return hipErrorInvalidValue;
  const int QT = (16 * PP_NCT) / (a.H / a.Hkv);
  dim3 grid((a.T + QT - 1) / QT, a.Hkv), block(64 * PA_NW);
  const bool ok = pa_dispatch(D, a.kv_fp8, [&](auto d, auto f8) {
    hipLaunchKernelGGL((paged_prefill_kernel<decltype(d)::value, decltype(f8)::value>), grid, block, 0, stream, a);
  });
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

// ------------------------------------------------------------------------------ paged verify attention
// Up to T new query rows for each of B sequences in one launch (speculative decoding: the last
// accepted token plus its draft tokens).  Prefill's column mapping on decode's grid: one workgroup
// of 4 waves per (split, kv head, sequence) with decode's split policy (blocks per split derived
// from each sequence's ctx_len on the device) and its in-launch combine; MFMA column c <-> row
// c / G, head hk * G + c % G over NCT = 1, 2 or 4 column tiles (T * G <= 64), so a block's K / V
// fragments are loaded once per workgroup and reused by every row.  Row i of sequence b sits at
// position ctx_len[b] - n_rows[b] + i and sees tokens 0 .. that position; rows >= n_rows[b] see
// nothing and come out 0.  Everything that changes from step to step (block table, ctx_len,
// n_rows) is read from device memory: one captured graph replays for any step.  The rows' own
// k / v are in the cache already (rope_kv runs first).
template <int D, bool F8KV, int NCT>
__global__ void __launch_bounds__(64 * PA_NW) paged_verify_kernel(VerifyArgs a) {
  constexpr int NW = PA_NW;
  constexpr int KS = D / 32;   // k-steps of S^T over the head dim
  constexpr int NB = D / 16;   // 16-wide d blocks of O^T
  __shared__ WaveMerge<D> sm;
  __shared__ int sm_last;

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int col = lane & 15, g = lane >> 4;
  const int split = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
  const int G = a.H / a.Hkv;
  const int ctx = min(max(a.ctx_len[b], 0), a.bt_width * KV_BLOCK);   // never past the table row
  const int n = min(max(a.n_rows[b], 0), a.T);
  const int nblk = (ctx + KV_BLOCK - 1) / KV_BLOCK;
  const int bps = max(a.blocks_per_split, (nblk + (int)gridDim.x - 1) / (int)gridDim.x);
  const int blk0 = split * bps;
  const int blk1 = min(blk0 + bps, nblk);
  const int ns = max(1, (nblk + bps - 1) / bps);   // splits holding blocks
  if (split >= ns) return;
  const int* bt = a.block_table + (int64_t)b * a.bt_stride;
  int phys = blk0 + wid < blk1 ? bt[blk0 + wid] : 0;   // first load of the chain

  // Q^T fragments (B operand) of the column tiles; lim = tokens the column may see (0: padding)
  bf16x8_t qf[NCT][KS];
  int lim[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    const int c = ct * 16 + col;
    const int rl = c / G, hg = c - rl * G;
    const bool ok = rl < n;
    lim[ct] = ok ? ctx - n + rl + 1 : 0;
    const uint16_t* qp = a.q + ((int64_t)b * a.T + (ok ? rl : 0)) * a.q_ld + (int64_t)(hk * G + hg) * D;
#pragma unroll
    for (int t = 0; t < KS; ++t) {
      u32x4_t w = *(const u32x4_t*)(qp + t * 32 + g * 8);
      if (!ok) w = (u32x4_t){0u, 0u, 0u, 0u};
      qf[ct][t] = __builtin_bit_cast(bf16x8_t, w);
    }
  }

  f32x4_t o[NCT][NB];
  float mrow[NCT], lrow[NCT];
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    mrow[ct] = -INFINITY;
    lrow[ct] = 0.f;
#pragma unroll
    for (int j = 0; j < NB; ++j) o[ct][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  }

  for (int bi = blk0 + wid; bi < blk1; bi += NW) {
    if (bi != blk0 + wid) phys = bt[bi];
    phys = min(max(phys, 0), a.num_blocks - 1);   // a bad table entry must not leave the pool
    const int tok0 = bi * KV_BLOCK;
    bf16x8_t kf[4][KS];
    bf16x8_t vf[2][NB];
    load_kv_block<D, F8KV>(a.k_cache, a.v_cache, ((int64_t)phys * a.Hkv + hk) * KV_BLOCK * D, col, g, kf, vf);
    zero_v_tail(vf, min(KV_BLOCK, ctx - tok0), g);
#pragma unroll
    for (int ct = 0; ct < NCT; ++ct) {
      if (ct * 16 >= n * G) continue;   // a tile of padding columns only (workgroup-uniform)
      f32x4_t sc[4];
      qk_scores(kf, qf[ct], sc);
      softmax_step(sc, lim[ct] - tok0, a.scale_log2, g, mrow[ct], lrow[ct], o[ct]);
      pv_step(sc, vf, o[ct]);
    }
  }

  // ---- merge the NW wave states through LDS, one column tile at a time
#pragma unroll
  for (int ct = 0; ct < NCT; ++ct) {
    if (ct > 0) __syncthreads();
    sm.store(wid, col, g, mrow[ct], lrow[ct], o[ct]);
    __syncthreads();
    for (int idx = tid; idx < 16 * D; idx += 64 * NW) {
      const int qc = idx / D, d = idx - qc * D;
      const int c = ct * 16 + qc;
      const int rl = c / G, hg = c - rl * G;
      if (rl >= a.T) continue;
      float M, L, O;
      sm.reduce(qc, d, M, L, O);
      const int64_t row = (int64_t)b * a.T + rl;
      const int h = hk * G + hg;
      if (ns == 1) a.o[row * a.o_ld + (int64_t)h * D + d] = f2bf(L > 0.f ? O / L : 0.f);
      else publish_split<D>(a.part_o, a.part_ml, (row * a.H + h) * a.nsplit + split, d, M, L, O);
    }
  }
  if (ns == 1) return;

  // ---- in-launch combine: the last split of (b, hk) to arrive merges all ns splits
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) sm_last = split_ticket(a.split_cnt + (int64_t)b * a.Hkv + hk, ns) ? 1 : 0;
  __syncthreads();
  if (!sm_last) return;
  for (int idx = tid; idx < a.T * G * D; idx += 64 * NW) {
    const int c = idx / D, d = idx - c * D;
    const int rl = c / G, hg = c - rl * G;
    const int64_t row = (int64_t)b * a.T + rl;
    const int h = hk * G + hg;
    a.o[row * a.o_ld + (int64_t)h * D + d] = f2bf(merge_splits<D>(a.part_o, a.part_ml, (row * a.H + h) * a.nsplit, ns, d));
  }
}

hipError_t paged_verify(const VerifyArgs& a, int B, int D, hipStream_t stream) {
  if (B <= 0) return hipSuccess;
  if (a.T < 1 || a.Hkv <= 0 || a.H % a.Hkv != 0 || a.H / a.Hkv > 16 || a.T * (a.H / a.Hkv) > 64 || a.num_blocks <= 0 ||
      a.bt_width <= 0 || a.nsplit < 1 || a.nsplit > 32 || a.blocks_per_split < 1 ||
      (a.nsplit > 1 && (a.split_cnt == nullptr || a.part_o == nullptr || a.part_ml == nullptr)))
    return hipErrorInvalidValue;
  const int cols = a.T * (a.H / a.Hkv);
  dim3 grid(a.nsplit, a.Hkv, B), block(64 * PA_NW);
  const bool ok = pa_dispatch(D, a.kv_fp8, [&](auto d, auto f8) {
    constexpr int Dc = decltype(d)::value;
    constexpr bool F8 = decltype(f8)::value;
    if (cols <= 16) hipLaunchKernelGGL((paged_verify_kernel<Dc, F8, 1>), grid, block, 0, stream, a);
    else if (cols <= 32) hipLaunchKernelGGL((paged_verify_kernel<Dc, F8, 2>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((paged_verify_kernel<Dc, F8, 4>), grid, block, 0, stream, a);
  });
  return ok ? hipGetLastError() : hipErrorInvalidValue;
}

// ------------------------------------------------------------------------------ repetition penalty
__global__ void rep_penalty_kernel(float* logits, int64_t ld, const int* ids, int maxn, const float* penalty, int V) {
  const int b = blockIdx.x;
  const float p = penalty[b];
  for (int j = threadIdx.x; j < maxn; j += blockDim.x) {
    const int id = ids[(int64_t)b * maxn + j];
    if (id < 0 || id >= V) continue;
    float* l = logits + (int64_t)b * ld + id;
    const float v = *l;
    *l = v > 0.f ? v / p : v * p;
  }
}

hipError_t rep_penalty(float* logits, int64_t ld, const int* ids, int maxn, const float* penalty, int B, int V,
                       hipStream_t stream) {
  if (B == 0 || maxn == 0) return hipSuccess;
  hipLaunchKernelGGL(rep_penalty_kernel, dim3(B), dim3(256), 0, stream, logits, ld, ids, maxn, penalty, V);
  return hipGetLastError();
}

// Small integer arrays (token ids, cache slots) uploaded through the kernel arguments: no copy
// engine / blit path, so behind a queue of kernels (a request's prefill inputs behind its image
// tower) the values land one tiny kernel after the queue drains instead of 20-70 us later per
// hipMemcpyAsync (profiles/r5_ttft_*).
__global__ void upload_i64_kernel(UploadArgs a, int64_t* __restrict__ out, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = a.v[i];
}

hipError_t upload_i64(const UploadArgs& a, int64_t* out, int n, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  hipLaunchKernelGGL(upload_i64_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, a, out, n);
  return hipGetLastError();
}

}  // namespace lumen
