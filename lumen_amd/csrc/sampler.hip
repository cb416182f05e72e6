// Vocab sampler for the decode graph: what the host path does per step with
// rep_penalty_ + logits.mul_ + row_topk(64) + a D2H + numpy (ops/llm.py sample_from_candidates),
// as one or two launches that read the [B, V] fp32 logits once and never write them.
//
// Per row: x -> (seen token ? (x > 0 ? x / penalty : x * penalty) : x) * inv_t in the same fp32
// operations as the host path, so the 64 candidates match it bit for bit; the scan, the online
// (max, sum-exp) and the merge are row_topk's (topk_core.h), in the same one- or two-phase
// split.  "Seen" is a bit per token in the row's bitmap slot (staged in LDS per chunk) or the
// step's input token.  The workgroup that holds the final 64 candidates (lane j of wave 0 =
// candidate j) then draws: p_j = exp(v_j - lse), its running sum, the nucleus length n and the
// pick are fp64, in numpy's order of operations (cumsum is a sequential sum), so the same
// candidates and uniform choose the same token as numpy's Generator.choice:
//   thr = c_63 < top_p ? top_p * c_63 : top_p;  n = #{c_j < thr} + 1
//   j*  = min(n - 1, #{j < n : c_j / c_{n-1} <= u})
// Last, the step's INPUT token is marked in the bitmap -- after every read of the row's bitmap:
// the staging of the single launch, or the whole first launch of the two-phase form -- so a
// look-ahead step that is later discarded has only marked a token that really was emitted.
//
// A greedy row needs its best candidate only: unless the caller asked for the candidates, its
// workgroups run one merge round instead of 64 (the rounds, two barriers each, are most of the
// sampler's time on a vocabulary-sized row).
#include "sampler.h"

#include "topk_core.h"

namespace lumen {

int topk_chunks(int N);   // topk.hip: the sampler splits rows exactly as row_topk does

constexpr int SAMPLE_STAGE_WORDS = 512;   // bitmap words of the widest single-launch row (16384 columns)

struct SeenXf {
  const int* bits;   // LDS: word 0 holds columns j0 .. j0 + 31 (j0 is a multiple of 32)
  int j0, in_id;
  float pen, inv_t;
  bool on;
  __device__ __forceinline__ float operator()(float x, const int j) const {
    if (on) {
      const int r = j - j0;
      if (((bits[r >> 5] >> (r & 31)) & 1) || j == in_id) x = x > 0.f ? x / pen : x * pen;
    }
    return x * inv_t;
  }
};

// winner r stays in lane r of wave 0 (k = 64 = one wave); thread 0 also writes the optional outputs
struct LaneSink {
  float v;
  int i;
  float* out_v;
  int* out_i;
  int64_t obase;
  __device__ __forceinline__ void operator()(const int r, const float fv, const int fi) {
    if ((int)threadIdx.x == r) { v = fv; i = fi; }
    if (threadIdx.x == 0 && out_v) { out_v[obase + r] = fv; out_i[obase + r] = fi; }
  }
};

enum : int { SAMPLE_PARTIAL = 0, SAMPLE_SINGLE = 1, SAMPLE_MERGE = 2 };

// PARTIAL: grid (B, chunks), transformed candidates + (max, sum-exp) of one chunk -> workspace.
// SINGLE:  grid (B, 1), the whole row in one workgroup, then the draw.
// MERGE:   grid (B, 1), the chunks' candidates and statistics merged, then the draw.
template <int MODE>
__global__ void __launch_bounds__(256)
sample_rows_kernel(const SampleArgs a, float* __restrict__ cv, int* __restrict__ ci, float* __restrict__ pml,
                   int nch) {
  __shared__ int bits[SAMPLE_STAGE_WORDS];
  const int row = blockIdx.x;
  const int slot_in = a.seen_slot[row];
  const int slot = slot_in < a.S ? slot_in : -1;
  const int64_t in64 = a.in_ids[row];
  const int in_id = in64 >= 0 && in64 < a.V ? (int)in64 : -1;
  const int k = a.greedy[row] && !a.out_v ? 1 : SAMPLE_K;
  float lse0;
  LaneSink lanes{-INFINITY, -1, a.out_v, a.out_i, (int64_t)row * SAMPLE_K};
  if constexpr (MODE == SAMPLE_MERGE) {
    lse0 = topk_block<SAMPLE_K>(cv, (int64_t)nch * SAMPLE_K, nch * SAMPLE_K, k, 1.f, a.out_lse, ci, pml, nch,
                                nch * SAMPLE_K, nullptr, true, TopkIdentity{}, lanes);
  } else {
    const int chunk = MODE == SAMPLE_PARTIAL ? TOPK_CHUNK : a.V;
    const int j0 = blockIdx.y * chunk, j1 = min(a.V, j0 + chunk);
    SeenXf xf{bits, j0, in_id, a.penalty[row], a.inv_t[row], false};
    xf.on = slot >= 0 && xf.pen != 1.f;
    if (xf.on) {
      const int* srow = a.seen + (int64_t)slot * a.words + (j0 >> 5);
      const int nw = min((j1 - j0 + 31) >> 5, SAMPLE_STAGE_WORDS);
      for (int t = threadIdx.x; t < nw; t += 256) bits[t] = srow[t];
      __syncthreads();
    }
    if constexpr (MODE == SAMPLE_PARTIAL) {
      TopkStore store{cv, ci, ((int64_t)row * gridDim.y + blockIdx.y) * SAMPLE_K, 0};
      topk_block<SAMPLE_K>(a.logits, a.ld, a.V, k, 1.f, nullptr, nullptr, nullptr, 1, chunk, pml, false, xf, store);
      for (int t = k + threadIdx.x; t < SAMPLE_K; t += 256) {   // the merge reads 64 per chunk
        cv[store.obase + t] = -INFINITY;
        ci[store.obase + t] = -1;
      }
      return;
    } else {
      lse0 = topk_block<SAMPLE_K>(a.logits, a.ld, a.V, k, 1.f, a.out_lse, nullptr, nullptr, 1, chunk, nullptr,
                                  true, xf, lanes);
    }
  }
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  const float lse = __shfl(lse0, 0, 64);
  const double p = exp((double)lanes.v - (double)lse);
  double c = 0.0;   // c_lane = ((p_0 + p_1) + p_2) + ... : numpy's cumsum
  for (int i = 0; i < SAMPLE_K; ++i) {
    const double pi = __shfl(p, i, 64);
    if (i <= lane) c += pi;
  }
  const double top_p = a.top_p[row], ctot = __shfl(c, SAMPLE_K - 1, 64);
  const double thr = ctot < top_p ? top_p * ctot : top_p;
  const int n = min(max(__popcll(__ballot(c < thr)) + 1, 1), SAMPLE_K);
  const double cn = __shfl(c, n - 1, 64);
  int js = min(__popcll(__ballot(lane < n && c / cn <= a.u[row])), n - 1);
  if (a.greedy[row]) js = 0;
  const int t = __shfl(lanes.i, js, 64);
  if (lane == 0) {
    a.tok[row] = t;
    a.out_ids[row] = t < 0 ? 0 : t;      // a row without a finite logit must not index the embedding with -1
    if (slot >= 0 && in_id >= 0) {       // a slot belongs to one row: plain read-modify-write
      int* w = a.seen + (int64_t)slot * a.words + (in_id >> 5);
      *w = *w | (int)(1u << (in_id & 31));
    }
  }
}

int64_t sample_ws_floats(int B, int V) {
  const int nch = topk_chunks(V);
  return nch > 1 ? (int64_t)B * nch * (2 * SAMPLE_K + 2) : 0;
}

hipError_t sample_rows(const SampleArgs& a, float* ws, hipStream_t stream) {
  if (a.B == 0) return hipSuccess;
  if (a.V < SAMPLE_K || a.words != (a.V + 31) / 32) return hipErrorInvalidValue;
  const int nch = topk_chunks(a.V);
  if (nch == 1) {
    if (a.words > SAMPLE_STAGE_WORDS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_rows_kernel<SAMPLE_SINGLE>, dim3(a.B, 1), dim3(256), 0, stream, a, nullptr, nullptr,
                       nullptr, 1);
    return hipGetLastError();
  }
  if (ws == nullptr) return hipErrorInvalidValue;
  float* cv = ws;
  int* ci = reinterpret_cast<int*>(ws + (int64_t)a.B * nch * SAMPLE_K);
  float* pml = ws + (int64_t)a.B * nch * SAMPLE_K * 2;
  hipLaunchKernelGGL(sample_rows_kernel<SAMPLE_PARTIAL>, dim3(a.B, nch), dim3(256), 0, stream, a, cv, ci, pml, nch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(sample_rows_kernel<SAMPLE_MERGE>, dim3(a.B, 1), dim3(256), 0, stream, a, cv, ci, pml, nch);
  return hipGetLastError();
}

}  // namespace lumen
