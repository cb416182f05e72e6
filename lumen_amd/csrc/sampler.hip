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
//
// Verify form (SampleArgs.T > 0, speculative decoding): R = B * T rows, sequence-major; row (b, i)
// holds the logits after sequence b's input i (its last token, then its draft tokens) and is live
// while i < n_rows[b] (a dead row only writes tok = -1).  The per-sequence arguments are read at
// b, the uniform and the input token at the row.  The penalty set of row (b, i) is b's bitmap slot
// and inputs 0 .. i of b: those are OR-ed into the LDS copy of the bitmap chunk before the scan, so
// the per-element test stays the one bit test, and the floating-point operations and the order of
// the candidates are the decode form's.  A verify row marks nothing: verify_accept, one launch
// behind the draw, finds per sequence the number of draft tokens that equal the token drawn for the
// row before them and marks the inputs up to the last accepted one -- a rejected draft token never
// reaches the bitmap.
//
// Guided form (template flag GUIDED; the other instantiations are compiled as before): a row with a grammar state s >= 0 stages row s of the arena of allowed-token bitmaps
// into a second LDS array, chunked like the seen bitmap, and a logit whose bit is clear becomes
// -inf before the penalty and the 1/T: it is never a candidate and adds nothing to the
// log-sum-exp, so the allowed set is renormalised.  After the draw lane 0 walks the drawn token's
// bytes through the byte DFA from s and stores the new state, which the look-ahead step reads.
//
// Verify form, guided (VERIFY and GUIDED): the guide is per row.  g_in has B * T entries, entry
// b * T + i the arena-global state in which row (b, i) draws -- the state after sequence b's text and
// its draft tokens 1 .. i, which the host computes -- or -1 for an unguided row; a state outside the
// arena allows nothing (tok = -1).  The row's allow row is staged like the decode form's and GuideXf
// wraps the SeenXf whose bitmap has the inputs 0 .. i OR-ed in.  This form reads and writes neither
// g_slot nor g_state and walks no DFA: every step around a verify step is fed by the host, so
// nothing would read a stored state, and verify_accept is the unguided form's.
#include "sampler.h"

#include <type_traits>

#include "topk_core.h"

namespace lumen {

int topk_chunks(int N);   // topk.hip: the sampler splits rows exactly as row_topk does

constexpr int SAMPLE_STAGE_WORDS = 512;   // bitmap words of the widest single-launch row (16384 columns)

struct SeenXf {
  static constexpr bool kSkipNegInf = false;
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

// the guided form: a column whose bit in the state's allow row is clear is -inf, then SeenXf
struct GuideXf {
  static constexpr bool kSkipNegInf = true;
  SeenXf seen;
  const int* allow;   // LDS: word 0 holds columns j0 .. j0 + 31
  int mode;           // 0: unguided row, 1: test the bit, 2: nothing is allowed
  __device__ __forceinline__ float operator()(float x, const int j) const {
    if (mode) {
      const int r = j - seen.j0;
      if (mode == 2 || !((allow[r >> 5] >> (r & 31)) & 1)) return -INFINITY;
    }
    return seen(x, j);
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
// VERIFY: row = (sequence seq, input vi) of the verify form; else seq = row.
template <int MODE, bool VERIFY, bool GUIDED = false>
__global__ void __launch_bounds__(256)
sample_rows_kernel(const SampleArgs a, float* __restrict__ cv, int* __restrict__ ci, float* __restrict__ pml,
                   int nch) {
  __shared__ int bits[SAMPLE_STAGE_WORDS];
  __shared__ int allow[GUIDED ? SAMPLE_STAGE_WORDS : 1];   // 2 KB more in the guided form; unused (and dropped) otherwise
  const int row = blockIdx.x;
  const int seq = VERIFY ? row / a.T : row, vi = VERIFY ? row % a.T : 0;
  if constexpr (VERIFY) {
    if (vi >= a.n_rows[seq]) {   // a dead row: the whole workgroup leaves (the merge never reads its partials)
      if (MODE != SAMPLE_PARTIAL && threadIdx.x == 0) a.tok[row] = -1;
      return;
    }
  }
  const int slot_in = a.seen_slot[seq];
  const int slot = slot_in < a.S ? slot_in : -1;
  const int64_t in64 = a.in_ids[row];
  // verify: the inputs up to the row's own are bits of the staged bitmap, not a compare per element
  const int in_id = !VERIFY && in64 >= 0 && in64 < a.V ? (int)in64 : -1;
  const int k = a.greedy[seq] && !a.out_v ? 1 : SAMPLE_K;
  // guided: the row's slot of g_state and its grammar state (-1: unguided row; a state outside the
  // arena allows nothing).  Every thread reads the state before the first barrier, lane 0 stores the
  // new one after the last.  The verify form takes the row's state from the host and keeps none.
  int gslot = -1, gs = -1;
  if constexpr (GUIDED && VERIFY) {
    gs = a.g_in[row];
    if (gs < 0) gs = -1;
    else if (gs >= a.g_A) gs = a.g_A;
  } else if constexpr (GUIDED) {
    gslot = a.g_slot[row];
    if (gslot >= a.g_S) gslot = -1;
    if (gslot >= 0) {
      const int fed = a.g_in[row];
      gs = fed >= 0 ? fed : a.g_state[gslot];
      if (gs < 0 || gs >= a.g_A) gs = a.g_A;   // no such state: nothing is allowed, tok = -1
    }
  }
  float lse0;
  LaneSink lanes{-INFINITY, -1, a.out_v, a.out_i, (int64_t)row * SAMPLE_K};
  if constexpr (MODE == SAMPLE_MERGE) {
    lse0 = topk_block<SAMPLE_K>(cv, (int64_t)nch * SAMPLE_K, nch * SAMPLE_K, k, 1.f, a.out_lse, ci, pml, nch,
                                nch * SAMPLE_K, nullptr, true, TopkIdentity{}, lanes);
  } else {
    const int chunk = MODE == SAMPLE_PARTIAL ? TOPK_CHUNK : a.V;
    const int j0 = blockIdx.y * chunk, j1 = min(a.V, j0 + chunk);
    SeenXf xf{bits, j0, in_id, a.penalty[seq], a.inv_t[seq], false};
    xf.on = slot >= 0 && xf.pen != 1.f;
    if (xf.on) {
      const int* srow = a.seen + (int64_t)slot * a.words + (j0 >> 5);
      const int nw = min((j1 - j0 + 31) >> 5, SAMPLE_STAGE_WORDS);
      for (int t = threadIdx.x; t < nw; t += 256) bits[t] = srow[t];
      __syncthreads();
      if constexpr (VERIFY) {
        if (threadIdx.x == 0) {   // at most T ids, two of which may share a word: one thread, in turn
          for (int q = 0; q <= vi; ++q) {
            const int64_t id = a.in_ids[row - vi + q];
            if (id >= j0 && id < j1) {
              const int r = (int)id - j0;
              if ((r >> 5) < nw) bits[r >> 5] |= (int)(1u << (r & 31));
            }
          }
        }
        __syncthreads();
      }
    }
    std::conditional_t<GUIDED, GuideXf, SeenXf> xg;
    if constexpr (GUIDED) {
      xg = GuideXf{xf, allow, gs < 0 ? 0 : gs < a.g_A ? 1 : 2};
      if (xg.mode == 1) {   // uniform over the workgroup: one row, one state
        const int* arow = a.g_allow + (int64_t)gs * a.words + (j0 >> 5);
        const int nw = min((j1 - j0 + 31) >> 5, SAMPLE_STAGE_WORDS);
        for (int t = threadIdx.x; t < nw; t += 256) allow[t] = arow[t];
        __syncthreads();
      }
    } else {
      xg = xf;
    }
    if constexpr (MODE == SAMPLE_PARTIAL) {
      TopkStore store{cv, ci, ((int64_t)row * gridDim.y + blockIdx.y) * SAMPLE_K, 0};
      topk_block<SAMPLE_K>(a.logits, a.ld, a.V, k, 1.f, nullptr, nullptr, nullptr, 1, chunk, pml, false, xg, store);
      for (int t = k + threadIdx.x; t < SAMPLE_K; t += 256) {   // the merge reads 64 per chunk
        cv[store.obase + t] = -INFINITY;
        ci[store.obase + t] = -1;
      }
      return;
    } else {
      lse0 = topk_block<SAMPLE_K>(a.logits, a.ld, a.V, k, 1.f, a.out_lse, nullptr, nullptr, 1, chunk, nullptr,
                                  true, xg, lanes);
    }
  }
  if (threadIdx.x >= 64) return;
  const int lane = threadIdx.x;
  const float lse = __shfl(lse0, 0, 64);
  // Fewer than 64 finite candidates (a guided row that allows m < 64 tokens): lanes m .. 63 hold
  // v = -inf, so p = exp(-inf - lse) = 0 and c_j = c_{m-1} = ctot for every j >= m.  thr <= ctot in
  // both branches below, so no c_j of the tail is < thr, nor is c_{m-1}: n <= m, and the pick
  // js <= n - 1 is a finite candidate.  The -inf tail has probability 0 and is never picked.
  // m = 0 (nothing allowed, lse = -inf): p is NaN, every comparison is false, n = 1, js = 0 and
  // lane 0 holds id -1: tok = -1, as for a row without a finite logit.
  const double p = exp((double)lanes.v - (double)lse);
  double c = 0.0;   // c_lane = ((p_0 + p_1) + p_2) + ... : numpy's cumsum
  for (int i = 0; i < SAMPLE_K; ++i) {
    const double pi = __shfl(p, i, 64);
    if (i <= lane) c += pi;
  }
  const double top_p = a.top_p[seq], ctot = __shfl(c, SAMPLE_K - 1, 64);
  const double thr = ctot < top_p ? top_p * ctot : top_p;
  const int n = min(max(__popcll(__ballot(c < thr)) + 1, 1), SAMPLE_K);
  const double cn = __shfl(c, n - 1, 64);
  int js = min(__popcll(__ballot(lane < n && c / cn <= a.u[row])), n - 1);
  if (a.greedy[seq]) js = 0;
  const int t = __shfl(lanes.i, js, 64);
  if (lane == 0) {
    a.tok[row] = t;
    if constexpr (!VERIFY) {
      a.out_ids[row] = t < 0 ? 0 : t;    // a row without a finite logit must not index the embedding with -1
      if (slot >= 0 && in_id >= 0) {     // a slot belongs to one row: plain read-modify-write
        int* w = a.seen + (int64_t)slot * a.words + (in_id >> 5);
        *w = *w | (int)(1u << (in_id & 31));
      }
    }
    if constexpr (GUIDED && !VERIFY) {
      // the slot belongs to this sequence: plain loads and a plain store.  An EOS or zero-length
      // token has no bytes and leaves the state; so does tok = -1.  The drawn token's bit was set, so
      // the walk stays alive; a walk that does not (a token outside every table) keeps the state too.
      if (gslot >= 0) {
        int ns = gs < a.g_A ? gs : -1;
        if (ns >= 0 && t >= 0 && t < a.V) {
          for (int q = a.tok_off[t], q1 = a.tok_off[t + 1]; q < q1 && ns >= 0 && ns < a.g_A; ++q)
            ns = a.g_dfa[(int64_t)ns * 256 + a.tok_dat[q]];
          if (ns < 0 || ns >= a.g_A) ns = gs;
        }
        if (ns >= 0) a.g_state[gslot] = ns;
      }
    }
  }
}

// One wave, lane b = sequence b (B <= 64; the verify form has at most 32 rows): n_acc[b] = the
// draft tokens of b that equal the token drawn for the row before them, up to the first that does
// not; inputs 0 .. n_acc[b] (the last token and the accepted draft tokens) are marked in b's slot.
// A slot belongs to one sequence and a lane marks its ids in turn: plain read-modify-write.
__global__ void __launch_bounds__(64) verify_accept_kernel(const SampleArgs a) {
  const int b = threadIdx.x;
  if (b >= a.B) return;
  const int n = min(a.n_rows[b], a.T);
  const int* tok = a.tok + (int64_t)b * a.T;
  const int64_t* in = a.in_ids + (int64_t)b * a.T;
  int j = 0;
  while (j < n - 1 && (int64_t)tok[j] == in[j + 1]) ++j;
  a.n_acc[b] = j;
  const int slot = a.seen_slot[b];
  if (n <= 0 || slot < 0 || slot >= a.S) return;
  int* srow = a.seen + (int64_t)slot * a.words;
  for (int q = 0; q <= j; ++q) {
    const int64_t id = in[q];
    if (id >= 0 && id < a.V) srow[id >> 5] |= (int)(1u << ((int)id & 31));
  }
}

int64_t sample_ws_floats(int B, int V) {
  const int nch = topk_chunks(V);
  return nch > 1 ? (int64_t)B * nch * (2 * SAMPLE_K + 2) : 0;
}

// the draw of R rows (the decode form: R = a.B; the verify form: R = a.B * a.T)
template <bool VERIFY, bool GUIDED = false>
static hipError_t launch_rows(const SampleArgs& a, int R, float* ws, hipStream_t stream) {
  const int nch = topk_chunks(a.V);
  if (nch == 1) {
    if (a.words > SAMPLE_STAGE_WORDS) return hipErrorInvalidValue;
    hipLaunchKernelGGL((sample_rows_kernel<SAMPLE_SINGLE, VERIFY, GUIDED>), dim3(R, 1), dim3(256), 0, stream, a,
                       nullptr, nullptr, nullptr, 1);
    return hipGetLastError();
  }
  if (ws == nullptr) return hipErrorInvalidValue;
  float* cv = ws;
  int* ci = reinterpret_cast<int*>(ws + (int64_t)R * nch * SAMPLE_K);
  float* pml = ws + (int64_t)R * nch * SAMPLE_K * 2;
  hipLaunchKernelGGL((sample_rows_kernel<SAMPLE_PARTIAL, VERIFY, GUIDED>), dim3(R, nch), dim3(256), 0, stream, a, cv,
                     ci, pml, nch);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((sample_rows_kernel<SAMPLE_MERGE, VERIFY, GUIDED>), dim3(R, 1), dim3(256), 0, stream, a, cv, ci,
                     pml, nch);
  return hipGetLastError();
}

hipError_t sample_rows(const SampleArgs& a, float* ws, hipStream_t stream) {
  if (a.B == 0) return hipSuccess;
  if (a.V < SAMPLE_K || a.words != (a.V + 31) / 32) return hipErrorInvalidValue;
  // the guided form: every guide argument or none (the verify form reads g_allow and g_in only)
  const bool guided = a.g_slot != nullptr || a.g_in != nullptr || a.g_allow != nullptr || a.g_dfa != nullptr ||
                      a.tok_off != nullptr || a.tok_dat != nullptr || a.g_state != nullptr;
  if (guided && (a.g_slot == nullptr || a.g_in == nullptr || a.g_allow == nullptr || a.g_dfa == nullptr ||
                 a.tok_off == nullptr || a.tok_dat == nullptr || a.g_state == nullptr || a.g_A < 1 || a.g_S < 1))
    return hipErrorInvalidValue;
  if (a.T == 0) return guided ? launch_rows<false, true>(a, a.B, ws, stream) : launch_rows<false>(a, a.B, ws, stream);
  if (a.T < 1 || a.T > SAMPLE_VERIFY_MAX_T || a.B > 64 || a.n_rows == nullptr || a.n_acc == nullptr)
    return hipErrorInvalidValue;
  hipError_t e = guided ? launch_rows<true, true>(a, a.B * a.T, ws, stream)
                        : launch_rows<true>(a, a.B * a.T, ws, stream);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(verify_accept_kernel, dim3(1), dim3(64), 0, stream, a);
  return hipGetLastError();
}

}  // namespace lumen
