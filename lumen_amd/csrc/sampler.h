// Device vocab sampler (sampler.hip): repetition penalty, temperature, top-64 candidates,
// nucleus cut and the draw itself in one or two launches that never write the logits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace lumen {

constexpr int SAMPLE_K = 64;   // candidates per row = one wave
constexpr int SAMPLE_VERIFY_MAX_T = 8;   // rows per sequence of the verify form

struct SampleArgs {
  const float* logits;      // [B, V] rows of stride ld; read only
  int64_t ld;
  int B, V;
  const float* inv_t;       // [B] 1 / temperature (1 for a greedy row)
  const double* top_p;      // [B] nucleus mass
  const float* penalty;     // [B] repetition penalty
  const double* u;          // [B] the uniform of this token (unused by a greedy row)
  const int* greedy;        // [B] != 0: take the best candidate
  const int* seen_slot;     // [B] row of `seen`, or -1: no penalty, nothing marked
  int* seen;                // [S, words] bitmaps of the tokens already fed, bit t of a row = token t
  int S, words;             // words = ceil(V / 32)
  const int64_t* in_ids;    // [B] the step's input tokens (penalised like seen ones, then marked)
  int64_t* out_ids;         // [B] sampled tokens; may be the same buffer as in_ids
  int* tok;                 // [B] sampled tokens for the host (-1: no finite logit in the row)
  float* out_v;             // optional [B, 64] candidate values (transformed logits, descending)
  int* out_i;               // optional [B, 64] candidate token ids
  float* out_lse;           // optional [B] log-sum-exp of the transformed row
  // Verify form (speculative decoding), T > 0: logits, u, in_ids, tok and the optional outputs have
  // B * T rows, row b * T + i = input i of sequence b; everything else stays per sequence [B].
  // in_ids of a sequence are its last token and its draft tokens; out_ids is unused.  T = 0: the
  // decode form above.
  int T;
  const int* n_rows;        // [B] live rows of each sequence (a dead row writes tok = -1 only)
  int* n_acc;               // [B] out: accepted draft tokens; in_ids 0 .. n_acc are marked in the slot
  // Guided form (all null / zero when unused): a row whose grammar state s is
  // >= 0 draws among the tokens whose bit is set in g_allow[s], and lane 0 then walks the drawn
  // token's bytes through g_dfa from s and stores the new state.  s = g_in[b] when that is >= 0
  // (a step fed by the host), else g_state[g_slot[b]] (a look-ahead step, straight after the step
  // that wrote it).  g_slot[b] = -1: an unguided row of a guided batch.
  // Verify form, guided (T > 0): g_in has B * T entries, entry b * T + i the state in which row
  // (b, i) draws (the host walks the draft tokens), -1 an unguided row; a state outside the arena
  // allows nothing.  All guide arguments must still be set, but g_slot, g_state, g_dfa and the token
  // bytes are not read and nothing is stored: no state is kept on the device between verify steps.
  const int* g_allow;       // [A, words] arena of allowed-token bitmaps, one row per grammar state
  const int16_t* g_dfa;     // [A, 256] byte transitions in arena-global state ids, -1 = dead
  const int* tok_off;       // [V + 1] CSR of the token bytes ...
  const uint8_t* tok_dat;   // ... and the bytes
  const int* g_slot;        // [B] row of g_state the sequence owns, or -1
  const int* g_in;          // [B] the state fed by the host, or -1: read g_state[g_slot]; verify form: [B * T]
  int* g_state;             // [g_S] the states the device keeps between look-ahead steps
  int g_A, g_S;
};

// floats of workspace sample_rows needs for B rows (the verify form: B * T) of V columns (0: single launch)
int64_t sample_ws_floats(int B, int V);
hipError_t sample_rows(const SampleArgs& a, float* ws, hipStream_t stream);

}  // namespace lumen
