// Speculative decoding state shared by spec.hip (draft / accept kernels) and runtime.hip (the spec graphs).
#pragma once
#include <hip/hip_runtime.h>

constexpr int SPEC_K_MAX = 7;  // drafts per sequence and step: a sequence verifies at most 8 rows

extern "C" {

// One decode batch of R sequences verified K + 1 rows per sequence: row x = r (K + 1) + j of the expanded state is
// sequence r's own row (j = 0) or its j-th draft (engine/speculative.py states the rule).
struct CainSpec {
  int K;      // 1 .. SPEC_K_MAX
  int mode;   // 0: n-gram lookup in the sequence's own record; 1: drafts given by the caller
  int slots;  // rows of `seq`
  int lds;    // its row stride (>= T_max)
  int ldv;    // row stride of `given`
  int ldt;    // row stride of `step_tokens` (a ring: step % ldt)
  int vocab;  // a given draft id outside [0, vocab) ends the draft
  int ldg;    // row stride of x_gen
  int* seq;          // [slots][lds]: the tokens of each cache slot by position (prompt, then generated)
  const int* given;  // [R][ldv]: mode 1, the draft of generated index n at [r][n]; negative ends a draft
  // expanded row state, R (K + 1) rows (the CainRows of the verify forward)
  int* x_tok;
  int* x_pos;
  int* x_slot;
  int* x_n_gen;
  int* x_max_new;
  int* x_done;
  int* x_hist;  // [R (K + 1)][64]
  int* x_gen;   // [R (K + 1)][ldg]: the sampler's output ring of the expanded rows (scratch)
  void* x_params;  // [R (K + 1)] SampleParams
  int* nd;     // [R]: drafts of this step
  int* draft;  // [R][K]: their ids (-1 beyond nd)
  // per sequence counters
  int* drafted;
  int* accepted;
  int* n_step;       // steps the sequence was live for
  int* step_tokens;  // [R][ldt]: tokens committed by step n_step % ldt
};

// Draft-model mode (engine/speculative.py "Draft model"): a second, smaller model with its own plan and KV cache
// proposes the step's K tokens and writes them into CainSpec::given; verify and accept are given mode, unchanged.
// The draft rows are the CainRows of the draft plan's forwards: row r < R is sequence r's sampled row (the input of
// draft forward j at position pos + j - 1), row R + r its catch-up row at pos - 1 (first forward only).
struct CainSpecDraft {
  int K;       // 1 .. SPEC_K_MAX (the CainSpec's)
  int dvocab;  // rows of the draft model's embedding: a token id outside [0, dvocab) enters as `dbos`
  int dbos;    // the draft model's bos id, in [0, dvocab)
  int slots;   // rows of `seq` and entries of `dvalid` (cache slots of both models)
  int lds;     // row stride of `seq` (>= T_max)
  int ldv;     // row stride of `given`
  int ldg;     // row stride of r_gen
  int pad_;
  const int* seq;  // CainSpec::seq
  int* given;      // CainSpec::given: the drafts of generated index n at [r][n]
  int* dvalid;     // [slots]: leading positions of the slot's draft cache that hold K / V of seq
  int* p0;         // [R]: the sequence's position before the step
  int* nd;         // [R]: draft forwards the sequence is live for this step (d; 0: none)
  // the draft rows, 2 R of them
  int* r_tok;
  int* r_pos;
  int* r_slot;
  int* r_n_gen;
  int* r_max_new;
  int* r_done;
  int* r_hist;     // [2 R][64]
  int* r_gen;      // [2 R][ldg]: the sampler's output ring of the draft rows (scratch)
  void* r_params;  // [2 R] SampleParams: the request's own, stop ids off
};

}  // extern "C"
