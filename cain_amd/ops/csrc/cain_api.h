// The C API of libcain_kernels.so that crosses a file boundary: every entry point one .hip file defines and another
// calls, declared once (host-only declarations; common.h includes this header, so each definition is checked against
// its prototype), CainGemm, the one call record of every GEMM entry, and CainStep, the one call record of a plan's
// step, with the records it points to (ops/__init__.py mirrors them in ctypes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "spec.h"

#define CAIN_API extern "C" __attribute__((visibility("default")))

extern "C" {

// One GEMM call: Y = epi(B(X)[M, K] . W[N, K]^T).  Every family reads X, ldx, K, N, M, Y, ldy, bias, W, epi and, under
// EPI_QKV_ROPE, slot .. T_max; fields a family does not read are zero.  What else each entry reads:
//   cain_gemm_bf16     norm, eps; waves; ws / ws_bytes (cain_gemm_ws_bytes, zeroed once; null: the skinny kernel)
//   cain_gemm_fp8      norm, eps; sc: fp32 scale per weight row
//   cain_gemm_mxfp4    norm, eps; sc: e8m0 scale bytes; ws / ws_bytes (cain_gemm_w4_ws_bytes; null: never split)
//   cain_gemm_gguf     norm, eps; fmt; sc, dd: the format's scale arrays (dd null for Q4_0); gain; tile0 (Q6_K only)
//   cain_gemm_fp8a8    X / ldx: the e4m3 rows of cain_quant_rows, xs their scales; sc as fp8; ws / ws_bytes
//   cain_gemm_mxfp4a8  the same with sc as mxfp4 (ws: cain_w8a8_ws_bytes for both)
struct CainGemm {
  const void* W;      // packed weights, in the family's packing
  const void* sc;     // weight scales (null: bf16)
  const void* dd;     // GGUF Q4_K (d, dmin) / Q6_K fp32 super-block scales
  const float* gain;  // GGUF: fp32 RMSNorm gain applied to the activations (null: none, or folded into W)
  const float* xs;    // A8: per-row activation scales
  const void* X;
  void* Y;
  const float* bias;
  // EPI_QKV_ROPE
  const int* slot;
  const int* pos;
  const float* cos_t;
  const float* sin_t;
  void* kc;
  void* vtc;
  void* ws;
  long long ws_bytes;
  int ldx, K, N, M, ldy;
  int norm;  // fused RMSNorm of the rows of X
  float eps;
  int H, Hkv, hd, T_max;
  int epi;    // EPI_* (gemm_epi.h), EPI_KV_FP8 or-ed in
  int fmt;    // GGUF: 0 Q4_0, 1 Q4_K, 2 Q6_K (gemm_q.h)
  int tile0;  // GGUF Q6_K: the 16-row tile of the whole projection the first of the N weight rows is
  int waves;  // bf16 skinny kernel: waves per workgroup (0: the rule)
};

// The rows of a forward (runtime.hip): decode -- one row per live sequence; prefill -- one row per prompt token.
struct CainRows {
  int* tok;
  int* pos;
  int* slot;
  // sampling state (decode rows only; may be null for prefill)
  int* n_gen;
  const int* max_new;
  int* done;
  int* hist;
  int* gen;
  int ldg;
  const void* sample_params;
  const void* sample_ext;  // [M] SampleExt (sample.hip: min_p, presence and frequency penalties); null: neutral
};

// Token log-probabilities of a forward (logprob.hip; CainStep::lp).  Decode forwards (want_sample): the statistics
// and the top-n run between the LM head and the sampler, the sampled token's logprob after it, into rings indexed
// like CainRows::gen: lp[m * ldg + n], top_id / top_lp[(m * ldg + n) * 20 + j].
// Forwards with logits but no sampler (teacher forcing): `target` names each row's token, results are per row:
// lp[m], top_id / top_lp[m * 20 + j].
struct CainLogprob {
  const int* topn;  // per row: -1 not wanted, else how many alternatives (0 .. 20)
  int nmax;         // the largest of them
  float* lp;
  int* top_id;
  float* top_lp;
  void* keep;         // decode: cain_logprob_keep_bytes(M) of scratch between the two launches
  const int* target;  // teacher forcing
};

// JSON mode of a decode forward (grammar.hip; CainStep::gr): the mask runs between the LM head (after
// cain_logprob_pre: logprobs stay the model's own distribution) and the sampler, the state advances after it.
struct CainGrammar {
  const int* gram_on;          // per row: 0 off, else the row is in JSON mode
  void* gstate;                // per row: 16 bytes of JsonState (json_pda.h)
  const int* piece_off;        // [V + 1]: token t's bytes are piece_bytes[piece_off[t] .. piece_off[t + 1])
  const uint8_t* piece_bytes;
};

// Stop sequences of a decode forward (stopseq.hip; CainStep::st): the match runs after the sampler, and after JSON
// mode's advance where that is on too (a token it took back is not consumed).
struct CainStop {
  const int* stop_on;          // per row: 0 off, else the row has stop strings
  void* sstate;                // per row: 48 bytes of StopState (stop_match.h)
  const int32_t* stop_len;     // [M][8]: bytes of each string, 0 for an unused entry
  const uint8_t* stop_bytes;   // [M][8][32]
  const int* piece_off;        // the piece table, as CainGrammar's
  const uint8_t* piece_bytes;
};

// Embedding pooling of a prefill-style forward (pool.hip; CainStep::pool): after the last layer the rows of `x` --
// the residual stream -- go through the model's own final RMSNorm (the fp32 `gain`, never folded) into the fp32
// accumulators of their sequences.  seg_off[S + 1] cuts the forward's rows into S runs of consecutive positions of
// one sequence each, seg_dst[s] names the run's row of acc [B][d] / cnt [B]; the runs of one step name distinct rows.
struct CainPool {
  const float* gain;   // [d]
  const int* seg_off;  // [S + 1], ascending, within 0 .. M
  const int* seg_dst;  // [S]
  float* acc;
  int* cnt;
  float* rinv;         // [M] scratch: each row's RMSNorm scale
  int S;
  int mode;            // POOL_MEAN: every row, in ascending order; POOL_LAST: each run's final row only
};
enum { POOL_MEAN = 0, POOL_LAST = 1 };

// One step of a plan, the call record of cain_step_run (enqueue it once) and cain_step_capture (record `steps` of
// them into one graph): a forward over M rows -- with `spec`, a speculative step over M sequences (spec.h).  A null
// feature record leaves the launches exactly those of a step without the feature.  What runtime.hip step_ok refuses
// is refused with -1 before any HIP call.
struct CainStep {
  void* plan;    // cain_plan_create
  void* draft2;  // spec_draft: the draft model's plans for forwards of 2 M and of M rows (null otherwise)
  void* draft1;
  const CainRows* rows;
  const CainLogprob* lp;  // needs want_logits
  const CainGrammar* gr;  // needs want_logits, want_sample and the rows' sampling state
  const CainStop* st;     // likewise
  const CainSpec* spec;   // draft -> forward over M (K + 1) expanded rows -> accept; not with lp / gr / st
  const CainSpecDraft* spec_draft;  // with `spec` in given mode: the draft model proposes the drafts
  const CainPool* pool;   // after the last layer of a forward without logits or sampler; not with lp / gr / st / spec
  int M;
  int want_logits, want_sample;  // a speculative step and every captured step: both 1
};

}  // extern "C"

// ---- the step (runtime.hip)
CAIN_API int cain_step_size();
CAIN_API int cain_step_run(const CainStep* s, hipStream_t st);
CAIN_API void* cain_step_capture(const CainStep* s, int steps, hipStream_t st, int* err);

// ---- GEMMs (gemm.hip, gemm_w8.hip, gemm_w4.hip, gemm_qstream.hip, wgemm8.hip, wgemm.hip)
CAIN_API int cain_gemm_size();
CAIN_API int cain_gemm_bf16(const CainGemm* g, hipStream_t st);
CAIN_API int cain_gemm_fp8(const CainGemm* g, hipStream_t st);
CAIN_API int cain_gemm_mxfp4(const CainGemm* g, hipStream_t st);
CAIN_API int cain_gemm_gguf(const CainGemm* g, hipStream_t st);
CAIN_API int cain_gemm_fp8a8(const CainGemm* g, hipStream_t st);
CAIN_API int cain_gemm_mxfp4a8(const CainGemm* g, hipStream_t st);
CAIN_API int cain_gemm_q4_rows(int K, int epi);
CAIN_API int cain_gemm_q6_rows(int K, int epi);
CAIN_API int cain_quant_rows(const void* x, int ldx, int K, int M, void* x8, int ld8, float* xs, int norm, float eps,
                             hipStream_t st);
CAIN_API int cain_w8a8_eligible(int N, int K, int M);
CAIN_API int cain_wgemm_eligible(int N, int K, int M);
CAIN_API long long cain_wgemm_ws_bytes(int N, int K, int M);
CAIN_API int cain_wgemm_plan(int N, int K, int M);
// Chunk maxima of the next few-row fp32-logits GEMM (gemm.hip): set by the caller, claimed by the entry that runs
// it for its GemmArgs::cmax (null: none pending or N not whole chunks), reported written by cain_gemm_cmax_take()
CAIN_API void cain_gemm_set_cmax(float* cmax);
CAIN_API int cain_gemm_cmax_take();
CAIN_API float* cain_gemm_cmax_claim(int N);

// CUs the launch sizing of the persistent / CU-proportional grids assumes: the device's, or the smaller budget of
// cain_set_cu_budget (runtime.hip) while the work runs on a CU-masked stream (cain_stream_create_cu_limited).
CAIN_API int cain_cu_budget();

// ---- embedding pooling (pool.hip)
CAIN_API int cain_pool_rows(const void* x, int ldx, int M, int d, const float* gain, float eps, const int* seg_off,
                            const int* seg_dst, int S, int mode, float* acc, int* cnt, float* rinv, hipStream_t st);
CAIN_API int cain_pool_finish(const float* acc, const int* cnt, float* out, int B, int d, int normalize,
                              hipStream_t st);

// ---- the rest of a forward (norm.hip, attention.hip, sample.hip, logprob.hip, grammar.hip, stopseq.hip, spec.hip)
CAIN_API int cain_embed(const int* tok, const void* E, void* out, int ldo, int M, int d, float scale, hipStream_t st);
CAIN_API int cain_attention_ex(const void* q, const void* kc, const void* vtc, const int* slot, const int* pos,
                               float* part_o, float* part_ml, unsigned* counters, void* out, int ldo, int M, int H,
                               int Hkv, int hd, int T_max, int nsplit, float scale, int kv8, float kscale,
                               float vscale, hipStream_t st);
CAIN_API int cain_attention(const void* q, const void* kc, const void* vtc, const int* slot, const int* pos,
                            float* part_o, float* part_ml, unsigned* counters, void* out, int ldo, int M, int H,
                            int Hkv, int hd, int T_max, int nsplit, float scale, hipStream_t st);
CAIN_API int cain_sample(float* logits, int ldl, int V, int* tok, int* pos, int* gen, int ldg, int* n_gen,
                         const int* max_new, int* done, int* hist, const int* slot, int T_max, int M,
                         const void* params, const void* ext, hipStream_t st);
CAIN_API int cain_sample_ext_size();
CAIN_API long long cain_sample_ws_bytes(int M);
CAIN_API int cain_sample_split_max();
CAIN_API int cain_sample_cm_enabled();
CAIN_API int cain_sample_cm(float* logits, int ldl, int V, const float* cmax, int* tok, int* pos, int* gen, int ldg,
                            int* n_gen, const int* max_new, int* done, int* hist, const int* slot, int T_max, int M,
                            const void* params, const void* ext, hipStream_t st);
CAIN_API int cain_sample_lean(float* logits, int ldl, int V, const float* cmax, int* tok, int* pos, int* gen, int ldg,
                              int* n_gen, const int* max_new, int* done, int* hist, const int* slot, int T_max, int M,
                              const void* params, const void* ext, hipStream_t st);
CAIN_API int cain_sample_ex(float* logits, int ldl, int V, int* tok, int* pos, int* gen, int ldg, int* n_gen,
                            const int* max_new, int* done, int* hist, const int* slot, int T_max, int M,
                            const void* params, const void* ext, void* ws, long long ws_bytes, hipStream_t st);
CAIN_API int cain_logprob_rows(const float* logits, int ldl, int V, int M, const int* slot, const int* done,
                               const int* topn, int nmax, const int* target, float* lse, float* lp, int* top_id,
                               float* top_lp, hipStream_t st);
CAIN_API int cain_logprob_pre(const float* logits, int ldl, int V, int M, const int* slot, const int* done,
                              const int* topn, int nmax, const int* n_gen, const int* hist, int ldg, int* top_id,
                              float* top_lp, void* keep, hipStream_t st);
CAIN_API int cain_logprob_chosen(const float* logits, int ldl, int V, int M, const int* gen, int ldg, const void* keep,
                                 float* lp, hipStream_t st);
CAIN_API int cain_json_mask(float* logits, int ldl, int V, int M, const int* gram_on, const int* done,
                            const void* gstate, const int* piece_off, const uint8_t* piece_bytes, float* cmax,
                            hipStream_t st);
CAIN_API int cain_json_advance(int M, int V, const int* gram_on, const int* gen, int ldg, int* n_gen, int* done,
                               void* gstate, const int* piece_off, const uint8_t* piece_bytes, hipStream_t st);
CAIN_API int cain_stop_advance(int M, int V, const int* stop_on, const int* gen, int ldg, const int* n_gen, int* done,
                               void* sstate, const int32_t* stop_len, const uint8_t* stop_bytes, const int* piece_off,
                               const uint8_t* piece_bytes, hipStream_t st);
CAIN_API int cain_stop_state_size();
CAIN_API int cain_spec_draft(const CainSpec* s, int R, int T_max, const int* tok, const int* pos, const int* slot,
                             const int* n_gen, const int* max_new, const int* done, const int* hist,
                             const void* params, hipStream_t st);
CAIN_API int cain_spec_accept(const CainSpec* s, int R, int T_max, int* tok, int* pos, const int* slot, int* n_gen,
                              const int* max_new, int* done, int* hist, int* gen, int ldg, const void* params,
                              hipStream_t st);
CAIN_API int cain_spec_model_rows(const CainSpecDraft* s, int R, int T_max, const int* tok, const int* pos,
                                  const int* slot, const int* n_gen, const int* max_new, const int* done,
                                  const int* hist, const void* params, hipStream_t st);
CAIN_API int cain_spec_model_next(const CainSpecDraft* s, int R, int j, int T_max, const int* slot, const int* n_gen,
                                  hipStream_t st);
CAIN_API int cain_spec_dvalid(const CainSpecDraft* s, int R, int T_max, const int* slot, const int* pos,
                              hipStream_t st);
