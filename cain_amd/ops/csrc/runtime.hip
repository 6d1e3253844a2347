// Native decode runtime: the per-step kernel schedule of one model and its
// hipGraph capture/replay.
//
// The Python engine owns every buffer (torch allocations on the GPU) and hands
// the raw pointers over once in a PlanDesc.  Every step crosses the C boundary
// as one record, CainStep (cain_api.h): the plan, the rows and, each null when
// off, the records of the decode-time features (token log-probabilities, JSON
// mode, stop sequences, speculative decoding with or without a draft model).
// `cain_step_run` enqueues one step: a forward over M rows (decode: one row per
// live sequence; prefill: one row per prompt token, each with its own cache slot
// and position):
//
//   embed -> L x [QKV GEMM(+RMSNorm, +bias, RoPE, KV append)
//                 -> attention(+split combine) -> O GEMM(+residual)
//                 -> gate/up GEMM(+RMSNorm, act*mul) -> down GEMM(+residual)]
//                 -> LM-head GEMM(+RMSNorm) -> sample
//
// = 5 launches per layer (the unfused schedule had 9).  `cain_step_capture` records `steps` consecutive
// decode steps into ONE hipGraph; since the sampler advances tok/pos/n_gen on
// the device, a whole generation is a handful of graph launches with no host
// round trip per token (graph-replay floor instead of ~290 host launches per
// token: MI355X_MICROARCH.md rows 'boundary', 'graph-replay-floor').
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "common.h"

constexpr int CAIN_MAX_ROWS = 256;  // rows per forward (decode batch / prefill chunk)

extern "C" {

// weight storage of a plan (CainPlanDesc::wfmt)
enum { WFMT_BF16 = 0, WFMT_FP8 = 1, WFMT_FP4 = 2, WFMT_Q4_0 = 3, WFMT_Q4_K = 4 };
// format of one matrix of a WFMT_Q4_* plan (CainLayer::f*, CainPlanDesc::flm_head): 0 = the plan's wfmt, else
// WFMT_Q4_0 / WFMT_Q4_K or Q6_K (gemm_qstream.hip: a Q4_K_M file's output head, attn_v and ffn_down tensors)
enum { MFMT_PLAN = 0, MFMT_Q6_K = 5 };

// RMSNorm gains are folded into the weight columns of the GEMM each norm feeds (attn_norm -> wqkv,
// mlp_norm -> wgu, final_norm -> lm_head; models/weights.py fold_gain), so a norm is just a flag here.
struct CainLayer {
  const void* wqkv;
  const float* bqkv;
  const void* wo;
  const void* wgu;
  const void* wdown;
  // scales of each packed matrix (null for bf16): fp8 -- fp32 per output row; fp4 -- e8m0 bytes per 32-k block in
  // the kernel's lane order (models/weights.py pack_mxfp4)
  const void* sqkv;
  const void* so;
  const void* sgu;
  const void* sdown;
  // fp8 weights in the W8A8 wide kernel's packing (wgemm8.hip; null: W8A16 only), same scales as above
  const void* wqkv8;
  const void* wo8;
  const void* wgu8;
  const void* wdown8;
  // WFMT_Q4_* plans: each matrix's format (MFMT_*; 0: the plan's), and the V rows of the QKV projection packed on
  // their own as Q6_K (null: V is inside wqkv, which then has all (H + 2 Hkv) hd rows)
  int fqkv, fo, fgu, fdown;
  const void* wv;
  const void* sv;
};

struct CainPlanDesc {
  int n_layers, d, H, Hkv, hd, ffn, V, act_kind, T_max, Mpad, nsplit, waves;
  float eps, embed_scale, attn_scale;
  const void* embed;
  const void* lm_head;
  const CainLayer* layers;
  void* kcache;  // [L][S][Hkv][T_max][hd] fragment-major, bf16 (kv8: e4m3)
  void* vtcache; // [L][S][Hkv][hd][T_max]
  long long kv_layer_elems;
  const float* cos_t;
  const float* sin_t;
  void* x;
  void* q;
  void* attn;
  void* act;
  float* logits;
  float* part_o;
  float* part_ml;
  unsigned* counters;
  void* gemm_ws;  // batched-GEMM workspace (counters zeroed once + split-K partials), see gemm.hip
  long long gemm_ws_bytes;
  // WFMT_FP8: e4m3 weights with per-row scales, W8A16 kernels (gemm_w8.hip) up to 64 rows (W8A8 above 16 rows
  // when the <name>8 packings are present); WFMT_FP4: MXFP4 weights, W4A16 kernels (gemm_w4.hip) up to 64 rows,
  // W4A8 (wgemm8.hip FP4, the same packed bytes) above 16 rows (cain_w4a8_set_min_rows) when x8 / xs are present
  int wfmt;
  const void* lm_head_scale;  // fp8 / fp4: scales of the packed LM head
  // 1: the KV caches hold fp8 e4m3 elements (same fragment-major offsets, one byte each, unscaled and
  // saturated at +-448): the QKV epilogue writes them (gemm_epi.h EPI_KV_FP8), attention widens them
  int kv8;
  // W8A8 (fp8 with the <name>8 packings) / W4A8 (fp4): wide forwards quantise each GEMM input per row into
  // x8 [Mpad][x8_ld] e4m3 + xs [Mpad] (wgemm8.hip quant_rows_kernel) and run the scaled-MFMA wide kernel
  const void* lm_head8;
  void* x8;
  float* xs;
  int x8_ld;
  // WFMT_Q4_*: 1 when each norm-fed weight's scale buffer ends with its fp32 RMSNorm gain (weights not gain-folded)
  int q4_gain;
  int flm_head;  // WFMT_Q4_* plans: the LM head's format (MFMT_*; 0: the plan's)
};

}  // extern "C"

namespace {

struct Plan {
  CainPlanDesc d;
  std::vector<CainLayer> layers;
  // two-stage sampler workspace (sample.hip cain_sample_ex) for decode forwards of <= 64 rows, zeroed once
  void* sample_ws = nullptr;
  long long sample_ws_bytes = 0;
  // LM-head chunk maxima ([Mpad][V / 16] floats; sample.hip sample_cm_kernel)
  float* cmax = nullptr;
  ~Plan() {
    if (sample_ws) (void)hipFree(sample_ws);
    if (cmax) (void)hipFree(cmax);
  }
};

// first failing call of the last failed forward (source text + line), for the Python error message
thread_local char g_fail[160] = {0};

#define CK(x)                                                                    \
  do {                                                                           \
    int _e = (x);                                                                \
    if (_e != 0) {                                                               \
      if (!g_fail[0]) snprintf(g_fail, sizeof(g_fail), "runtime.hip:%d %s", __LINE__, #x); \
      return _e;                                                                 \
    }                                                                            \
  } while (0)

// Rows above which an fp4 plan with x8 runs W4A8 (the W4A16 kernels take up to 64): 16, the W4A8 minimum -- at 24 /
// 48 / 64 rows W4A8 decodes 7.7k / 13.6k / 16.6k tok/s against W4A16's 5.1k / 5.0k / 6.4k
// (profiles/r4/ab/w4a8_crossover.txt)
static int g_w4a8_min_rows = 16;

// rows a forward of this plan may have: 64 for the few-row-only weight formats
int max_rows(const CainPlanDesc& d) {
  if ((d.wfmt == WFMT_FP4 || d.wfmt == WFMT_FP8) && !d.x8) return d.Mpad < 64 ? d.Mpad : 64;
  if (d.wfmt == WFMT_Q4_0 || d.wfmt == WFMT_Q4_K) return d.Mpad < 64 ? d.Mpad : 64;  // 16-row launches (gemm_qstream.hip)
  return d.Mpad < CAIN_MAX_ROWS ? d.Mpad : CAIN_MAX_ROWS;
}

// 5 launches per layer: QKV(+RMSNorm, bias, RoPE, KV append) -> attention(+combine) ->
// O(+residual) -> gate/up(+RMSNorm, act*mul) -> down(+residual); 6 in a layer whose V rows are Q6_K beside Q4 q / k.
// lq: the caller's logprob buffers (null: none -- the launches are exactly those of a plan without the feature)
// gr: JSON mode's buffers (null: none, likewise)
// sq: the stop sequences' buffers (null: none, likewise)
// pl: embedding pooling of the rows after the last layer (null: none, likewise; step_ok: no logits, no sampler)
int forward(const Plan& p, int M, const CainRows& r, int want_logits, int want_sample, hipStream_t st,
            const CainLogprob* lq = nullptr, const CainGrammar* gr = nullptr, const CainStop* sq = nullptr,
            const CainPool* pl = nullptr) {
  const CainPlanDesc& d = p.d;
  const int qkv_dim = (d.H + 2 * d.Hkv) * d.hd;
  const int q_dim = d.H * d.hd;
  const int epi_act = d.act_kind == 1 ? 4 : 3;
  // one GEMM of the schedule: the bf16 kernels (gemm.hip / wgemm.hip), fp8 weights (gemm_w8.hip / wgemm8.hip) or
  // MXFP4 weights (gemm_w4.hip)
  // mf: the matrix's own format in a GGUF plan (MFMT_*); tile0: the first 16-row tile of N in the epilogue's eyes
  // (Q6_K only: the V rows of a QKV projection launched on their own)
  auto gemm = [&](const void* W, const void* W8, const void* ws, const void* X, int ldx, int K, int N, void* Y,
                  int ldy, const float* bias, int norm, const void* kc, const void* vc, int epi, int mf = MFMT_PLAN,
                  int tile0 = 0) -> int {
    CainGemm g{};
    g.W = W, g.sc = ws, g.X = X, g.ldx = ldx, g.K = K, g.N = N, g.M = M, g.Y = Y, g.ldy = ldy, g.bias = bias;
    g.norm = norm, g.eps = d.eps, g.slot = r.slot, g.pos = r.pos, g.cos_t = d.cos_t, g.sin_t = d.sin_t;
    g.kc = const_cast<void*>(kc), g.vtc = const_cast<void*>(vc);
    g.H = d.H, g.Hkv = d.Hkv, g.hd = d.hd, g.T_max = d.T_max, g.epi = epi, g.tile0 = tile0;
    const bool gguf = d.wfmt == WFMT_Q4_0 || d.wfmt == WFMT_Q4_K;
    const bool q6 = gguf && mf == MFMT_Q6_K;
    if (!q6 && (tile0 != 0 || (mf != MFMT_PLAN && !(gguf && (mf == WFMT_Q4_0 || mf == WFMT_Q4_K))))) return -1;
    const int qf = gguf ? (mf == MFMT_PLAN ? d.wfmt : mf) : 0;
    // W4A8 / W8A8: the rows quantised per row to fp8 for the scaled-MFMA wide kernels
    auto a8 = [&]() -> int {
      g.X = d.x8, g.ldx = d.x8_ld, g.xs = d.xs, g.ws = d.gemm_ws, g.ws_bytes = d.gemm_ws_bytes;
      return cain_quant_rows(X, ldx, K, M, d.x8, d.x8_ld, d.xs, norm, d.eps, st);
    };
    if (d.wfmt == WFMT_FP4 && d.x8 && (M > g_w4a8_min_rows || M > 64) && cain_w8a8_eligible(N, K, M)) {
      CK(a8());
      return cain_gemm_mxfp4a8(&g, st);
    }
    if (gguf) {
      // ws = [scales: N K / 16 bytes (Q4: per block, Q6_K: int8 per group)][Q4_K: (d, dmin), Q6_K: fp32 d: N K / 64
      // bytes][the fp32 norm gain over K, when the plan keeps gains unfolded (a GGUF file's exact values)]
      const char* dd = static_cast<const char*>(ws) + (size_t)N * K / 16;
      g.fmt = q6 ? 2 : qf == WFMT_Q4_K;
      g.dd = dd;
      if (d.q4_gain && norm) g.gain = reinterpret_cast<const float*>(dd + (g.fmt ? (size_t)N * K / 64 : 0));
      return cain_gemm_gguf(&g, st);
    }
    if (d.wfmt == WFMT_FP4) {
      g.ws = d.gemm_ws, g.ws_bytes = d.gemm_ws_bytes;
      return cain_gemm_mxfp4(&g, st);
    }
    if (d.wfmt == WFMT_FP8 && W8 && d.x8 && cain_w8a8_eligible(N, K, M)) {
      CK(a8());
      g.W = W8;
      return cain_gemm_fp8a8(&g, st);
    }
    if (d.wfmt == WFMT_FP8) return cain_gemm_fp8(&g, st);
    g.ws = d.gemm_ws, g.ws_bytes = d.gemm_ws_bytes, g.waves = d.waves;
    return cain_gemm_bf16(&g, st);
  };
  CK(cain_embed(r.tok, d.embed, d.x, d.d, M, d.d, d.embed_scale, st));
  for (int l = 0; l < d.n_layers; ++l) {
    const CainLayer& L = p.layers[l];
    const size_t kv_off = (size_t)l * d.kv_layer_elems * (d.kv8 ? 1 : 2);  // bytes
    char* kc = static_cast<char*>(d.kcache) + kv_off;
    char* vc = static_cast<char*>(d.vtcache) + kv_off;
    const int epi_qkv = /*EPI_QKV_ROPE*/ 5 | (d.kv8 ? /*EPI_KV_FP8*/ 0x100 : 0);
    if (L.wv) {
      // V in Q6_K beside Q4 q / k rows (a Q4_K_M layer): two launches, both staging and normalising the activations
      // -- the q and k rows with their RoPE and K append (the epilogue keys on H / Hkv / hd, not N), then the V rows
      // with the tile offset that makes them the projection's V block
      const int nqk = (d.H + d.Hkv) * d.hd;
      CK(gemm(L.wqkv, nullptr, L.sqkv, d.x, d.d, d.d, nqk, d.q, q_dim, L.bqkv, 1, kc, vc, epi_qkv, L.fqkv));
      CK(gemm(L.wv, nullptr, L.sv, d.x, d.d, d.d, qkv_dim - nqk, d.q, q_dim, L.bqkv, 1, kc, vc, epi_qkv, MFMT_Q6_K,
              nqk / 16));
    } else {
      CK(gemm(L.wqkv, L.wqkv8, L.sqkv, d.x, d.d, d.d, qkv_dim, d.q, q_dim, L.bqkv, 1, kc, vc, epi_qkv, L.fqkv));
    }
    CK(cain_attention_ex(d.q, kc, vc, r.slot, r.pos, d.part_o, d.part_ml, d.counters, d.attn, q_dim, M, d.H, d.Hkv,
                         d.hd, d.T_max, d.nsplit, d.attn_scale, d.kv8, 1.f, 1.f, st));
    CK(gemm(L.wo, L.wo8, L.so, d.attn, q_dim, q_dim, d.d, d.x, d.d, nullptr, 0, nullptr, nullptr, /*EPI_RESID*/ 1,
            L.fo));
    CK(gemm(L.wgu, L.wgu8, L.sgu, d.x, d.d, d.d, 2 * d.ffn, d.act, d.ffn, nullptr, 1, nullptr, nullptr, epi_act,
            L.fgu));
    CK(gemm(L.wdown, L.wdown8, L.sdown, d.act, d.ffn, d.ffn, d.d, d.x, d.d, nullptr, 0, nullptr, nullptr,
            /*EPI_RESID*/ 1, L.fdown));
  }
  if (pl)
    CK(cain_pool_rows(d.x, d.d, M, d.d, pl->gain, d.eps, pl->seg_off, pl->seg_dst, pl->S, pl->mode, pl->acc, pl->cnt,
                      pl->rinv, st));
  if (want_logits) {
    // the LM head also writes the chunk maxima the chunk-max samplers start from (the bf16 skinny / wide kernels and
    // the few-row fp8 / MXFP4 / Q4 kernels; a kernel that does not leaves cain_gemm_cmax_take() at 0)
    const int cm_mode = cain_sample_cm_enabled();
    if (p.cmax && (cm_mode == 1 || cm_mode == 3 || (cm_mode == 2 && M > 64))) cain_gemm_set_cmax(p.cmax);
    CK(gemm(d.lm_head, d.lm_head8, d.lm_head_scale, d.x, d.d, d.d, d.V, d.logits, d.V, nullptr, 1, nullptr, nullptr,
            /*EPI_F32*/ 2, d.flm_head));
  }
  const bool cm = want_logits && cain_gemm_cmax_take();
  if (lq && !want_logits) return -1;
  if (lq && want_sample)  // before the sampler: two of its kernels apply the repeat penalty in place on the logits
    CK(cain_logprob_pre(d.logits, d.V, d.V, M, r.slot, r.done, lq->topn, lq->nmax, r.n_gen, r.hist, r.ldg, lq->top_id,
                        lq->top_lp, lq->keep, st));
  if (lq && !want_sample)
    CK(cain_logprob_rows(d.logits, d.V, d.V, M, r.slot, nullptr, lq->topn, lq->nmax, lq->target, nullptr, lq->lp,
                         lq->top_id, lq->top_lp, st));
  if (gr)  // the chunk maxima the LM head wrote are rewritten from the masked logits (a sampler starts from them)
    CK(cain_json_mask(d.logits, d.V, d.V, M, gr->gram_on, r.done, gr->gstate, gr->piece_off, gr->piece_bytes,
                      cm ? p.cmax : nullptr, st));
  if (want_sample) {
    // the chunk-max sampler refuses (< 0) vocabularies beyond its chunk capacity: the two-stage / one-workgroup
    // kernels take those
    const int cm_mode = cain_sample_cm_enabled();
    const int e = !cm ? -1
                  : cm_mode == 3 ? cain_sample_lean(d.logits, d.V, d.V, p.cmax, r.tok, r.pos, r.gen, r.ldg, r.n_gen,
                                                    r.max_new, r.done, r.hist, r.slot, d.T_max, M, r.sample_params,
                                                    r.sample_ext, st)
                                 : cain_sample_cm(d.logits, d.V, d.V, p.cmax, r.tok, r.pos, r.gen, r.ldg, r.n_gen,
                                                  r.max_new, r.done, r.hist, r.slot, d.T_max, M, r.sample_params,
                                                  r.sample_ext, st);
    if (e > 0) CK(e);
    if (e < 0)
      CK(cain_sample_ex(d.logits, d.V, d.V, r.tok, r.pos, r.gen, r.ldg, r.n_gen, r.max_new, r.done, r.hist, r.slot,
                        d.T_max, M, r.sample_params, r.sample_ext, p.sample_ws, p.sample_ws_bytes, st));
    if (lq) CK(cain_logprob_chosen(d.logits, d.V, d.V, M, r.gen, r.ldg, lq->keep, lq->lp, st));
    if (gr)
      CK(cain_json_advance(M, d.V, gr->gram_on, r.gen, r.ldg, r.n_gen, r.done, gr->gstate, gr->piece_off,
                           gr->piece_bytes, st));
    if (sq)
      CK(cain_stop_advance(M, d.V, sq->stop_on, r.gen, r.ldg, r.n_gen, r.done, sq->sstate, sq->stop_len,
                           sq->stop_bytes, sq->piece_off, sq->piece_bytes, st));
  }
  return 0;
}

// One speculative decode step over R sequences (spec.hip): draft into the expanded state, verify with the ordinary
// forward over R (K + 1) rows -- logits and the ordinary sampler on the expanded rows -- then commit what matched.
int forward_spec(const Plan& p, int R, const CainRows& r, const CainSpec& s, hipStream_t st) {
  const int T = p.d.T_max;
  CK(cain_spec_draft(&s, R, T, r.tok, r.pos, r.slot, r.n_gen, r.max_new, r.done, r.hist, r.sample_params, st));
  CainRows x{};  // (sample_ext stays null: the expanded rows have no SampleExt records, the engine refuses the mix)
  x.tok = s.x_tok, x.pos = s.x_pos, x.slot = s.x_slot, x.n_gen = s.x_n_gen, x.max_new = s.x_max_new;
  x.done = s.x_done, x.hist = s.x_hist, x.gen = s.x_gen, x.ldg = s.ldg, x.sample_params = s.x_params;
  CK(forward(p, R * (s.K + 1), x, 1, 1, st));
  CK(cain_spec_accept(&s, R, T, r.tok, r.pos, r.slot, r.n_gen, r.max_new, r.done, r.hist, r.gen, r.ldg,
                      r.sample_params, st));
  return 0;
}

// One speculative step whose drafts a draft model proposes (spec.h CainSpecDraft): the draft rows from the decode
// state, the draft plan's forward over 2 R rows (each sequence's catch-up row and its own row, sampled with the
// request's options), K - 1 further draft forwards over R rows, each fed by the token the one before sampled; every
// sampled token lands in `given`, which the given-mode step then verifies.  `d2` / `d1`: the draft model's plans for
// forwards of 2 R and of R rows (they differ in their attention split count only).  All on the one stream.
int forward_spec_model(const Plan& p, const Plan& d2, const Plan& d1, int R, const CainRows& r, const CainSpec& s,
                       const CainSpecDraft& sd, hipStream_t st) {
  const int T = p.d.T_max;
  CK(cain_spec_model_rows(&sd, R, T, r.tok, r.pos, r.slot, r.n_gen, r.max_new, r.done, r.hist, r.sample_params, st));
  CainRows x{};  // (sample_ext null, as forward_spec's rows)
  x.tok = sd.r_tok, x.pos = sd.r_pos, x.slot = sd.r_slot, x.n_gen = sd.r_n_gen, x.max_new = sd.r_max_new;
  x.done = sd.r_done, x.hist = sd.r_hist, x.gen = sd.r_gen, x.ldg = sd.ldg, x.sample_params = sd.r_params;
  CK(forward(d2, 2 * R, x, 1, 1, st));
  for (int j = 1; j < sd.K; ++j) {
    CK(cain_spec_model_next(&sd, R, j, T, r.slot, r.n_gen, st));
    CK(forward(d1, R, x, 1, 1, st));
  }
  CK(cain_spec_model_next(&sd, R, sd.K, T, r.slot, r.n_gen, st));  // d_K into `given`
  CK(forward_spec(p, R, r, s, st));
  CK(cain_spec_dvalid(&sd, R, T, r.slot, r.pos, st));
  return 0;
}

// What both step entries refuse before anything is launched (`capture`: cain_step_capture, of `steps` steps).
// First what can be told without reading the plan: a null record, plan or rows, a combination that does not exist,
// a missing buffer.
//   lp          logprobs without logits, or with a result buffer missing
//   gr, st      JSON mode or stop sequences on anything but a decode forward (logits, sampler and the rows' sampling
//               state), or with a table or state missing
//   pool        together with logits, the sampler, lp, gr, st, spec or a capture; a buffer missing; more runs than
//               rows; a width cain_pool_rows refuses
//   spec        together with lp, gr or st (the K + 1 expanded rows would each need the state after their drafts);
//               K outside 1 .. SPEC_K_MAX; rows without sampling state; M (K + 1) rows above what a forward of the
//               plan may have; a draft vocabulary beyond the plan's
//   spec_draft  without spec, or a spec that is not in given mode over the draft record's own buffers; a draft plan
//               or a buffer missing; 2 M rows above what a forward of the draft plan may have; plans of different
//               T_max; a draft vocabulary beyond the draft plan's
bool step_ok(const CainStep* sp, bool capture, int steps) {
  if (!sp || !sp->plan || !sp->rows || (capture && steps < 1) || sp->M < 1) return false;
  const CainStep& s = *sp;
  const CainRows& r = *s.rows;
  const CainSpec* sc = s.spec;
  const CainSpecDraft* sd = s.spec_draft;
  if ((capture || sc) && !(s.want_logits && s.want_sample)) return false;
  if ((sc && (s.lp || s.gr || s.st)) || (sd && !sc)) return false;
  if (s.pool) {
    const CainPool& q = *s.pool;
    if (capture || s.want_logits || s.want_sample || s.lp || s.gr || s.st || sc || sd) return false;
    if (!(q.gain && q.seg_off && q.seg_dst && q.acc && q.cnt && q.rinv) || q.S < 0 || q.S > s.M) return false;
    if (q.mode != POOL_MEAN && q.mode != POOL_LAST) return false;
  }
  if (s.lp && (!s.want_logits || !s.lp->topn)) return false;
  if (s.lp && s.want_sample && (!s.lp->keep || !s.lp->lp || !s.lp->top_id || !s.lp->top_lp)) return false;
  if ((s.gr || s.st) && (!s.want_logits || !s.want_sample || !r.n_gen || !r.done || !r.gen || r.ldg < 1)) return false;
  if (s.gr && !(s.gr->gram_on && s.gr->gstate && s.gr->piece_off && s.gr->piece_bytes)) return false;
  if (s.st && !(s.st->stop_on && s.st->sstate && s.st->stop_len && s.st->stop_bytes && s.st->piece_off &&
                s.st->piece_bytes))
    return false;
  if (sc && (sc->K < 1 || sc->K > SPEC_K_MAX || !r.n_gen || !r.max_new || !r.done || !r.hist || !r.gen ||
             !r.sample_params))
    return false;
  if (sd) {
    if (!s.draft2 || !s.draft1) return false;
    if (sc->mode != 1 || sd->K != sc->K || sd->given != sc->given || sd->seq != sc->seq || sd->ldv != sc->ldv ||
        sd->lds != sc->lds || sd->slots != sc->slots)
      return false;
    if (sd->dvocab < 1 || sd->dbos < 0 || sd->dbos >= sd->dvocab || sd->ldg < 1) return false;
    if (!(sd->dvalid && sd->p0 && sd->nd && sd->r_tok && sd->r_pos && sd->r_slot && sd->r_n_gen && sd->r_max_new &&
          sd->r_done && sd->r_hist && sd->r_gen && sd->r_params && r.tok && r.pos && r.slot))
      return false;
  }
  // ... then against the plans
  const CainPlanDesc& d = static_cast<const Plan*>(s.plan)->d;
  if (s.M * (sc ? sc->K + 1 : 1) > max_rows(d) || (sc && sc->vocab > d.V)) return false;
  if (s.pool && (d.d % 8 || d.d < 8 || d.d > 16384)) return false;
  if (sd) {
    const CainPlanDesc& d2 = static_cast<const Plan*>(s.draft2)->d;
    const CainPlanDesc& d1 = static_cast<const Plan*>(s.draft1)->d;
    if (d2.T_max != d.T_max || d1.T_max != d.T_max || d2.V != d1.V) return false;
    if (2 * s.M > max_rows(d2) || s.M > max_rows(d1) || sd->dvocab > d2.V) return false;
  }
  return true;
}

// The step of a record step_ok passed: the plain forward, or the speculative step with or without a draft model.
int run_step(const CainStep& s, hipStream_t st) {
  const Plan& p = *static_cast<const Plan*>(s.plan);
  if (s.spec_draft)
    return forward_spec_model(p, *static_cast<const Plan*>(s.draft2), *static_cast<const Plan*>(s.draft1), s.M,
                              *s.rows, *s.spec, *s.spec_draft, st);
  if (s.spec) return forward_spec(p, s.M, *s.rows, *s.spec, st);
  return forward(p, s.M, *s.rows, s.want_logits, s.want_sample, st, s.lp, s.gr, s.st, s.pool);
}

// `steps` calls of `step` recorded on `st` into one executable graph (null and *err on failure).
template <class F>
void* capture_steps(hipStream_t st, int steps, int* err, F step) {
  hipGraph_t g = nullptr;
  hipError_t e = hipStreamBeginCapture(st, hipStreamCaptureModeThreadLocal);
  if (e != hipSuccess) {
    *err = int(e);
    return nullptr;
  }
  int fe = 0;
  for (int s = 0; s < steps && fe == 0; ++s) fe = step();
  e = hipStreamEndCapture(st, &g);
  if (fe != 0 || e != hipSuccess) {
    *err = fe ? fe : int(e);
    if (g) (void)hipGraphDestroy(g);
    return nullptr;
  }
  hipGraphExec_t ex = nullptr;
  e = hipGraphInstantiate(&ex, g, nullptr, nullptr, 0);
  (void)hipGraphDestroy(g);
  if (e != hipSuccess) {
    *err = int(e);
    return nullptr;
  }
  return ex;
}

}  // namespace

extern "C" {

CAIN_API void* cain_plan_create(const CainPlanDesc* desc) {
  auto* p = new Plan();
  p->d = *desc;
  p->layers.assign(desc->layers, desc->layers + desc->n_layers);
  p->d.layers = p->layers.data();
  const int ms = desc->Mpad < cain_sample_split_max() ? desc->Mpad : cain_sample_split_max();
  if (ms > 0) {
    const long long nb = cain_sample_ws_bytes(ms);
    if (hipMalloc(&p->sample_ws, nb) == hipSuccess && hipMemset(p->sample_ws, 0, nb) == hipSuccess) {
      p->sample_ws_bytes = nb;
    } else {
      if (p->sample_ws) (void)hipFree(p->sample_ws);
      p->sample_ws = nullptr;  // the one-workgroup sampler needs no workspace
    }
  }
  // LM-head chunk maxima ([Mpad][V / 16])
  if (desc->V % 64 == 0 && desc->Mpad > 0) {
    if (hipMalloc(&p->cmax, (size_t)desc->Mpad * (desc->V / 16) * sizeof(float)) != hipSuccess) p->cmax = nullptr;
  }
  return p;
}

CAIN_API void cain_plan_destroy(void* plan) { delete static_cast<Plan*>(plan); }

CAIN_API void cain_w4a8_set_min_rows(int m) { g_w4a8_min_rows = m > 16 ? m : 16; }

CAIN_API const char* cain_plan_last_failure() { return g_fail; }

// Enqueue one step on `st`: 0, -1 for what step_ok refuses (nothing launched), else the first failing launch's code
// (cain_plan_last_failure names it).
CAIN_API int cain_step_run(const CainStep* s, hipStream_t st) {
  g_fail[0] = 0;
  if (!step_ok(s, false, 1)) return -1;
  return run_step(*s, st);
}

// Record `steps` such steps on `st` (one stream: no parallel branch) into a graph; returns the executable graph, or
// null with *err set (-1 for what step_ok refuses).
CAIN_API void* cain_step_capture(const CainStep* s, int steps, hipStream_t st, int* err) {
  *err = 0;
  if (!step_ok(s, true, steps)) {
    *err = -1;
    return nullptr;
  }
  return capture_steps(st, steps, err, [&] { return run_step(*s, st); });
}

CAIN_API int cain_graph_launch(void* exec, hipStream_t st) {
  return int(hipGraphLaunch(static_cast<hipGraphExec_t>(exec), st));
}

CAIN_API void cain_graph_destroy(void* exec) {
  if (exec) (void)hipGraphExecDestroy(static_cast<hipGraphExec_t>(exec));
}

// ---- CU-limited streams: the batch-1 energy lever (tools/cu_sweep.py).  A stream whose hardware queue may use only
// n of the device's CUs (hipExtStreamCreateWithCUMask), chosen as whole groups of 8 consecutive mask bits spaced
// evenly over the mask: balanced over the 8 XCDs whether the mask's CU numbering interleaves the XCDs or runs
// through them one after the other (n a multiple of 64 balances exactly under both).  Kernels captured or launched
// for such a stream size their grids by cain_cu_budget().
static int g_cu_budget = 0;

static int device_cus() {
  static const int n = [] {
    int dev = 0, c = 0;
    (void)hipGetDevice(&dev);
    return hipDeviceGetAttribute(&c, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && c > 0 ? c : 256;
  }();
  return n;
}

CAIN_API int cain_cu_budget() {
  const int n = device_cus();
  return g_cu_budget > 0 && g_cu_budget < n ? g_cu_budget : n;
}

CAIN_API void cain_set_cu_budget(int n) { g_cu_budget = n > 0 ? n : 0; }
CAIN_API int cain_get_cu_budget() { return cain_cu_budget(); }

// The mask itself (host-side; tests): n_cu of total bits set, or -1.
CAIN_API int cain_cu_mask(int n_cu, int total, uint32_t* mask, int words) {
  if (total <= 0 || total % 8 || n_cu <= 0 || n_cu > total || n_cu % 8 || words * 32 < total) return -1;
  for (int i = 0; i < words; ++i) mask[i] = 0;
  const int groups = total / 8, take = n_cu / 8;
  for (int j = 0; j < take; ++j) {
    const int g = (int)((long long)j * groups / take);
    for (int b = 0; b < 8; ++b) mask[(g * 8 + b) / 32] |= 1u << ((g * 8 + b) % 32);
  }
  return 0;
}

CAIN_API void* cain_stream_create_cu_limited(int n_cu) {
  const int total = device_cus();
  std::vector<uint32_t> mask((total + 31) / 32);
  if (cain_cu_mask(n_cu, total, mask.data(), (int)mask.size()) != 0) return nullptr;
  hipStream_t st = nullptr;
  if (hipExtStreamCreateWithCUMask(&st, (uint32_t)mask.size(), mask.data()) != hipSuccess) return nullptr;
  return st;
}

CAIN_API int cain_stream_destroy(void* st) { return hipStreamDestroy(static_cast<hipStream_t>(st)) == hipSuccess ? 0 : -1; }

CAIN_API int cain_step_size() { return int(sizeof(CainStep)); }
CAIN_API int cain_rows_size() { return int(sizeof(CainRows)); }
CAIN_API int cain_logprob_size() { return int(sizeof(CainLogprob)); }
CAIN_API int cain_grammar_size() { return int(sizeof(CainGrammar)); }
CAIN_API int cain_stop_size() { return int(sizeof(CainStop)); }
CAIN_API int cain_plan_desc_size() { return int(sizeof(CainPlanDesc)); }
CAIN_API int cain_layer_size() { return int(sizeof(CainLayer)); }

}  // extern "C"
