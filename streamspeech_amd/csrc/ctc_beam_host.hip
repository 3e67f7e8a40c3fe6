// The plain-C++ twin of the CTC prefix beam search (ctc_beam.hip): ss_ctc_beam_host, ss_ctc_beam_lm_host and the resumable
// ctc_stream_host_run (the object and its entry points: ctc_stream.hip).  The frame is ctc_beam.hpp's -- the functions the kernel
// body calls, on the kernel's layout (CtcBeamHostState) -- so what is written here is what belongs to a side: the candidates of a
// row, the serial loops with the rank count's early exit, the slot writes of the next beam, and the records.  Three steps over one
// utterance's state (start, frames, emit) serve the one-shot and the resumable twin.  FORM (CTC_FORM_*) without the LM bit: lv / lw
// / ws unused; without the bias bit: bv / bs unused; 0: records ss_ctc_beam_hyp.  No kernel and no HIP call:
// tools/ctc_beam_host_check.cpp runs it under a sanitizer.
#include "ctc_beam.hpp"

#include <algorithm>
#include <cstring>

#include "ctc_bias.hpp"
#include "ngram_lm.hpp"

#include "../../include/streamspeech_hip.h"
#include "ctc_row.hpp"
#include "elementwise.hpp"

namespace ss {

namespace {

constexpr int NONE = 0x7fffffff;

int g_host_max_beam = CTC_BEAM_MAX_BEAM;      // ss_debug_ctc_beam_host_max: the host twin's cap alone (the exhaustive test)

// ctc_beam_cand_kernel's candidates: the k-th column in the order (logit descending, id ascending) among the unmasked non-blank ones.
void row_cand_host(const float* r, int N, int pad, int unk, int C, int* out) {
  float lv = INFINITY;
  int li = -1;
  for (int k = 0; k < C; ++k) {
    float bv = -INFINITY;
    int bi = NONE;
    for (int n = 1; n < N; ++n) {
      const float x = r[n];
      if (n == pad || n == unk || !(x > -INFINITY) || !(x < lv || (x == lv && n > li))) continue;
      if (bi == NONE || x > bv) { bv = x; bi = n; }
    }
    out[k] = bi == NONE ? -1 : bi;
    lv = bi == NONE ? -INFINITY : bv;
    li = bi;
  }
}

}  // namespace

// What an LM call, on the device or here, is refused for past the plain refusals, before anything is launched or written.
int ctc_beam_lm_check(const ss_ngram_lm* lm, int V, const ss_ctc_lm_opts* o) {
  if (!lm || !o || lm->host.V != V || !std::isfinite(o->lm_weight) || !std::isfinite(o->word_score)) return SS_ERR_ARG;
  if (o->eos_term && lm->host.eos < 0) return SS_ERR_ARG;
  return SS_OK;
}

// What a bias call, on the device or here, is refused for past the plain refusals and the model's: no set or no options, a set made
// for another vocabulary, pad or unk, a non-finite scale, a model without options or options without a model.
int ctc_beam_bias_check(const ss_ctc_bias* bias, int V, int pad, int unk, const ss_ctc_bias_opts* bo, const ss_ngram_lm* lm,
                        const ss_ctc_lm_opts* o) {
  if (!bias || !bo || bias->host.V != V || bias->host.pad != pad || bias->host.unk != unk || !std::isfinite(bo->scale)) return SS_ERR_ARG;
  if ((lm == nullptr) != (o == nullptr)) return SS_ERR_ARG;
  return SS_OK;
}

void CtcBeamHostState::start(int beam_, int max_T, int form, int lm_start) {
  const bool lm = (form & CTC_FORM_LM) != 0;
  const long long slots = ctc_stream_slots(beam_, max_T);
  const size_t n_nodes = (size_t)ctc_stream_nodes(beam_, max_T);
  mask = (int)(slots - 1);
  keys.assign((size_t)slots, CTC_BEAM_EMPTY);
  vals.assign((size_t)slots, -1);
  nodes.assign(n_nodes, make_int2(-1, -1));
  if (lm) { n_sum.assign(n_nodes, 0.0); n_bonus.assign(n_nodes, 0.0); n_state.assign(n_nodes, 0); n_state[0] = lm_start; }
  if (form & CTC_FORM_BIAS) { n_bonus.assign(n_nodes, 0.0); n_bsum.assign(n_nodes, 0.0); n_bstate.assign(n_nodes, 0); }
  beam = beam_;
  for (std::vector<double>* b : {&b_pb, &b_pnb, &b_tot, &b_bonus}) b->assign(2 * (size_t)beam, 0.0);
  b_node.assign(2 * (size_t)beam, -1); b_last.assign(2 * (size_t)beam, -1);
  b_pnb[0] = -INFINITY; b_node[0] = 0;                         // the root: pb = tot = bonus = 0, no last label
  cur = 0; alive = 1; frames = 0; bad = false;
}

// The frames S.frames .. S.frames + n - 1 from the n rows at `rows`; h_den [n][2] / h_cand [n][C] (may be NULL) receive the
// candidate kernel's values of every one of them, whatever the search makes of it.
template <int FORM>
static void ctc_beam_host_frames(CtcBeamHostState& S, const float* rows, int ld, int V, int pad, int unk, int n, int C,
                                 const NgramView& lv, double lw, double ws, const BiasView& bv, double bs, float* h_den,
                                 int32_t* h_cand_id) {
  constexpr bool LM = FORM != 0;                               // (what follows asks whether the order has a fused key)
  const int W = C + 1, beam = S.beam;
  std::vector<int> cid_all((size_t)n * C);
  std::vector<float> den_all(2 * (size_t)n);
  for (int i = 0; i < n; ++i) {                                // the candidate kernel: every row, whatever the search makes of it
    const float* r = rows + (size_t)i * ld;
    float* den = &den_all[2 * (size_t)i];
    if (ctc_row_den_host(r, V, &den[0], &den[1])) den[0] = den[1] = __builtin_nanf("");
    row_cand_host(r, V, pad, unk, C, &cid_all[(size_t)i * C]);
  }
  if (h_den && n > 0) memcpy(h_den, den_all.data(), den_all.size() * sizeof(float));
  if (h_cand_id && n > 0) memcpy(h_cand_id, cid_all.data(), cid_all.size() * sizeof(int));
  std::vector<double> s_pb(beam), s_pnb(beam), s_give(beam), e_tot((size_t)beam * W), e_fus(LM ? (size_t)beam * W : 1);
  std::vector<int> e_node((size_t)beam * W), s_c(C);
  std::vector<float> s_lpc(C), s_lpl(beam);
  float s_lp0 = 0.f;
  const CtcBeamFrame F{S.b_pb.data(), S.b_pnb.data(), S.b_tot.data(), S.b_bonus.data(), S.b_node.data(), S.b_last.data(),
                       s_pb.data(), s_pnb.data(), s_give.data(), e_tot.data(), e_fus.data(), e_node.data(),
                       s_c.data(), s_lpc.data(), s_lpl.data(), &s_lp0, S.keys.data(), S.vals.data(), S.mask,
                       S.n_bonus.data(), S.n_state.data(), S.n_bstate.data()};
  const int f0 = S.frames;
  S.frames += n;
  for (int t = f0; t < f0 + n && !S.bad; ++t) {
    const float* r = rows + (size_t)(t - f0) * ld;
    const float mx = den_all[2 * (size_t)(t - f0)], ls = den_all[2 * (size_t)(t - f0) + 1];
    if (ls != ls) { S.bad = true; break; }
    const int co = S.cur * beam, no = (S.cur ^ 1) * beam, nb = S.alive, n_ent = nb * W;
    for (int k = 0; k < C; ++k) {                              // A
      const int c = cid_all[(size_t)(t - f0) * C + k];
      s_c[k] = c;
      s_lpc[k] = c >= 0 ? ctc_beam_lp(r[c], mx, ls) : -INFINITY;
    }
    for (int i = 0; i < nb; ++i) {
      const int last = F.b_last[co + i];
      s_lpl[i] = last >= 0 ? ctc_beam_lp(r[last], mx, ls) : -INFINITY;
      s_give[i] = -INFINITY;
    }
    s_lp0 = ctc_beam_lp(r[0], mx, ls);
    for (int e = 0; e < n_ent; ++e) ctc_beam_entry_b<FORM>(F, co, nb, W, e, lv, lw, ws, bv, bs);   // B
    for (int i = 0; i < nb; ++i) ctc_beam_entry_c<FORM>(F, co, W, i);                              // C
    const double* e_key = LM ? F.e_fus : F.e_tot;              // what the order compares
    int alive = 0;
    for (int e = 0; e < n_ent; ++e) {                          // D
      const double key = e_key[e];
      if (!(key > -INFINITY)) continue;
      int rank = 0;
      for (int f = 0; f < n_ent && rank < beam; ++f) rank += ctc_beam_before(e_key[f], f, key, e);
      if (rank >= beam) continue;
      const double tot = F.e_tot[e];                           // the state keeps the pure CTC total
      const int i = e / W, k = e - i * W - 1;
      int node = F.e_node[e];
      if (k < 0) {
        F.b_pb[no + rank] = s_pb[i]; F.b_pnb[no + rank] = s_pnb[i]; F.b_last[no + rank] = F.b_last[co + i];
        F.b_bonus[no + rank] = F.b_bonus[co + i];
      } else {
        const int c = s_c[k];
        if (node < 0)
          node = ctc_beam_make_node<FORM>(t, beam, rank, F.b_node[co + i], c, F.b_bonus[co + i], F.keys, F.vals, F.mask,
                                          S.nodes.data(), S.n_sum.data(), S.n_bonus.data(), S.n_state.data(), lv, lw, ws,
                                          S.n_bsum.data(), S.n_bstate.data(), bv, bs);
        F.b_pb[no + rank] = -INFINITY; F.b_pnb[no + rank] = tot; F.b_last[no + rank] = c;
        F.b_bonus[no + rank] = LM ? S.n_bonus[node] : 0.0;
      }
      F.b_tot[no + rank] = tot; F.b_node[no + rank] = node;
      if (rank + 1 > alive) alive = rank + 1;                  // ranks are 0 .. alive - 1 without a gap
    }
    S.alive = alive;
    S.cur ^= 1;
  }
}

// The n-best of the beam as it stands: h_hyps_b [nbest] records and h_tokens_b [nbest][out_stride] of this utterance.  eos: the LM
// form's eos term; finish: the bias forms' finish term.
template <int FORM>
static void ctc_beam_host_emit(const CtcBeamHostState& S, int nbest, bool eos, const NgramView& lv, double lw, bool finish,
                               const BiasView& bv, double bs, void* h_hyps_b, int32_t* h_tokens_b, int out_stride) {
  constexpr bool LM = FORM != 0, HAS_LM = (FORM & CTC_FORM_LM) != 0, BIAS = (FORM & CTC_FORM_BIAS) != 0;
  const bool bad = S.bad;
  const int co = S.cur * S.beam, nb = bad ? 0 : S.alive;
  const double nothing = bad ? (double)__builtin_nanf("") : -INFINITY;
  typedef typename std::conditional<BIAS, ss_ctc_beam_bias_hyp,
                                    typename std::conditional<LM, ss_ctc_beam_lm_hyp, ss_ctc_beam_hyp>::type>::type Hyp;
  Hyp* h_hyps = static_cast<Hyp*>(h_hyps_b);
  std::vector<double> fin(nb), lms(nb, 0.0), bss(nb, 0.0);     // the plain form: fin = tot, the beam's own order
  for (int r = 0; r < nb; ++r) {
    [[maybe_unused]] const int node = S.b_node[co + r];
    fin[r] = S.b_tot[co + r];
    if constexpr (HAS_LM)
      ctc_beam_finish(S.b_tot[co + r], S.b_bonus[co + r], S.n_sum[node], S.n_state[node], eos ? lv.eos : -1, lv, lw, &fin[r], &lms[r]);
    else if constexpr (BIAS)
      fin[r] = S.b_tot[co + r] + S.b_bonus[co + r];
    if constexpr (BIAS) ctc_beam_bias_finish(bv, S.n_bstate[node], S.n_bsum[node], bs, finish, &fin[r], &bss[r]);
  }
  for (int k = nb; k < nbest; ++k) {                           // the empty slots
    Hyp& h = h_hyps[k];
    h.score = nothing; h.n_tokens = 0; h.status = bad ? 2 : 1;
    if constexpr (LM) { h.ctc_score = nothing; h.lm_score = 0.0; }
    if constexpr (BIAS) h.bias_score = 0.0;
  }
  for (int r = 0; r < nb; ++r) {
    int rank = LM ? 0 : r;
    if constexpr (LM)
      for (int f = 0; f < nb; ++f) rank += ctc_beam_before(fin[f], f, fin[r], r);
    if (rank >= nbest) continue;
    Hyp& h = h_hyps[rank];
    h.n_tokens = ctc_beam_trace(S.nodes.data(), S.b_node[co + r], h_tokens_b + (size_t)rank * out_stride);
    h.score = fin[r]; h.status = 0;
    if constexpr (LM) { h.ctc_score = S.b_tot[co + r]; h.lm_score = lms[r]; }
    if constexpr (BIAS) h.bias_score = bss[r];
  }
}

// The stable-prefix pass of the resumable kernel: the smallest depth of the lowest common ancestor of a beam prefix and prefix 0.
static CtcStreamPart ctc_beam_host_part(const CtcBeamHostState& S) {
  const int co = S.cur * S.beam, nb = S.bad ? 0 : S.alive;
  int stable = nb > 0 ? NONE : 0;
  for (int r = 0; r < nb; ++r) stable = std::min(stable, ctc_beam_lca_depth(S.nodes.data(), S.b_node[co + r], S.b_node[co]));
  return CtcStreamPart{S.frames, stable, nb, S.bad ? 2 : 0};
}

// The resumable twin: every pointer a HOST pointer, h_logits the stacked new rows (session i's upto - f rows behind those of the
// sessions before it).  The checks are the caller's (ss_ctc_stream_advance_host, ctc_stream.hip).
int ctc_stream_host_run(std::vector<CtcBeamHostState>& slots, const float* h_logits, int ld, int V, int pad, int unk, int n,
                        const CtcStreamSess* sess, int beam, int cand, int nbest, const ss_ngram_lm* lm, const ss_ctc_lm_opts* o,
                        void* h_hyps, int32_t* h_tokens, int out_stride, CtcStreamPart* h_part, const ss_ctc_bias* bias,
                        const ss_ctc_bias_opts* bo) {
  NgramView lv{};
  BiasView bv{};
  double lw = 0.0, ws = 0.0, bs = 0.0;
  if (lm) { lv = lm->host.view(); lw = o->lm_weight; ws = o->word_score; }
  if (bias) { bv = bias->host.view(); bs = bo->scale; }
  const size_t rec = bias ? sizeof(ss_ctc_beam_bias_hyp) : lm ? sizeof(ss_ctc_beam_lm_hyp) : sizeof(ss_ctc_beam_hyp);
  for (int i = 0; i < n; ++i) {
    const CtcStreamSess& se = sess[i];
    CtcBeamHostState& S = slots[se.slot];
    const float* rows = h_logits + (size_t)se.row0 * ld;
    unsigned char* hy = static_cast<unsigned char*>(h_hyps) + (size_t)i * nbest * rec;
    int32_t* tk = h_tokens + (size_t)i * nbest * out_stride;
    const auto run = [&](auto form) {
      ctc_beam_host_frames<decltype(form)::value>(S, rows, ld, V, pad, unk, se.upto - se.f, cand, lv, lw, ws, bv, bs, nullptr, nullptr);
      ctc_beam_host_emit<decltype(form)::value>(S, nbest, lm && se.fin && o->eos_term, lv, lw, bias && se.fin && bo->finish, bv, bs,
                                                hy, tk, out_stride);
    };
    if (bias) lm ? run(std::integral_constant<int, CTC_FORM_LM | CTC_FORM_BIAS>{}) : run(std::integral_constant<int, CTC_FORM_BIAS>{});
    else lm ? run(std::integral_constant<int, CTC_FORM_LM>{}) : run(std::integral_constant<int, 0>{});
    h_part[i] = ctc_beam_host_part(S);
  }
  return SS_OK;
}

}  // namespace ss

using namespace ss;

extern "C" int ss_debug_ctc_beam_host_max(int max_beam) {
  const int was = g_host_max_beam;
  if (max_beam >= 1) g_host_max_beam = max_beam;
  return was;
}

template <int FORM>
static int ctc_beam_host_any(const float* h_logits, int ld, int V, int pad, int unk, int B, const int32_t* h_T, int beam, int cand,
                             int nbest, const ss_ngram_lm* lm, const ss_ctc_lm_opts* o, void* h_hyps_out, int32_t* h_tokens,
                             int out_stride, float* h_den, int32_t* h_cand_id, const ss_ctc_bias* bias = nullptr,
                             const ss_ctc_bias_opts* bo = nullptr) {
  constexpr bool LM = (FORM & CTC_FORM_LM) != 0, BIAS = (FORM & CTC_FORM_BIAS) != 0;
  if (!h_logits || ld < V || !h_hyps_out || !h_tokens) return SS_ERR_ARG;
  CtcBeamPlan p;
  RET(ctc_beam_plan(V, B, h_T, beam, cand, nbest, out_stride, p, g_host_max_beam));
  NgramView lv{};
  BiasView bv{};
  double lw = 0.0, ws = 0.0, bs = 0.0;
  if constexpr (BIAS) {
    RET(ctc_beam_bias_check(bias, V, pad, unk, bo, lm, o));
    bv = bias->host.view(); bs = bo->scale;
  }
  if constexpr (LM) {
    RET(ctc_beam_lm_check(lm, V, o));
    lv = lm->host.view(); lw = o->lm_weight; ws = o->word_score;
  }
  const size_t rec = BIAS ? sizeof(ss_ctc_beam_bias_hyp) : LM ? sizeof(ss_ctc_beam_lm_hyp) : sizeof(ss_ctc_beam_hyp);
  CtcBeamHostState S;
  for (int b = 0; b < B; ++b) {
    const CtcBeamSeg& sg = p.segs[b];
    S.start(beam, sg.T, FORM, lv.start);
    ctc_beam_host_frames<FORM>(S, h_logits + (size_t)sg.row0 * ld, ld, V, pad, unk, sg.T, cand, lv, lw, ws, bv, bs,
                               h_den ? h_den + 2 * (size_t)sg.row0 : nullptr, h_cand_id ? h_cand_id + (size_t)sg.row0 * cand : nullptr);
    ctc_beam_host_emit<FORM>(S, nbest, LM && o->eos_term, lv, lw, BIAS && bo->finish, bv, bs,
                             static_cast<unsigned char*>(h_hyps_out) + (size_t)b * nbest * rec,
                             h_tokens + (size_t)b * nbest * out_stride, out_stride);
  }
  return SS_OK;
}

extern "C" int ss_ctc_beam_host(const float* h_logits, int ld, int V, int pad, int unk, int B, const int32_t* h_T, int beam, int cand,
                                int nbest, ss_ctc_beam_hyp* h_hyps, int32_t* h_tokens, int out_stride, float* h_den,
                                int32_t* h_cand_id) {
  return ctc_beam_host_any<0>(h_logits, ld, V, pad, unk, B, h_T, beam, cand, nbest, nullptr, nullptr, h_hyps, h_tokens, out_stride,
                                  h_den, h_cand_id);
}

extern "C" int ss_ctc_beam_lm_host(const float* h_logits, int ld, int V, int pad, int unk, int B, const int32_t* h_T, int beam, int cand,
                                   int nbest, ss_ctc_beam_lm_hyp* h_hyps, int32_t* h_tokens, int out_stride, float* h_den,
                                   int32_t* h_cand_id, const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts) {
  return ctc_beam_host_any<CTC_FORM_LM>(h_logits, ld, V, pad, unk, B, h_T, beam, cand, nbest, lm, opts, h_hyps, h_tokens, out_stride,
                                        h_den, h_cand_id);
}

extern "C" int ss_ctc_beam_bias_host(const float* h_logits, int ld, int V, int pad, int unk, int B, const int32_t* h_T, int beam,
                                     int cand, int nbest, ss_ctc_beam_bias_hyp* h_hyps, int32_t* h_tokens, int out_stride, float* h_den,
                                     int32_t* h_cand_id, const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts, const ss_ctc_bias* bias,
                                     const ss_ctc_bias_opts* bias_opts) {
  if (lm)
    return ctc_beam_host_any<CTC_FORM_LM | CTC_FORM_BIAS>(h_logits, ld, V, pad, unk, B, h_T, beam, cand, nbest, lm, opts, h_hyps, h_tokens,
                                                          out_stride, h_den, h_cand_id, bias, bias_opts);
  return ctc_beam_host_any<CTC_FORM_BIAS>(h_logits, ld, V, pad, unk, B, h_T, beam, cand, nbest, lm, opts, h_hyps, h_tokens, out_stride,
                                          h_den, h_cand_id, bias, bias_opts);
}
