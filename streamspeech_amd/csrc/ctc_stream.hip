// The resumable CTC prefix beam search (ss_ctc_stream_*): the object that keeps every slot's search between launches, its refusals,
// and the three ways to move it -- on a model's encoder rows (ss_ctc_stream_advance: the rows a slot has not consumed are stacked,
// go through the head under the batch call's pack-invariance setting, then the candidate kernel and one launch of the resumable
// search kernel), on the caller's device logits (ss_op_ctc_stream_advance) and in plain C++ (ss_ctc_stream_advance_host).  The
// kernel is ctc_beam.hip's, the twin ctc_beam_host.hip's, and the frame both run is ctc_beam.hpp's: there is one statement of a frame.
#include "model_internal.hpp"
#include "ctc_beam.hpp"
#include "ctc_bias.hpp"
#include "ngram_lm.hpp"

int launch_pool_stack_rows(float* out, const float* enc, int W, const int* src, const int* pre, int nsess, int total,
                           hipStream_t s);   // stream_pool.hip

struct ss_ctc_stream {
  int V = 0, pad = -1, unk = -1, head = -1;
  int S = 0, max_frames = 0, beam = 0, cand = 0, nbest = 0;
  const ss_ngram_lm* lm = nullptr;
  ss_ctc_lm_opts opts{};
  const ss_ctc_bias* bias = nullptr; // a hotword set (ss_ctc_stream_create_bias): the bias forms, records ss_ctc_beam_bias_hyp
  ss_ctc_bias_opts bopts{};
  ss_scratch* sc = nullptr;          // the set the state is booked on (ss_ctc_stream_create), else null
  bool on_device = false;
  DevBuf buf;                        // the slots' state, ctc_stream_carve'd into dev
  CtcStreamDev dev{};
  CtcStreamBiasDev bdev{nullptr, nullptr};
  int form() const { return (lm ? CTC_FORM_LM : 0) | (bias ? CTC_FORM_BIAS : 0); }
  std::vector<CtcBeamHostState> host;   // ... or the twin's, one per slot
  std::vector<int> frames;           // frames consumed per slot
  std::vector<char> dirty;           // the slot's child table holds an earlier utterance's keys (or nothing yet): cleared at its next advance
};

namespace {

int stream_make(int V, int pad, int unk, int max_sessions, int max_frames, int beam, int cand, int nbest, const ss_ngram_lm* lm,
                const ss_ctc_lm_opts* opts, ss_ctc_stream** out, bool with_bias = false, const ss_ctc_bias* bias = nullptr,
                const ss_ctc_bias_opts* bopts = nullptr) {
  if (!out) return SS_ERR_ARG;
  *out = nullptr;
  if (max_sessions <= 0 || max_sessions > (1 << 16) || max_frames < 1 || max_frames > CTC_BEAM_MAX_T || (lm == nullptr) != (opts == nullptr))
    return SS_ERR_ARG;
  CtcBeamPlan plan;                  // the limits of the one-shot calls, on one utterance of max_frames
  const int32_t T1 = max_frames;
  RET(ctc_beam_plan(V, 1, &T1, beam, cand, nbest, max_frames, plan));
  if (with_bias) RET(ctc_beam_bias_check(bias, V, pad, unk, bopts, lm, opts));
  if (lm) RET(ctc_beam_lm_check(lm, V, opts));
  ss_ctc_stream* cs = new ss_ctc_stream();
  if (with_bias) { cs->bias = bias; cs->bopts = *bopts; }
  cs->V = V; cs->pad = pad; cs->unk = unk;
  cs->S = max_sessions; cs->max_frames = max_frames; cs->beam = beam; cs->cand = cand; cs->nbest = nbest;
  cs->lm = lm;
  if (opts) cs->opts = *opts;
  cs->frames.assign(max_sessions, 0);
  cs->dirty.assign(max_sessions, 1);
  *out = cs;
  return SS_OK;
}

int stream_alloc_device(ss_ctc_stream* cs) {
  RET(cs->buf.ensure((size_t)cs->S * ctc_stream_slot_bytes(cs->beam, cs->max_frames, cs->form()), true));
  ctc_stream_carve(cs->buf.p, cs->S, cs->beam, cs->max_frames, cs->form(), &cs->dev, &cs->bdev);
  cs->on_device = true;
  return SS_OK;
}

// Every refusal of an advance past its pointers; fills the sessions and the number of stacked new rows.  h_T may be NULL (the twins).
int stream_check(const ss_ctc_stream* cs, int n, const int32_t* h_slots, const int32_t* h_T, const int32_t* h_upto,
                 const int32_t* h_final, int out_stride, std::vector<CtcStreamSess>& sess, int* rows) {
  if (n <= 0 || n > cs->S) return SS_ERR_ARG;
  std::vector<char> seen(cs->S, 0);
  sess.resize(n);
  int total = 0;
  for (int i = 0; i < n; ++i) {
    const int sl = h_slots[i];
    if (sl < 0 || sl >= cs->S || seen[sl]) return SS_ERR_ARG;
    seen[sl] = 1;
    const int f = cs->frames[sl], upto = h_upto[i];
    if (upto < f || (h_T && upto > h_T[i]) || upto > cs->max_frames || out_stride < upto) return SS_ERR_ARG;
    sess[i] = CtcStreamSess{sl, total, f, upto, h_final[i] != 0, 0};
    total += upto - f;
  }
  *rows = total;
  return SS_OK;
}

// The call went through: the slots have consumed their frames; an utterance's last call resets its slot.
void stream_commit(ss_ctc_stream* cs, const std::vector<CtcStreamSess>& sess) {
  for (const CtcStreamSess& se : sess) {
    cs->frames[se.slot] = se.fin ? 0 : se.upto;
    if (se.fin && se.upto > 0) cs->dirty[se.slot] = 1;
  }
}

// The child tables of the call's slots that still hold an earlier utterance: filled with 0xff on the call's stream.
int stream_clear_device(ss_ctc_stream* cs, const std::vector<CtcStreamSess>& sess, hipStream_t s) {
  for (const CtcStreamSess& se : sess) {
    if (!cs->dirty[se.slot]) continue;
    SS_HIP_CHECK(hipMemsetAsync(cs->dev.keys + (size_t)se.slot * cs->dev.slots_per, 0xff, (size_t)cs->dev.slots_per * 8, s));
    cs->dirty[se.slot] = 0;
  }
  return SS_OK;
}

}  // namespace

static int stream_create(ss_model* m, int head, int max_sessions, int max_frames, int beam, int cand, int nbest, const ss_ngram_lm* lm,
                         const ss_ctc_lm_opts* opts, bool with_bias, const ss_ctc_bias* bias, const ss_ctc_bias_opts* bopts,
                         ss_ctc_stream** out) {
  if (!out) return SS_ERR_ARG;
  *out = nullptr;
  if (!m || head < 0 || head > 1 || (m->cfg.enc_dim & 3) != 0 || m->cfg.enc_dim > 1024) return SS_ERR_ARG;
  const ss_config& c = m->cfg;
  ss_ctc_stream* cs = nullptr;
  RET(stream_make(head == 0 ? c.src_vocab : c.tgt_vocab, c.pad, c.unk, max_sessions, max_frames, beam, cand, nbest, lm, opts, &cs,
                  with_bias, bias, bopts));
  cs->head = head;
  cs->buf.acct = &m->sc->acct;
  const int rc = stream_alloc_device(cs);   // exact size; refused on the cap (or the device): the set is left as it was
  if (rc != SS_OK) { delete cs; return rc; }
  cs->sc = m->sc;
  cs->sc->extra.push_back(&cs->buf);
  cs->sc->refs.fetch_add(1);                // the set lives as long as an object booked in it
  *out = cs;
  return SS_OK;
}

extern "C" int ss_ctc_stream_create(ss_model* m, int head, int max_sessions, int max_frames, int beam, int cand, int nbest,
                                    const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts, ss_ctc_stream** out) {
  return stream_create(m, head, max_sessions, max_frames, beam, cand, nbest, lm, opts, false, nullptr, nullptr, out);
}

extern "C" int ss_ctc_stream_create_bias(ss_model* m, int head, int max_sessions, int max_frames, int beam, int cand, int nbest,
                                         const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts, const ss_ctc_bias* bias,
                                         const ss_ctc_bias_opts* bias_opts, ss_ctc_stream** out) {
  return stream_create(m, head, max_sessions, max_frames, beam, cand, nbest, lm, opts, true, bias, bias_opts, out);
}

static int debug_stream_create(int V, int pad, int unk, int on_device, int max_sessions, int max_frames, int beam, int cand, int nbest,
                               const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts, bool with_bias, const ss_ctc_bias* bias,
                               const ss_ctc_bias_opts* bopts, ss_ctc_stream** out) {
  ss_ctc_stream* cs = nullptr;
  if (!out) return SS_ERR_ARG;
  *out = nullptr;
  RET(stream_make(V, pad, unk, max_sessions, max_frames, beam, cand, nbest, lm, opts, &cs, with_bias, bias, bopts));
  if (on_device) {
    const int rc = stream_alloc_device(cs);
    if (rc != SS_OK) { delete cs; return rc; }
  } else {
    cs->host.resize(max_sessions);
  }
  *out = cs;
  return SS_OK;
}

extern "C" int ss_debug_ctc_stream_create(int V, int pad, int unk, int on_device, int max_sessions, int max_frames, int beam, int cand,
                                          int nbest, const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts, ss_ctc_stream** out) {
  return debug_stream_create(V, pad, unk, on_device, max_sessions, max_frames, beam, cand, nbest, lm, opts, false, nullptr, nullptr, out);
}

extern "C" int ss_debug_ctc_stream_create_bias(int V, int pad, int unk, int on_device, int max_sessions, int max_frames, int beam,
                                               int cand, int nbest, const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts,
                                               const ss_ctc_bias* bias, const ss_ctc_bias_opts* bias_opts, ss_ctc_stream** out) {
  return debug_stream_create(V, pad, unk, on_device, max_sessions, max_frames, beam, cand, nbest, lm, opts, true, bias, bias_opts, out);
}

extern "C" void ss_ctc_stream_destroy(ss_ctc_stream* cs) {
  if (!cs) return;
  cs->buf.release();                        // (hipFree waits for whatever still reads or writes the slots)
  if (cs->sc) {
    auto& ex = cs->sc->extra;
    ex.erase(std::remove(ex.begin(), ex.end(), &cs->buf), ex.end());
    scratch_unref(cs->sc);
  }
  delete cs;
}

extern "C" int ss_ctc_stream_reset(ss_ctc_stream* cs, int slot) {
  if (!cs || slot < 0 || slot >= cs->S) return SS_ERR_ARG;
  if (cs->frames[slot] > 0) cs->dirty[slot] = 1;
  cs->frames[slot] = 0;
  return SS_OK;
}

extern "C" int ss_ctc_stream_advance(ss_model* m, void* stream, ss_ctc_stream* cs, int n, const int32_t* h_slots,
                                     const float* d_enc_packed, const int32_t* h_T, const int32_t* h_upto, const int32_t* h_final,
                                     void* d_hyps, int32_t* d_tokens, int out_stride, ss_ctc_stream_part* d_part) {
  if (!m || !cs || !cs->sc || cs->sc != m->sc || !h_slots || !d_enc_packed || !h_T || !h_upto || !h_final || !d_hyps || !d_tokens ||
      !d_part)
    return SS_ERR_ARG;
  const ss_config& c = m->cfg;
  const int d = c.enc_dim, V = cs->V;
  if (V != (cs->head == 0 ? c.src_vocab : c.tgt_vocab)) return SS_ERR_ARG;
  std::vector<CtcStreamSess> sess;
  int rows = 0;
  RET(stream_check(cs, n, h_slots, h_T, h_upto, h_final, out_stride, sess, &rows));
  // the stacking tables: stacked row r of session i (rows pre[i] ..) is packed row src[i] + r - pre[i]
  std::vector<int> ti(2 * (size_t)n + 1);
  int *src = ti.data(), *pre = src + n, total = 0;
  for (int i = 0; i < n; ++i) {
    src[i] = total + sess[i].f;
    pre[i] = sess[i].row0;
    total += h_T[i];
  }
  pre[n] = rows;
  SkScope sk_scope(m->sc->skws);
  CanonScope canon_scope(m->pack_invariant ? CANON_SEQ : CANON_NONE);
  hipStream_t s = (hipStream_t)stream;
  const size_t sess_bytes = (size_t)n * sizeof(CtcStreamSess);
  RET(m->sc->seg_buf.ensure(sess_bytes + ti.size() * sizeof(int)));
  RET(m->sc->mt_ws.ensure((size_t)rows * V * sizeof(float)));
  RET(m->sc->ws.ensure((size_t)rows * ((size_t)d * sizeof(float) + 8 + 4 * (size_t)cs->cand)));
  float* logits = m->sc->mt_ws.f();         // (a call without new rows launches no head; the search kernel reads no row then)
  float* stk = m->sc->ws.f();
  float* den = stk + (size_t)rows * d;
  int* cand_id = reinterpret_cast<int*>(den + 2 * (size_t)rows);
  int* dti = reinterpret_cast<int*>(static_cast<unsigned char*>(m->sc->seg_buf.p) + sess_bytes);
  RET(stream_clear_device(cs, sess, s));
  if (rows > 0) {
    SS_HIP_CHECK(hipMemcpyAsync(dti, ti.data(), ti.size() * sizeof(int), hipMemcpyHostToDevice, s));
    RET(launch_pool_stack_rows(stk, d_enc_packed, d, dti, dti + n, n, rows, s));
    RET(ctc_head_logits(m, s, cs->head, stk, d, rows, false, &logits));
  }
  RET(launch_ctc_stream(logits, V, V, cs->pad, cs->unk, rows, n, sess.data(), m->sc->seg_buf.p, den, cand_id, cs->beam, cs->cand,
                        cs->nbest, cs->dev, cs->lm, cs->lm ? &cs->opts : nullptr, d_hyps, d_tokens, out_stride,
                        reinterpret_cast<CtcStreamPart*>(d_part), s, cs->bias, cs->bias ? &cs->bopts : nullptr, cs->bdev));
  stream_commit(cs, sess);
  return SS_OK;
}

extern "C" int ss_op_ctc_stream_advance(void* stream, ss_ctc_stream* cs, int n, const int32_t* h_slots, const float* d_logits, int ld,
                                        const int32_t* h_upto, const int32_t* h_final, void* d_hyps, int32_t* d_tokens, int out_stride,
                                        ss_ctc_stream_part* d_part) {
  if (!cs || !cs->on_device || cs->sc || !h_slots || !d_logits || ld < cs->V || !h_upto || !h_final || !d_hyps || !d_tokens || !d_part)
    return SS_ERR_ARG;
  std::vector<CtcStreamSess> sess;
  int rows = 0;
  RET(stream_check(cs, n, h_slots, nullptr, h_upto, h_final, out_stride, sess, &rows));
  hipStream_t s = (hipStream_t)stream;
  static thread_local std::map<hipStream_t, DevBuf> tmps;   // scratch as ss_op_ctc_beam's: sessions | den | cand_id
  DevBuf& tmp = tmps[s];
  const size_t sess_bytes = ((size_t)n * sizeof(CtcStreamSess) + 7) & ~(size_t)7;
  RET(tmp.ensure(sess_bytes + (size_t)rows * (8 + 4 * (size_t)cs->cand)));
  float* den = reinterpret_cast<float*>(static_cast<unsigned char*>(tmp.p) + sess_bytes);
  int* cand_id = reinterpret_cast<int*>(den + 2 * (size_t)rows);
  RET(stream_clear_device(cs, sess, s));
  RET(launch_ctc_stream(d_logits, ld, cs->V, cs->pad, cs->unk, rows, n, sess.data(), tmp.p, den, cand_id, cs->beam, cs->cand, cs->nbest,
                        cs->dev, cs->lm, cs->lm ? &cs->opts : nullptr, d_hyps, d_tokens, out_stride,
                        reinterpret_cast<CtcStreamPart*>(d_part), s, cs->bias, cs->bias ? &cs->bopts : nullptr, cs->bdev));
  stream_commit(cs, sess);
  return SS_OK;
}

extern "C" int ss_ctc_stream_advance_host(ss_ctc_stream* cs, int n, const int32_t* h_slots, const float* h_logits, int ld,
                                          const int32_t* h_upto, const int32_t* h_final, void* h_hyps, int32_t* h_tokens,
                                          int out_stride, ss_ctc_stream_part* h_part) {
  if (!cs || cs->on_device || cs->host.empty() || !h_slots || !h_logits || ld < cs->V || !h_upto || !h_final || !h_hyps || !h_tokens ||
      !h_part)
    return SS_ERR_ARG;
  std::vector<CtcStreamSess> sess;
  int rows = 0;
  RET(stream_check(cs, n, h_slots, nullptr, h_upto, h_final, out_stride, sess, &rows));
  for (const CtcStreamSess& se : sess) {
    if (!cs->dirty[se.slot]) continue;
    cs->host[se.slot].start(cs->beam, cs->max_frames, cs->form(), cs->lm ? cs->lm->host.start : 0);
    cs->dirty[se.slot] = 0;
  }
  RET(ctc_stream_host_run(cs->host, h_logits, ld, cs->V, cs->pad, cs->unk, n, sess.data(), cs->beam, cs->cand, cs->nbest, cs->lm,
                          cs->lm ? &cs->opts : nullptr, h_hyps, h_tokens, out_stride, reinterpret_cast<CtcStreamPart*>(h_part), cs->bias,
                          cs->bias ? &cs->bopts : nullptr));
  stream_commit(cs, sess);
  return SS_OK;
}
