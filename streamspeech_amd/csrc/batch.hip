// Ragged-batch twins of the model stages (ss_batch_*): B independent utterances packed along the row axis, no padding anywhere,
// pack-invariant arithmetic (ss_model_set_pack_invariant).  Reference: every stage of agent/speech_to_speech.streamspeech.agent.py
// :425-717 run for B = 1 utterances at a time.
#include <cstring>
#include "model_internal.hpp"
#include "ctc_align.hpp"
#include "ctc_beam.hpp"

// =================================================================================================
// Ragged-batch stage twins: B independent utterances packed along the row axis.  No padding exists
// anywhere -- every utterance keeps the B = 1 arithmetic of the single-utterance entry points
// (SURVEY.md H2b); only launches, weight streaming and tile occupancy are shared.
// =================================================================================================
extern "C" int ss_batch_fbank_cmvn(ss_model* m, void* stream, int B, const float* d_pcm, const int64_t* h_pcm_start,
                                   const int32_t* h_n_samples, float pcm_scale, float* d_feat, int32_t* h_T) {
  if (!m || B <= 0 || !d_pcm || !d_feat || !h_pcm_start || !h_n_samples || !h_T) return SS_ERR_ARG;
  // every refusal first, for the whole call: nothing is written (h_T included) and nothing launched on one.  The kernel's segment
  // fields {pcm_start, n_frames, frame_start} are ints: a start and the pack's row count must fit them.
  int64_t rows = 0;
  for (int b = 0; b < B; ++b) {
    if (h_n_samples[b] < 0 || h_pcm_start[b] < 0 || h_pcm_start[b] > (int64_t)0x7fffffff) return SS_ERR_ARG;
    rows += ss_fbank_num_frames(h_n_samples[b]);
  }
  if (rows > (int64_t)0x7fffffff) return SS_ERR_ARG;
  hipStream_t s = (hipStream_t)stream;
  std::vector<int> segs(3 * (size_t)B);
  int row = 0;
  for (int b = 0; b < B; ++b) {
    const int T = ss_fbank_num_frames(h_n_samples[b]);
    h_T[b] = T;
    segs[3 * (size_t)b] = (int)h_pcm_start[b]; segs[3 * (size_t)b + 1] = T; segs[3 * (size_t)b + 2] = row;
    row += T;
  }
  if (row == 0) return SS_OK;
  RET(m->sc->seg_buf.ensure(segs.size() * sizeof(int)));
  const int* dt = (const int*)m->sc->seg_buf.p;
  RET(upload(s, (int*)m->sc->seg_buf.p, segs));
  // B is the grid's y extent (at most 65535): the table goes out in slices of that many segments, each with its own longest
  // utterance as the x extent.  A segment's fields are offsets into the whole pack, so a slice is the same kernel on a later part
  // of the one uploaded table.
  constexpr int kSlice = 65535;
  for (int b0 = 0; b0 < B; b0 += kSlice) {
    const int nb = std::min(kSlice, B - b0);
    int mx = 0;
    for (int b = b0; b < b0 + nb; ++b) mx = std::max(mx, segs[3 * (size_t)b + 1]);
    RET(launch_fbank_cmvn_batch(d_pcm, pcm_scale, m->fe_window, m->fe_melw, fe_tables(m), m->fe_mean, m->fe_std, d_feat, dt + 3 * (size_t)b0, nb,
                                mx, s));
  }
  return SS_OK;
}

extern "C" int ss_batch_cmvn(ss_model* m, void* stream, const float* d_in, int64_t rows, float* d_out) {
  if (!m || rows < 0 || (rows > 0 && (!d_in || !d_out))) return SS_ERR_ARG;
  return launch_cmvn_rows(d_in, rows, m->fe_mean, m->fe_std, d_out, (hipStream_t)stream);
}

extern "C" int ss_batch_encoder_forward(ss_model* m, void* stream, int B, const float* d_fbank, const int32_t* h_T,
                                        int attn_chunk, int conv_chunk, float* d_enc_out, int32_t* h_Tp) {
  if (!m || B <= 0) return SS_ERR_ARG;
  SkScope sk_scope(m->sc->skws);
  CanonScope canon_scope(m->pack_invariant ? CANON_SEQ : CANON_NONE);
  const bool canon = m->pack_invariant && !debug_tile_forced();
  hipStream_t s = (hipStream_t)stream;
  const ss_config& c = m->cfg;
  const int d = c.enc_dim, f = c.enc_ffn, k = c.conv_kernel, Ld = c.enc_layers * d;
  std::vector<int> T1(B), T2(B);
  for (int b = 0; b < B; ++b) {
    if (h_T[b] <= 0) return SS_ERR_ARG;
    T1[b] = conv_out_len(h_T[b], k, 2); T2[b] = conv_out_len(T1[b], k, 2);
    if (T2[b] <= 0 || T2[b] > c.max_rel_pos) return SS_ERR_CAPACITY;
    h_Tp[b] = T2[b];
  }
  const Offsets o0 = prefix(h_T, B), o1 = prefix(T1.data(), B), o2 = prefix(T2.data(), B);
  const int M1 = o1.total, M2 = o2.total;
  const int cchunk = conv_chunk_cfg(conv_chunk);
  const int achunk = attn_chunk_cfg(attn_chunk);

  // segment tables: conv0 {out,in}, conv1 {out,in}, attention {q,k}, rows {start,len}
  std::vector<int> tab(14 * B);
  int* t0 = tab.data(); int* t1 = t0 + 4 * B; int* ta = t1 + 4 * B; int* tr = ta + 4 * B;
  for (int b = 0; b < B; ++b) {
    t0[4 * b] = o1.off[b]; t0[4 * b + 1] = T1[b]; t0[4 * b + 2] = o0.off[b]; t0[4 * b + 3] = h_T[b];
    t1[4 * b] = o2.off[b]; t1[4 * b + 1] = T2[b]; t1[4 * b + 2] = o1.off[b]; t1[4 * b + 3] = T1[b];
    ta[4 * b] = o2.off[b]; ta[4 * b + 1] = T2[b]; ta[4 * b + 2] = o2.off[b]; ta[4 * b + 3] = T2[b];
    tr[2 * b] = o2.off[b]; tr[2 * b + 1] = T2[b];
  }
  RET(m->sc->seg_buf.ensure(tab.size() * sizeof(int)));
  int* dt = (int*)m->sc->seg_buf.p;
  RET(upload(s, dt, tab));
  const int *d0 = dt, *d1 = dt + 4 * B, *da = dt + 8 * B, *dr = dt + 12 * B;

  const size_t n_h1 = (size_t)M1 * (c.conv_channels / 2), n_x = (size_t)M2 * d, n_f = (size_t)M2 * f,
               n_qkv = (size_t)M2 * 3 * d;
  RET(m->sc->ws.ensure((n_h1 + 3 * n_x + n_f + n_qkv) * sizeof(float)));
  float* h1 = m->sc->ws.f();
  float* x = d_enc_out;
  float* h = h1 + n_h1;
  float* g = h + n_x;
  float* g2 = g + n_x;
  float* ff = g2 + n_x;
  float* qkv = ff + n_f;
  GemmArgs a, b;
  subsampler_args(m, d_fbank, h1, g, a, b);
  a.chunk = cchunk; a.segs = d0; a.nseg = B; a.max_seg_out = o1.mx; a.M = M1; a.in_len = o0.total;
  b.chunk = cchunk; b.segs = d1; b.nseg = B; b.max_seg_out = o2.mx; b.M = M2; b.in_len = M1;
  RET(launch_conv_gemm(a, s));
  RET(launch_conv_gemm(b, s));
  RET(linear(s, g, d, M2, m->enc_linear, d, d, x, d));
  for (int l = 0; l < c.enc_layers; ++l) {
    const EncLayer& e = m->enc[l];
    // the macaron FFNs of packed batches: ONE launch each (ffn.hip), the [rows, 2048] hidden tile stays on chip
    // (pack-invariant contexts: ALWAYS the fused launch in its whole-tile form -- the two-launch form sums the 2048 hidden terms in
    //  another order, and which of the two runs must not depend on the row count)
    const bool fuse_ffn = (canon || (disp().ffn_fusion && M2 >= disp().ffn_min_rows)) && ffn_fused_eligible(d, f, ACT_SILU, M2, d, d, canon) &&
                          e.ffn1_w1.b && e.ffn1_w2.b && e.ffn2_w1.b && e.ffn2_w2.b;
    if (canon && !fuse_ffn) return SS_ERR_ARG;      // never switch FFN forms silently in a pack-invariant context (the two-launch form sums in another order)
    auto attention = [&] {
      AttnArgs at;
      at.Q = qkv; at.K = qkv + d; at.V = qkv + 2 * d; at.ldq = at.ldk = at.ldv = 3 * d;
      at.O = h; at.ldo = d; at.H = c.enc_heads; at.scale = 0.125f; at.chunk = achunk;
      at.P = m->pos_proj + (size_t)l * d; at.ldp = Ld; at.p_tmax = c.max_rel_pos; at.bias_u = e.u; at.bias_v = e.v;
      at.segs = da; at.nseg = B; at.max_q = o2.mx;
      return launch_attention(at, s);
    };
    auto dwconv = [&] {
      return launch_dwconv_bn_silu(g, d, g2, d, e.dw_wt, c.dw_kernel, e.bn_mean, e.bn_var, e.bn_g, e.bn_b, 1e-5f, o2.mx, d, cchunk, s,
                                   dr, B);
    };
    RET(enc_layer_ex(s, c, e, x, M2, h, ff, qkv, g, g2, fuse_ffn, canon, attention, dwconv));
  }
  return SS_OK;
}

// The greedy search of a pack: the {offset, length} table of its utterances, the head, the masked arg-max, the collapse.  d_lprob
// given (with d_last, d_tok_lprob): the same tables, head GEMM and CanonScope, the scored twins of the two glue kernels.
static int batch_ctc_greedy(ss_model* m, void* stream, int head, int B, const float* d_enc_out, const int32_t* h_Tp, int32_t* d_raw,
                            int32_t* d_tokens, int32_t* d_index, int32_t* d_counts, float* d_lprob, int32_t* d_last,
                            float* d_tok_lprob) {
  SkScope sk_scope(m->sc->skws);
  CanonScope canon_scope(m->pack_invariant ? CANON_SEQ : CANON_NONE);
  hipStream_t s = (hipStream_t)stream;
  const ss_config& c = m->cfg;
  const Offsets o = prefix(h_Tp, B);
  const int V = head == 0 ? c.src_vocab : c.tgt_vocab;
  RET(m->sc->mt_ws.ensure((size_t)o.total * V * sizeof(float)));
  std::vector<int> tr(2 * B);
  for (int b = 0; b < B; ++b) { tr[2 * b] = o.off[b]; tr[2 * b + 1] = h_Tp[b]; }
  RET(m->sc->seg_buf.ensure(tr.size() * sizeof(int)));
  int* segs = (int*)m->sc->seg_buf.p;
  RET(upload(s, segs, tr));
  float* logits = nullptr;
  RET(ctc_head_logits(m, s, head, d_enc_out, c.enc_dim, o.total, true, &logits));
  if (!d_lprob) {
    RET(launch_masked_argmax(logits, V, o.total, V, c.pad, c.unk, -1, -1, d_raw, s));
    return launch_ctc_collapse(d_raw, 0, 0, c.pad, d_tokens, d_index, d_counts, s, segs, B);
  }
  RET(launch_masked_argmax_lprob(logits, V, o.total, V, c.pad, c.unk, -1, d_raw, d_lprob, s));
  return launch_ctc_collapse_spans(d_raw, d_lprob, 0, 0, c.pad, d_tokens, d_index, d_last, d_tok_lprob, d_counts, s, segs, B);
}

extern "C" int ss_batch_ctc_greedy(ss_model* m, void* stream, int head, int B, const float* d_enc_out,
                                   const int32_t* h_Tp, int32_t* d_raw, int32_t* d_tokens, int32_t* d_index,
                                   int32_t* d_counts) {
  if (!m || B <= 0 || head < 0 || head > 1) return SS_ERR_ARG;
  return batch_ctc_greedy(m, stream, head, B, d_enc_out, h_Tp, d_raw, d_tokens, d_index, d_counts, nullptr, nullptr, nullptr);
}

extern "C" int ss_batch_ctc_greedy_scored(ss_model* m, void* stream, int head, int B, const float* d_enc_out, const int32_t* h_Tp,
                                          int32_t* d_raw, int32_t* d_tokens, int32_t* d_index, int32_t* d_counts, float* d_lprob,
                                          int32_t* d_last, float* d_tok_lprob) {
  if (!m || B <= 0 || head < 0 || head > 1 || !d_lprob || !d_last || !d_tok_lprob) return SS_ERR_ARG;
  return batch_ctc_greedy(m, stream, head, B, d_enc_out, h_Tp, d_raw, d_tokens, d_index, d_counts, d_lprob, d_last, d_tok_lprob);
}

// Forced alignment of given labels on a text head: ss_batch_ctc_greedy_scored's head GEMM (the same linear, CanonScope and workspace),
// then the two kernels of ctc_align.hip.  Every refusal comes before the first launch; the per-frame values and the back-pointers
// live in the encoder scratch (idle here: d_enc_out is the caller's), the tables in the segment buffer.
extern "C" int ss_batch_ctc_align(ss_model* m, void* stream, int head, int B, const float* d_enc_out, const int32_t* h_Tp,
                                  const int32_t* h_targets, const int32_t* h_n_targets, ss_ctc_align_result* d_results,
                                  int32_t* d_path, int32_t* d_first, int32_t* d_last, float* d_tok_lprob) {
  if (!m || B <= 0 || head < 0 || head > 1 || !d_enc_out || !h_Tp || !h_n_targets || !d_results) return SS_ERR_ARG;
  const ss_config& c = m->cfg;
  const int V = head == 0 ? c.src_vocab : c.tgt_vocab;
  CtcAlignPlan plan;
  RET(ctc_align_plan(V, c.pad, B, h_Tp, h_targets, h_n_targets, plan));
  if (plan.labels > 0 && (!d_first || !d_last || !d_tok_lprob)) return SS_ERR_ARG;
  SkScope sk_scope(m->sc->skws);
  CanonScope canon_scope(m->pack_invariant ? CANON_SEQ : CANON_NONE);
  hipStream_t s = (hipStream_t)stream;
  RET(m->sc->mt_ws.ensure((size_t)plan.rows * V * sizeof(float)));
  RET(m->sc->ws.ensure(plan.work_bytes()));
  RET(m->sc->seg_buf.ensure(ctc_align_table_bytes(plan)));
  float* logits = nullptr;
  RET(ctc_head_logits(m, s, head, d_enc_out, c.enc_dim, plan.rows, true, &logits));
  return launch_ctc_align(logits, V, V, plan, h_targets, m->sc->seg_buf.p, m->sc->ws.p, d_results, d_path, d_first, d_last, d_tok_lprob,
                          nullptr, s);
}

// The lock-step decode step of the three text searches (ss_batch_mt_greedy, ss_batch_mt_continue, beam.hip's beam_search; declared
// in model_internal.hpp).  What differs between them is in `a`; when the host looks at the tokens, what follows the logits (masked
// arg-max, or top-k and merge) and where the states end up stay with each search.
int mt_decode_rows(ss_model* m, hipStream_t s, const MtRowsWs& w, const MtRowsStep& a) {
  const ss_config& c = m->cfg;
  const int D = c.dec_dim, V = c.tgt_vocab, H = c.dec_heads, n = a.rows;
  const float emb_scale = sqrtf((float)D);
  if (a.row_pos)
    RET(launch_embed_tokens_rows(a.tok, m->mt_emb, m->mt_pos, c.max_tgt_pos, emb_scale, a.ci + c.pad + 1, a.row_pos, w.x, n, D, s,
                                 a.row_pad, V));
  else
    RET(launch_embed_tokens(a.tok, m->mt_emb, m->mt_pos, emb_scale, a.ci + c.pad + 1, w.x, n, D, s, 0, -1, V));
  for (int l = 0; l < c.mt_layers; ++l) {
    float* cache = m->sc->bmt_self.f() + (size_t)l * n * a.cache_ld * 3 * D;
    float* rows = cache + (size_t)a.ci * 3 * D;                      // search row r at + r * cache_ld * 3D: straight into its cache
    AttnArgs at;
    at.Q = rows; at.ldq = a.cache_ld * 3 * D; at.K = cache + D; at.V = cache + 2 * D; at.ldk = at.ldv = 3 * D;
    at.O = w.h; at.ldo = D; at.H = H; at.scale = 1.f; at.causal = 0;   // the key range holds exactly the visible keys
    at.segs = a.self_segs; at.nseg = n; at.max_q = 1;
    at.anc = a.anc; at.anc_ld = a.anc_ld; at.anc_slots = a.anc_slots;
    AttnArgs ac;
    ac.Q = w.q2; ac.ldq = D; ac.K = m->sc->mt_cross.f() + (size_t)l * a.n_enc * 2 * D; ac.V = ac.K + D; ac.ldk = ac.ldv = 2 * D;
    ac.O = w.h; ac.ldo = D; ac.H = H; ac.scale = 1.f; ac.segs = a.cross_segs; ac.nseg = n; ac.max_q = 1;
    RET(dec_layer_ex(s, c, m->mt[l], w.x, n, rows, a.cache_ld * 3 * D, at, &ac, w.h, w.q2, w.ff));
  }
  RET(launch_layernorm(w.x, D, a.states, a.states_ld, m->mt_ln.g, m->mt_ln.b, n, D, 1e-5f, s));
  Lin proj{m->mt_emb, nullptr};                                      // tied output projection, no bias
  return linear(s, a.states, a.states_ld, n, proj, V, D, w.logits, V);
}

// Prefix beam search on a text head: ss_batch_ctc_greedy_scored's head GEMM (the same linear, CanonScope and workspace), then the
// two kernels of ctc_beam.hip.  Every refusal comes before the first launch; the tries, child tables and per-frame values live in
// the encoder scratch (idle here: d_enc_out is the caller's), the table of the pack in the segment buffer.  with_lm: an n-gram
// model fused into the order (ctc_beam.hpp) -- the plain call's GEMM, scopes and buffers, 20 more bytes per trie node in the encoder
// scratch; the model's refusals come with the plain ones, before the first launch.  with_bias: a hotword set as well or alone
// (ctc_bias.hpp): 20 bytes per node, 32 with a model, and its refusals before the first launch too.
static int batch_ctc_beam(ss_model* m, void* stream, int head, int B, const float* d_enc_out, const int32_t* h_Tp, int beam, int cand,
                          int nbest, void* d_hyps, int32_t* d_tokens, int out_stride, bool with_lm, const ss_ngram_lm* lm,
                          const ss_ctc_lm_opts* opts, bool with_bias = false, const ss_ctc_bias* bias = nullptr,
                          const ss_ctc_bias_opts* bopts = nullptr) {
  if (!m || B <= 0 || head < 0 || head > 1 || !d_enc_out || !h_Tp || !d_hyps || !d_tokens) return SS_ERR_ARG;
  const ss_config& c = m->cfg;
  const int V = head == 0 ? c.src_vocab : c.tgt_vocab;
  CtcBeamPlan plan;
  RET(ctc_beam_plan(V, B, h_Tp, beam, cand, nbest, out_stride, plan));
  if (with_bias) RET(ctc_beam_bias_check(bias, V, c.pad, c.unk, bopts, lm, opts));
  if (with_lm) RET(ctc_beam_lm_check(lm, V, opts));
  SkScope sk_scope(m->sc->skws);
  CanonScope canon_scope(m->pack_invariant ? CANON_SEQ : CANON_NONE);
  hipStream_t s = (hipStream_t)stream;
  RET(m->sc->mt_ws.ensure((size_t)plan.rows * V * sizeof(float)));
  RET(m->sc->ws.ensure(plan.work_bytes_form((with_lm ? CTC_FORM_LM : 0) | (with_bias ? CTC_FORM_BIAS : 0))));
  RET(m->sc->seg_buf.ensure(ctc_beam_table_bytes(plan)));
  float* logits = nullptr;
  RET(ctc_head_logits(m, s, head, d_enc_out, c.enc_dim, plan.rows, true, &logits));
  return launch_ctc_beam(logits, V, V, c.pad, c.unk, plan, m->sc->seg_buf.p, m->sc->ws.p, lm, opts, d_hyps, d_tokens, out_stride, nullptr,
                         nullptr, s, bias, bopts);
}

extern "C" int ss_batch_ctc_beam(ss_model* m, void* stream, int head, int B, const float* d_enc_out, const int32_t* h_Tp, int beam,
                                 int cand, int nbest, ss_ctc_beam_hyp* d_hyps, int32_t* d_tokens, int out_stride) {
  return batch_ctc_beam(m, stream, head, B, d_enc_out, h_Tp, beam, cand, nbest, d_hyps, d_tokens, out_stride, false, nullptr, nullptr);
}

extern "C" int ss_batch_ctc_beam_lm(ss_model* m, void* stream, int head, int B, const float* d_enc_out, const int32_t* h_Tp, int beam,
                                    int cand, int nbest, ss_ctc_beam_lm_hyp* d_hyps, int32_t* d_tokens, int out_stride,
                                    const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts) {
  return batch_ctc_beam(m, stream, head, B, d_enc_out, h_Tp, beam, cand, nbest, d_hyps, d_tokens, out_stride, true, lm, opts);
}

extern "C" int ss_batch_ctc_beam_bias(ss_model* m, void* stream, int head, int B, const float* d_enc_out, const int32_t* h_Tp, int beam,
                                      int cand, int nbest, ss_ctc_beam_bias_hyp* d_hyps, int32_t* d_tokens, int out_stride,
                                      const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts, const ss_ctc_bias* bias,
                                      const ss_ctc_bias_opts* bias_opts) {
  return batch_ctc_beam(m, stream, head, B, d_enc_out, h_Tp, beam, cand, nbest, d_hyps, d_tokens, out_stride, lm != nullptr, lm, opts, true,
                        bias, bias_opts);
}

// Batched beam-1 search: all utterances start from [</s>] and advance in lockstep, one row per
// utterance (M = B GEMMs stream every decoder weight once per step for the whole batch).
extern "C" int ss_batch_mt_greedy(ss_model* m, void* stream, int B, const float* d_enc_out, const int32_t* h_Tp,
                                  const int32_t* h_max_len, int min_len, int32_t* h_out_tokens, int out_stride,
                                  int32_t* h_n_out, float* d_feats, int feat_rows) {
  if (!m || B <= 0 || B > 256 || !d_feats) return SS_ERR_ARG;     // (256: the segment tables of the slab kernels)
  SkScope sk_scope(m->sc->skws);
  CanonScope canon_scope(m->pack_invariant ? CANON_SEQ : CANON_NONE);     // cross K|V over the packed encoder rows
  hipStream_t s = (hipStream_t)stream;
  const ss_config& c = m->cfg;
  const int D = c.dec_dim, F = c.dec_ffn, V = c.tgt_vocab;
  int Lmax = 0;
  for (int b = 0; b < B; ++b) {
    if (h_Tp[b] <= 0 || h_max_len[b] < 0) return SS_ERR_ARG;   // an utterance without encoder rows has nothing to attend to
    Lmax = std::max(Lmax, h_max_len[b]);
  }
  const int Lcap = Lmax + 2;
  if (Lcap > feat_rows || Lcap + 2 > c.max_tgt_pos || out_stride < Lmax + 1) return SS_ERR_CAPACITY;
  const Offsets oe = prefix(h_Tp, B);
  // cross-attention K/V for every layer over the packed encoder rows
  RET(m->sc->mt_cross.ensure((size_t)c.mt_layers * oe.total * 2 * D * sizeof(float)));
  RET(mt_cross_kv(m, s, d_enc_out, oe.total));
  // caches / scratch
  RET(m->sc->bmt_self.ensure((size_t)c.mt_layers * B * Lcap * 3 * D * sizeof(float)));
  RET(m->sc->mt_ws.ensure(MtRowsWs::floats(B, D, F, V) * sizeof(float)));
  const MtRowsWs w(m->sc->mt_ws.f(), B, D, F);
  // int tables: tokens [Lcap+1][B], max_len [B], cross segs [B][4], self segs per step [Lcap][B][4]
  const size_t n_tok = (size_t)(Lcap + 1) * B;
  RET(m->sc->seg_buf.ensure((n_tok + B + 4 * B + (size_t)Lcap * 4 * B) * sizeof(int)));
  int* tok = (int*)m->sc->seg_buf.p;
  int* d_maxlen = tok + n_tok;
  int* d_cross = d_maxlen + B;
  int* d_self = d_cross + 4 * B;
  {
    std::vector<int> t0(B, c.eos), ml(h_max_len, h_max_len + B), cs(4 * B), ss((size_t)Lcap * 4 * B);
    for (int b = 0; b < B; ++b) { cs[4 * b] = b; cs[4 * b + 1] = 1; cs[4 * b + 2] = oe.off[b]; cs[4 * b + 3] = h_Tp[b]; }
    for (int st = 0; st < Lcap; ++st)
      for (int b = 0; b < B; ++b) {
        int* e = &ss[((size_t)st * B + b) * 4];
        e[0] = b; e[1] = 1; e[2] = b * Lcap; e[3] = st + 1;
      }
    RET(upload(s, tok, t0)); RET(upload(s, d_maxlen, ml)); RET(upload(s, d_cross, cs)); RET(upload(s, d_self, ss));
  }
  std::vector<int> host_tok(n_tok, c.pad);
  std::vector<int> eos_at(B, -1);
  int checked = 1;     // token rows [1, checked) already copied to the host
  int step = 0;        // position being fed
  constexpr int kCheck = 4;
  // the decode rows (one per utterance): the small-M kernel in a split-K form fixed by the layer shape -- not by B (with B <= 4 the
  // heuristic would take the GEMV, with B = 64 another wave arrangement for the vocabulary projection)
  CanonScope decode_scope(m->pack_invariant ? CANON_SMALLM : CANON_NONE);
  while (true) {
    // feed position `step` of every utterance; its states go to d_feats in place (utterance b at + b*feat_rows*D)
    MtRowsStep a;
    a.rows = B; a.cache_ld = Lcap; a.ci = step; a.tok = tok + (size_t)step * B;
    a.self_segs = d_self + (size_t)step * 4 * B; a.cross_segs = d_cross; a.n_enc = oe.total;
    a.states = d_feats + (size_t)step * D; a.states_ld = feat_rows * D;
    RET(mt_decode_rows(m, s, w, a));
    RET(launch_masked_argmax(w.logits, V, B, V, c.pad, step < min_len ? c.eos : -1, -1, -1, tok + (size_t)(step + 1) * B, s,
                             d_maxlen, step, c.eos));
    ++step;                                                           // tokens of row `step` now exist
    const bool last = step > Lmax;
    if (last || step % kCheck == 0) {
      SS_HIP_CHECK(hipMemcpyAsync(host_tok.data() + (size_t)checked * B, tok + (size_t)checked * B,
                                  (size_t)(step + 1 - checked) * B * sizeof(int), hipMemcpyDeviceToHost, s));
      SS_HIP_CHECK(hipStreamSynchronize(s));
      bool all_done = true;
      for (int b = 0; b < B; ++b) {
        for (int r = checked; r <= step && eos_at[b] < 0; ++r)
          if (host_tok[(size_t)r * B + b] == c.eos) eos_at[b] = r;
        if (eos_at[b] < 0) all_done = false;
      }
      checked = step + 1;
      if (all_done || last) break;
    }
  }
  for (int b = 0; b < B; ++b) {
    const int end = eos_at[b] >= 0 ? eos_at[b] : step;      // row of the last generated token
    h_n_out[b] = end;                                        // tokens generated = rows 1..end
    for (int r = 1; r <= end; ++r) h_out_tokens[(size_t)b * out_stride + (r - 1)] = host_tok[(size_t)r * B + b];
  }
  return SS_OK;
}

// ss_batch_t2u_units and ss_batch_t2u_units_pad.  h_pad == nullptr: no key is masked anywhere and no mask table exists (the launches
// of ss_batch_t2u_units as they always were).  Otherwise row b's last h_pad[b] states are trailing <pad> positions, masked as keys as
// ss_t2u_units(..., n_tail_pad) masks them: in the T2U encoder (h_pad[b] rows), the unit decoder's self-attention (up x h_pad[b]) and
// its cross-attention (h_pad[b]); they are still decoded.  A row with h_pad[b] = 0 takes exactly the unmasked arithmetic.
static int batch_t2u(ss_model* m, void* stream, int B, const float* d_feats, int feat_rows, const int32_t* h_n, const int32_t* h_pad,
                     int t2u_causal, int mask_eos, int32_t* d_raw, int32_t* d_tokens, int32_t* d_counts) {
  if (!m || B <= 0 || !h_n) return SS_ERR_ARG;
  SkScope sk_scope(m->sc->skws);
  CanonScope canon_scope(m->pack_invariant ? CANON_SEQ : CANON_NONE);
  hipStream_t s = (hipStream_t)stream;
  const ss_config& c = m->cfg;
  const int D = c.dec_dim, F = c.dec_ffn, V = c.unit_vocab, H = c.dec_heads, up = c.ctc_upsample;
  for (int b = 0; b < B; ++b)
    if (h_n[b] <= 0) return SS_ERR_ARG;                    // every utterance feeds at least the leading </s> state
  if (h_pad)
    for (int b = 0; b < B; ++b)
      if (h_pad[b] < 0 || h_pad[b] >= h_n[b]) return SS_ERR_ARG;   // the leading </s> state is never padding
  const Offsets on = prefix(h_n, B);
  const int Nn = on.total, U = Nn * up;
  const size_t nx = (size_t)U * D;
  // The unit decoder's input is up = 25 copies of each of the Nn rows t2u_out + pos_row, so its first layer's LayerNorm + QKV linear
  // need the Nn distinct rows only: under pack-invariant arithmetic a linear's output row is a function of its input row alone
  // (one summation order whatever the row count or kernel: launch_canon, gemm.hip) and so is the LayerNorm kernel's, hence the
  // copies of the Nn result rows are the bits the U-row launches gave.  Without it the route depends on the row count: all rows.
  const bool l0_distinct = m->pack_invariant && !debug_tile_forced() && disp().unit_l0_distinct && c.unit_layers > 0 && up > 1;
  RET(m->sc->ws.ensure((3 * nx + (size_t)U * 3 * D + (size_t)U * F + (size_t)Nn * 2 * D + (size_t)Nn * D +
                    (l0_distinct ? (size_t)Nn * 4 * D : 0) + (size_t)U * V + (size_t)U) * sizeof(float)));
  float* x = m->sc->ws.f();
  float* h = x + nx;
  float* q2 = h + nx;
  float* selfbuf = q2 + nx;
  float* ff = selfbuf + (size_t)U * 3 * D;
  float* crosskv = ff + (size_t)U * F;
  float* t2u_out = crosskv + (size_t)Nn * 2 * D;
  float* x0 = t2u_out + (size_t)Nn * D;          // l0_distinct: the distinct unit-decoder input rows [Nn, D] ...
  float* qkv0 = x0 + (size_t)Nn * D;              // ... and their first-layer QKV rows [Nn, 3D]
  float* logits = l0_distinct ? qkv0 + (size_t)Nn * 3 * D : x0;
  int32_t* idx_scratch = reinterpret_cast<int32_t*>(logits + (size_t)U * V);
  // tables: t2u self {off,n,off,n}; unit self {25off,25n,25off,25n}; unit cross {25off,25n,off,n}; rows {25off,25n}
  std::vector<int> tab(14 * B + Nn + (h_pad ? 3 * B : 0));   // + the packed row -> row of d_feats map of the gather below (+ the masks)
  for (int b = 0; b < B; ++b) {
    const int o = on.off[b], n = h_n[b];
    for (int r = 0; r < n; ++r) tab[14 * B + o + r] = b * feat_rows + r;
    int* a = &tab[4 * b]; a[0] = o; a[1] = n; a[2] = o; a[3] = n;
    int* u = &tab[4 * B + 4 * b]; u[0] = o * up; u[1] = n * up; u[2] = o * up; u[3] = n * up;
    int* x2 = &tab[8 * B + 4 * b]; x2[0] = o * up; x2[1] = n * up; x2[2] = o; x2[3] = n;
    tab[12 * B + 2 * b] = o * up; tab[12 * B + 2 * b + 1] = n * up;
    if (h_pad) {                                  // trailing keys masked per segment: T2U self | unit self | unit cross
      int* k = &tab[14 * B + Nn];
      k[b] = h_pad[b]; k[B + b] = h_pad[b] * up; k[2 * B + b] = h_pad[b];
    }
  }
  RET(m->sc->seg_buf.ensure(tab.size() * sizeof(int)));
  int* dt = (int*)m->sc->seg_buf.p;
  RET(upload(s, dt, tab));
  const int* tail = h_pad ? dt + 14 * B + Nn : nullptr;
  // gather the decoder states of each utterance into packed rows: ONE launch (round 4 issued B device-to-device copies per pack --
  // 2975 __amd_rocclr_copyBuffer launches, 1 % of the one-stream kernel time and 64 more dependent launches per pack)
  for (int b = 0; b < B; ++b)
    if (h_n[b] > feat_rows) return SS_ERR_CAPACITY;
  RET(launch_gather_rows(dt + 14 * B, d_feats, D, x, Nn, s, B * feat_rows));
  for (int l = 0; l < c.t2u_layers; ++l) {
    AttnArgs at;
    at.Q = selfbuf; at.ldq = 3 * D; at.K = selfbuf + D; at.V = selfbuf + 2 * D; at.ldk = at.ldv = 3 * D;
    at.O = h; at.ldo = D; at.H = H; at.scale = 1.f; at.causal = t2u_causal ? 1 : 0;
    at.segs = dt; at.nseg = B; at.max_q = on.mx;
    at.no_decode_kernel = m->pack_invariant;       // max_q is the pack's longest utterance: it must not pick the kernel
    at.seg_tail = tail;
    RET(dec_layer_ex(s, c, m->t2u[l], x, Nn, selfbuf, 3 * D, at, nullptr, h, q2, ff));
  }
  RET(launch_layernorm(x, D, t2u_out, D, m->t2u_ln.g, m->t2u_ln.b, Nn, D, 1e-5f, s));
  RET(launch_upsample_add_pos(t2u_out, Nn, up, m->unit_pos_row, (float)c.pad, x, D, s));
  for (int l = 0; l < c.unit_layers; ++l) {
    RET(linear(s, t2u_out, D, Nn, m->unit[l].cross_kv, 2 * D, D, crosskv, 2 * D));
    AttnArgs at;
    at.Q = selfbuf; at.ldq = 3 * D; at.K = selfbuf + D; at.V = selfbuf + 2 * D; at.ldk = at.ldv = 3 * D;
    at.O = h; at.ldo = D; at.H = H; at.scale = 1.f; at.causal = 1;
    at.segs = dt + 4 * B; at.nseg = B; at.max_q = on.mx * up; at.no_decode_kernel = m->pack_invariant;
    AttnArgs ac;
    ac.Q = q2; ac.ldq = D; ac.K = crosskv; ac.V = crosskv + D; ac.ldk = ac.ldv = 2 * D;
    ac.O = h; ac.ldo = D; ac.H = H; ac.scale = 1.f; ac.segs = dt + 8 * B; ac.nseg = B; ac.max_q = on.mx * up;
    ac.no_decode_kernel = m->pack_invariant;
    if (tail) { at.seg_tail = tail + B; ac.seg_tail = tail + 2 * B; }
    if (l == 0 && l0_distinct) {
      RET(launch_upsample_add_pos(t2u_out, Nn, 1, m->unit_pos_row, (float)c.pad, x0, D, s));   // the same formula: row r of x0 = rows 25 r .. 25 r + 24 of x
      RET(dec_layer_qkv(s, c, m->unit[0], x0, Nn, qkv0, 3 * D, h));
      RET(launch_upsample_rows(qkv0, Nn, up, selfbuf, 3 * D, s));
      RET(dec_layer_rest(s, c, m->unit[0], x, U, at, &ac, h, q2, ff));
      continue;
    }
    RET(dec_layer_ex(s, c, m->unit[l], x, U, selfbuf, 3 * D, at, &ac, h, q2, ff));
  }
  RET(launch_layernorm(x, D, h, D, m->unit_ln.g, m->unit_ln.b, U, D, 1e-5f, s));
  RET(linear(s, h, D, U, m->unit_out, V, D, logits, V));
  m->sc->dbg_logits = logits; m->sc->dbg_rows = U; m->sc->dbg_cols = V;
  RET(launch_masked_argmax(logits, V, U, V, c.pad, c.unk, mask_eos ? c.eos : -1, -1, d_raw, s));
  return launch_ctc_collapse(d_raw, 0, V - 1, c.pad, d_tokens, idx_scratch, d_counts, s, dt + 12 * B, B);
}

extern "C" int ss_batch_t2u_units(ss_model* m, void* stream, int B, const float* d_feats, int feat_rows,
                                  const int32_t* h_n, int t2u_causal, int mask_eos, int32_t* d_raw, int32_t* d_tokens,
                                  int32_t* d_counts) {
  return batch_t2u(m, stream, B, d_feats, feat_rows, h_n, nullptr, t2u_causal, mask_eos, d_raw, d_tokens, d_counts);
}

extern "C" int ss_batch_t2u_units_pad(ss_model* m, void* stream, int B, const float* d_feats, int feat_rows, const int32_t* h_n,
                                      const int32_t* h_n_tail_pad, int t2u_causal, int mask_eos, int32_t* d_raw, int32_t* d_tokens,
                                      int32_t* d_counts) {
  if (!h_n_tail_pad) return SS_ERR_ARG;
  return batch_t2u(m, stream, B, d_feats, feat_rows, h_n, h_n_tail_pad, t2u_causal, mask_eos, d_raw, d_tokens, d_counts);
}

// Ragged continuation of B independent beam-1 searches (ss_batch_mt_continue): row b feeds [</s>, prefix_b...] and generates, with
// the semantics of ss_mt_greedy per row.  Two phases:
//  * the prefix pass: ONE ragged decoder pass over the sum(n_prefix_b + 1) fed rows (causal self-attention per segment, cross-attention
//    per session, CANON_SEQ), its K/V rows scattered into the lock-step cache, only each segment's last row projected onto the vocabulary;
//  * the lock-step loop: one row per session.  Row b's cache is shifted by sh_b = S - start_b (S = the longest prefix), so every row's
//    first generated position sits at cache index S + 1 and the QKV rows of a step keep one stride.  Positions, the self-attention key
//    range and the min / max length tests are per row (position = cache index - sh_b).
// Host-side layout of one ss_batch_mt_continue call, and every refusal it makes (also exported as ss_batch_mt_continue_plan, which
// engine.plan_mt_continue reads: the tables below are what the call uploads).  `head` holds, in this order: max_len' [B] | min_len'
// [B] | row position offset [B] | lock-step cross segs [4B] | prefix self segs [4B] | prefix cross segs [4B] | lock-step self segs
// [Tr][4B] | prefix tokens [Np] | prefix positions [Np] | prefix row -> cache row [Np] | prefix row -> feature row [Np] | last prefix
// row of each segment [B].
struct McPlan {
  int S = 0, Tn = 0, Lcap = 0, Tr = 0, Np = 0, np_max = 0;   // longest prefix, most lock-step steps, cache rows, lock-step table rows,
  std::vector<int> head;                                     // prefix-pass rows, longest segment
};
static int mt_continue_plan(int B, const int32_t* h_Tp, const int32_t* h_prefix, const int32_t* h_n_prefix, const int32_t* h_max_len,
                            int min_len, int out_stride, int feat_rows, int max_tgt_pos, int vocab, int eos, McPlan& P) {
  if (B <= 0 || B > 256 || !h_Tp || !h_n_prefix || !h_max_len) return SS_ERR_ARG;   // (256: the segment tables of the slab kernels)
  int S = 0, Tn = 0, Np = 0, np_max = 0;
  for (int b = 0; b < B; ++b) {
    const int st = h_n_prefix[b];
    if (h_Tp[b] <= 0 || st < 0 || h_max_len[b] < st) return SS_ERR_ARG;
    if (st > 0 && !h_prefix) return SS_ERR_ARG;
    S = std::max(S, st);
    Tn = std::max(Tn, h_max_len[b] - st);
    Np += st + 1;
    np_max = std::max(np_max, st + 1);
  }
  {
    int o = 0;
    for (int b = 0; b < B; ++b) {
      for (int i = 0; i < h_n_prefix[b]; ++i)
        if (h_prefix[o + i] < 0 || h_prefix[o + i] >= vocab) return SS_ERR_ARG;   // nn.Embedding's IndexError in the reference
      o += h_n_prefix[b];
    }
  }
  for (int b = 0; b < B; ++b)                            // fed positions 0 .. max_len_b; tokens after the prefix up to max_len_b - st + 1
    if (h_max_len[b] + 1 > feat_rows || h_max_len[b] - h_n_prefix[b] + 1 > out_stride || h_max_len[b] + 3 > max_tgt_pos)
      return SS_ERR_CAPACITY;
  const int Lcap = S + 1 + Tn, Tr = std::max(Tn, 1);
  const Offsets oe = prefix(h_Tp, B);
  std::vector<int> seg_len(B);
  for (int b = 0; b < B; ++b) seg_len[b] = h_n_prefix[b] + 1;
  const Offsets op = prefix(seg_len.data(), B);
  const size_t np = (size_t)Np;
  P.S = S; P.Tn = Tn; P.Lcap = Lcap; P.Tr = Tr; P.Np = Np; P.np_max = np_max;
  P.head.assign(15 * (size_t)B + (size_t)Tr * 4 * B + 4 * np + B, 0);
  int* ml = P.head.data(); int* mn = ml + B; int* rp = mn + B; int* cs = rp + B; int* ps = cs + 4 * B; int* pc = ps + 4 * B;
  int* ls = pc + 4 * B; int* pt = ls + (size_t)Tr * 4 * B; int* pp = pt + np; int* pk = pp + np; int* pf = pk + np; int* pl = pf + np;
  int o = 0;
  for (int b = 0; b < B; ++b) {
    const int st = h_n_prefix[b], sh = S - st, r0 = op.off[b];
    ml[b] = h_max_len[b] + sh; mn[b] = min_len + sh; rp[b] = -sh;
    cs[4 * b] = b; cs[4 * b + 1] = 1; cs[4 * b + 2] = oe.off[b]; cs[4 * b + 3] = h_Tp[b];
    ps[4 * b] = r0; ps[4 * b + 1] = st + 1; ps[4 * b + 2] = r0; ps[4 * b + 3] = st + 1;
    pc[4 * b] = r0; pc[4 * b + 1] = st + 1; pc[4 * b + 2] = oe.off[b]; pc[4 * b + 3] = h_Tp[b];
    for (int t = 0; t < Tr; ++t) {
      int* e = &ls[((size_t)t * B + b) * 4];
      e[0] = b; e[1] = 1; e[2] = b * Lcap + sh; e[3] = st + 2 + t;      // keys: positions 0 .. st + 1 + t
    }
    for (int p = 0; p <= st; ++p) {
      pt[r0 + p] = p == 0 ? eos : h_prefix[o + p - 1];
      pp[r0 + p] = p;
      pk[r0 + p] = b * Lcap + sh + p;
      pf[r0 + p] = b * feat_rows + p;
    }
    pl[b] = r0 + st;
    o += st;
  }
  return SS_OK;
}

extern "C" int ss_batch_mt_continue_plan(int B, const int32_t* h_Tp, const int32_t* h_prefix, const int32_t* h_n_prefix,
                                         const int32_t* h_max_len, int min_len, int out_stride, int feat_rows, int max_tgt_pos,
                                         int vocab, int eos, int32_t* h_dims, int32_t* h_tables, int64_t tables_cap,
                                         int64_t* h_n_tables) {
  McPlan P;
  RET(mt_continue_plan(B, h_Tp, h_prefix, h_n_prefix, h_max_len, min_len, out_stride, feat_rows, max_tgt_pos, vocab, eos, P));
  if (h_dims) { h_dims[0] = P.S; h_dims[1] = P.Tn; h_dims[2] = P.Lcap; h_dims[3] = P.Np; }
  if (h_n_tables) *h_n_tables = (int64_t)P.head.size();
  if (h_tables) {
    if (tables_cap < (int64_t)P.head.size()) return SS_ERR_CAPACITY;
    std::copy(P.head.begin(), P.head.end(), h_tables);
  }
  return SS_OK;
}

// The ragged prefix pass of ss_batch_mt_continue and ss_batch_mt_features: the Np fed rows (tokens d_ptok at positions d_ppos) through
// every decoder layer in ONE ragged pass -- causal self-attention per segment (d_pself), cross-attention per session over the packed
// encoder rows whose K/V the caller put in mt_cross (d_pcross, n_enc rows), CANON_SEQ -- then the final LayerNorm.  d_ptail (may be
// null): trailing keys masked per segment in the self-attention (<pad> positions).  d_pcache (may be null): each layer's q|k|v rows
// are also scattered to rows d_pcache[] of the lock-step cache (cache_rows rows per layer: sessions x Lcap, or the beam search's
// slots x Lc).  B = the segments of the two tables.  Workspace: m->sc->ws, (7 D + F) floats a row, sized by the caller: x | h | q2 |
// post-LN states | q|k|v | ffn.  *out = the post-LN states [Np][D] (in ws).  Declared in model_internal.hpp (beam.hip calls it too).
int mt_prefix_pass(ss_model* m, hipStream_t s, int B, int Np, int np_max, int n_enc, const int* d_ptok, const int* d_ppos,
                   const int* d_pself, const int* d_pcross, const int* d_ptail, const int* d_pcache, int cache_rows, const float** out) {
  const ss_config& c = m->cfg;
  const int D = c.dec_dim, V = c.tgt_vocab, H = c.dec_heads;
  const size_t np = (size_t)Np;
  float* xp = m->sc->ws.f();
  float* hp = xp + np * D;
  float* q2p = hp + np * D;
  float* pfo = q2p + np * D;
  float* qkvp = pfo + np * D;
  float* ffp = qkvp + np * 3 * D;
  RET(launch_embed_tokens_rows(d_ptok, m->mt_emb, m->mt_pos, c.max_tgt_pos, sqrtf((float)D), c.pad + 1, d_ppos, xp, Np, D, s, c.pad,
                               V));
  for (int l = 0; l < c.mt_layers; ++l) {
    AttnArgs at;
    at.Q = qkvp; at.ldq = 3 * D; at.K = qkvp + D; at.V = qkvp + 2 * D; at.ldk = at.ldv = 3 * D;
    at.O = hp; at.ldo = D; at.H = H; at.scale = 1.f; at.causal = 1;
    at.segs = d_pself; at.nseg = B; at.max_q = np_max; at.no_decode_kernel = m->pack_invariant;   // max_q depends on the pack
    at.seg_tail = d_ptail;
    AttnArgs ac;
    ac.Q = q2p; ac.ldq = D; ac.K = m->sc->mt_cross.f() + (size_t)l * n_enc * 2 * D; ac.V = ac.K + D; ac.ldk = ac.ldv = 2 * D;
    ac.O = hp; ac.ldo = D; ac.H = H; ac.scale = 1.f; ac.segs = d_pcross; ac.nseg = B; ac.max_q = np_max;
    ac.no_decode_kernel = m->pack_invariant;
    RET(dec_layer_ex(s, c, m->mt[l], xp, Np, qkvp, 3 * D, at, &ac, hp, q2p, ffp));
    if (d_pcache)
      RET(launch_scatter_rows(d_pcache, qkvp, 3 * D, m->sc->bmt_self.f() + (size_t)l * cache_rows * 3 * D, 3 * D, 3 * D, Np,
                              cache_rows, s));
  }
  RET(launch_layernorm(xp, D, pfo, D, m->mt_ln.g, m->mt_ln.b, Np, D, 1e-5f, s));
  *out = pfo;
  return SS_OK;
}

extern "C" int ss_batch_mt_continue(ss_model* m, void* stream, int B, const float* d_enc_out, const int32_t* h_Tp,
                                    const int32_t* h_prefix, const int32_t* h_n_prefix, const int32_t* h_max_len, int min_len,
                                    int32_t* h_out_tokens, int out_stride, int32_t* h_n_out, float* d_feats, int feat_rows,
                                    int32_t* h_n_feats) {
  if (!m || !d_enc_out || !h_out_tokens || !h_n_out || !d_feats) return SS_ERR_ARG;
  const ss_config& c = m->cfg;
  const int D = c.dec_dim, F = c.dec_ffn, V = c.tgt_vocab;
  McPlan P;
  RET(mt_continue_plan(B, h_Tp, h_prefix, h_n_prefix, h_max_len, min_len, out_stride, feat_rows, c.max_tgt_pos, V, c.eos, P));
  const int S = P.S, Tn = P.Tn, Np = P.Np, np_max = P.np_max, Lcap = P.Lcap, Tr = P.Tr;
  const Offsets oe = prefix(h_Tp, B);

  // ---- every buffer first: a scratch cap refuses the call before anything is queued ----
  RET(m->sc->mt_cross.ensure((size_t)c.mt_layers * oe.total * 2 * D * sizeof(float)));
  RET(m->sc->bmt_self.ensure((size_t)c.mt_layers * B * Lcap * 3 * D * sizeof(float)));
  const size_t np = (size_t)Np;
  RET(m->sc->ws.ensure((np * (4 * D + 3 * D + F)) * sizeof(float)));
  // the decode rows (with a gap of B rows before the logits) | their states [B][Tr][D], scattered to d_feats at the end
  RET(m->sc->mt_ws.ensure((MtRowsWs::floats(B, D, F, V, (size_t)B * D) + (size_t)B * Tr * D) * sizeof(float)));
  // int tables: tokens [Tn + 2][B] | the plan's tables (mt_continue_plan) | lock-step feature map [B * Tr]
  const size_t n_tok = (size_t)(Tn + 2) * B;
  const size_t n_int = n_tok + P.head.size() + (size_t)B * Tr;
  RET(m->sc->seg_buf.ensure(n_int * sizeof(int)));

  SkScope sk_scope(m->sc->skws);
  CanonScope canon_scope(m->pack_invariant ? CANON_SEQ : CANON_NONE);
  hipStream_t s = (hipStream_t)stream;
  int* tok = (int*)m->sc->seg_buf.p;
  int* d_maxlen = tok + n_tok;
  int* d_minlen = d_maxlen + B;
  int* d_rowpos = d_minlen + B;
  int* d_cross = d_rowpos + B;
  int* d_pself = d_cross + 4 * B;
  int* d_pcross = d_pself + 4 * B;
  int* d_lself = d_pcross + 4 * B;
  int* d_ptok = d_lself + (size_t)Tr * 4 * B;
  int* d_ppos = d_ptok + np;
  int* d_pcache = d_ppos + np;
  int* d_pfeat = d_pcache + np;
  int* d_plast = d_pfeat + np;
  int* d_lfeat = d_plast + B;
  RET(upload(s, d_maxlen, P.head));                      // everything from max_len' to the last-row table, one upload
  RET(mt_cross_kv(m, s, d_enc_out, oe.total));           // of every layer over the packed encoder rows
  const MtRowsWs w(m->sc->mt_ws.f(), B, D, F, (size_t)B * D);
  float* lfeat = w.logits + (size_t)B * V;               // [B][Tr][D]
  // ---- the prefix pass ----
  {
    const float* pfo = nullptr;
    RET(mt_prefix_pass(m, s, B, Np, np_max, oe.total, d_ptok, d_ppos, d_pself, d_pcross, nullptr, d_pcache, B * Lcap, &pfo));
    float* hp = m->sc->ws.f() + np * D;
    RET(launch_scatter_rows(d_pfeat, pfo, D, d_feats, D, D, Np, B * feat_rows, s));
    RET(launch_gather_rows(d_plast, pfo, D, hp, B, s, Np));
    // the first generated token: projected as a lock-step row (one row per session, CANON_SMALLM)
    CanonScope row_scope(m->pack_invariant ? CANON_SMALLM : CANON_NONE);
    Lin proj{m->mt_emb, nullptr};
    RET(linear(s, hp, D, B, proj, V, D, w.logits, V));
    RET(launch_masked_argmax(w.logits, V, B, V, c.pad, -1, -1, -1, tok + B, s, d_maxlen, S, c.eos, d_minlen, c.eos));
  }
  // ---- the lock-step loop ----
  std::vector<int> host_tok(n_tok, c.pad);
  std::vector<int> eos_at(B, -1);
  int checked = 1;                                                   // token rows [1, checked) already on the host
  constexpr int kCheck = 4;
  CanonScope decode_scope(m->pack_invariant ? CANON_SMALLM : CANON_NONE);
  for (int it = 0;; ++it) {                                          // `it` steps done: token rows 1 .. it + 1 exist
    const bool last = it >= Tn;
    if (last || it % kCheck == 0) {
      SS_HIP_CHECK(hipMemcpyAsync(host_tok.data() + (size_t)checked * B, tok + (size_t)checked * B,
                                  (size_t)(it + 2 - checked) * B * sizeof(int), hipMemcpyDeviceToHost, s));
      SS_HIP_CHECK(hipStreamSynchronize(s));
      bool all_done = true;
      for (int b = 0; b < B; ++b) {
        const int lim = h_max_len[b] - h_n_prefix[b] + 1;           // token row forced to </s>
        for (int r = checked; r <= std::min(it + 1, lim) && eos_at[b] < 0; ++r)
          if (host_tok[(size_t)r * B + b] == c.eos) eos_at[b] = r;
        if (eos_at[b] < 0) all_done = false;
      }
      checked = it + 2;
      if (all_done || last) break;
    }
    MtRowsStep a;
    a.rows = B; a.cache_ld = Lcap; a.ci = S + 1 + it;                // the cache index every row feeds
    a.tok = tok + (size_t)(it + 1) * B; a.row_pos = d_rowpos; a.row_pad = c.pad;
    a.self_segs = d_lself + (size_t)it * 4 * B; a.cross_segs = d_cross; a.n_enc = oe.total;
    a.states = lfeat + (size_t)it * D; a.states_ld = Tr * D;
    RET(mt_decode_rows(m, s, w, a));
    RET(launch_masked_argmax(w.logits, V, B, V, c.pad, -1, -1, -1, tok + (size_t)(it + 2) * B, s, d_maxlen, a.ci, c.eos, d_minlen,
                             c.eos));
  }
  // outputs; the decode rows' states go to their positions start_b + 1 .. in d_feats (one launch)
  std::vector<int> fmap((size_t)B * Tr, -1);
  int n_lfeat = 0;
  for (int b = 0; b < B; ++b) {
    const int st = h_n_prefix[b], end = eos_at[b];                   // token rows 1 .. end are the output
    h_n_out[b] = end;
    for (int r = 1; r <= end; ++r) h_out_tokens[(size_t)b * out_stride + (r - 1)] = host_tok[(size_t)r * B + b];
    if (h_n_feats) h_n_feats[b] = st + end;                          // fed positions 0 .. st + end - 1
    for (int t = 0; t < end - 1; ++t) fmap[(size_t)b * Tr + t] = b * feat_rows + st + 1 + t;
    n_lfeat += end - 1;
  }
  if (n_lfeat > 0) {
    RET(upload(s, d_lfeat, fmap));
    RET(launch_scatter_rows(d_lfeat, lfeat, D, d_feats, D, D, B * Tr, B * feat_rows, s));
  }
  return SS_OK;
}

// The optional second answer of the pass below (ss_batch_mt_attention): the head-averaged cross-attention of the last layer.
struct MtAttnOut {
  const int32_t* h_first = nullptr;      // may be null: 0 for every row
  float* d_attn = nullptr; int64_t* h_attn_off = nullptr; int64_t attn_capacity = 0;
  int32_t* d_peak = nullptr; float* d_stat = nullptr;
};

// The optional third answer (ss_batch_mt_score): every fed position's state projected onto the vocabulary and scored against the
// token it predicts (mt_score.hip).  The B rows are texts for U <= B utterances: h_Tp then holds U lengths and row b reads the
// encoder rows of utterance h_src[b] (null: B == U, row b -> utterance b), so candidate texts for one audio share its cross K/V.
struct MtScoreOut {
  int U = 0;
  const int32_t* h_src = nullptr;
  float* d_stat = nullptr; int32_t* d_idx = nullptr;      // [R][2] each, R = sum (n_tokens_b + 1), packed in row order
};
constexpr int kMtScoreChunk = 2048;                       // state rows projected per launch: the logits buffer is [<= 2048][V]

// ss_batch_mt_features (ao == so == nullptr: its launches exactly), ss_batch_mt_attention and ss_batch_mt_score (n_tail_pad ==
// nullptr: no trailing <pad>; at most one of ao / so).
static int batch_mt_features(ss_model* m, void* stream, int B, const float* d_enc_out, const int32_t* h_Tp, const int32_t* h_tokens,
                             const int32_t* h_n_tokens, const int32_t* h_n_tail_pad, float* d_feats, int feat_rows,
                             const MtAttnOut* ao, const MtScoreOut* so = nullptr) {
  if (!m || B <= 0 || B > 256 || !d_enc_out || !h_Tp || !h_n_tokens || (ao && so)) return SS_ERR_ARG;
  if (so ? (!so->d_stat || !so->d_idx) : ao ? (!ao->d_peak || !ao->d_stat) : (!h_n_tail_pad || !d_feats)) return SS_ERR_ARG;
  if (d_feats && feat_rows <= 0) return SS_ERR_ARG;
  const ss_config& c = m->cfg;
  const int D = c.dec_dim, F = c.dec_ffn, V = c.tgt_vocab;
  if (ao && (c.dec_heads > ATTN_PROBS_MAX_H || c.mt_layers <= 0 || !m->mt[c.mt_layers - 1].has_cross)) return SS_ERR_ARG;
  const int U = so ? so->U : B;                           // utterances = entries of h_Tp
  if (so) {
    if (U <= 0 || U > B || (!so->h_src && U != B)) return SS_ERR_ARG;
    for (int u = 0; u < U; ++u)
      if (h_Tp[u] <= 0) return SS_ERR_ARG;
    for (int b = 0; so->h_src && b < B; ++b)
      if (so->h_src[b] < 0 || so->h_src[b] >= U) return SS_ERR_ARG;
  }
  std::vector<int> seg_len(B);
  int tok_total = 0;
  for (int b = 0; b < B; ++b) {
    const int pad_b = h_n_tail_pad ? h_n_tail_pad[b] : 0;
    if ((!so && h_Tp[b] <= 0) || h_n_tokens[b] < 0 || pad_b < 0) return SS_ERR_ARG;
    if (h_n_tokens[b] > 0 && !h_tokens) return SS_ERR_ARG;
    if (ao && ao->h_first && (ao->h_first[b] < 0 || ao->h_first[b] > h_n_tokens[b])) return SS_ERR_ARG;
    for (int i = 0; i < h_n_tokens[b]; ++i) {
      if (h_tokens[tok_total + i] < 0 || h_tokens[tok_total + i] >= c.tgt_vocab) return SS_ERR_ARG;   // nn.Embedding's IndexError
      if (so && h_tokens[tok_total + i] == c.pad) return SS_ERR_ARG;   // SequenceScorer strips pad: it is never a scored token
    }
    tok_total += h_n_tokens[b];
    seg_len[b] = 1 + h_n_tokens[b] + pad_b;
    if ((d_feats && seg_len[b] > feat_rows) || seg_len[b] + 2 > c.max_tgt_pos) return SS_ERR_CAPACITY;   // ss_mt_append's position bound
  }
  const Offsets oe = prefix(h_Tp, U), op = prefix(seg_len.data(), B);
  const int Np = op.total;
  const size_t np = (size_t)Np;
  // int tables: self segs [4B] | cross segs [4B] | self tail [B] | tokens [Np] | positions [Np] | feature rows [Np]
  //             (+ with ao: first answered row [B] | output row [B] | padding to 8 bytes | offsets into d_attn [B] int64)
  //             (+ with so: the token every position predicts [Np])
  const size_t n_base = 9 * (size_t)B + 3 * np;
  const size_t n_off = ao ? ((n_base + 2 * (size_t)B + 1) & ~(size_t)1) : n_base;
  std::vector<int> tab(ao ? n_off + 2 * (size_t)B : so ? n_base + np : n_base);
  int* ps = tab.data(); int* pc = ps + 4 * B; int* pt = pc + 4 * B; int* tk = pt + B; int* pp = tk + np; int* pf = pp + np;
  for (int b = 0, o = 0; b < B; ++b) {
    const int r0 = op.off[b], n = seg_len[b], nt = h_n_tokens[b];
    const int u = so && so->h_src ? so->h_src[b] : b;
    ps[4 * b] = r0; ps[4 * b + 1] = n; ps[4 * b + 2] = r0; ps[4 * b + 3] = n;
    pc[4 * b] = r0; pc[4 * b + 1] = n; pc[4 * b + 2] = oe.off[u]; pc[4 * b + 3] = h_Tp[u];
    pt[b] = h_n_tail_pad ? h_n_tail_pad[b] : 0;
    for (int p = 0; p < n; ++p) {
      tk[r0 + p] = p == 0 ? c.eos : p <= nt ? h_tokens[o + p - 1] : c.pad;
      pp[r0 + p] = p;
      pf[r0 + p] = b * feat_rows + p;
      if (so) tab[n_base + r0 + p] = p < nt ? h_tokens[o + p] : c.eos;   // position p predicts token p, the last one </s>
    }
    o += nt;
  }
  int max_rows = 0;
  if (ao) {
    int* qf = tab.data() + n_base; int* ro = qf + B;
    int rows = 0;
    int64_t off = 0;
    for (int b = 0; b < B; ++b) {
      qf[b] = ao->h_first ? ao->h_first[b] : 0;
      ro[b] = rows;
      const int n = seg_len[b] - qf[b];
      std::memcpy(tab.data() + n_off + 2 * (size_t)b, &off, sizeof(off));
      rows += n; max_rows = std::max(max_rows, n);
      off += (int64_t)n * h_Tp[b];
    }
    if (ao->d_attn && off > ao->attn_capacity) return SS_ERR_CAPACITY;
  }
  // ---- every buffer first: a scratch cap refuses the call before anything is queued ----
  RET(m->sc->mt_cross.ensure((size_t)c.mt_layers * oe.total * 2 * D * sizeof(float)));
  const int n_log = so ? std::min(Np, kMtScoreChunk) : 0;          // logits rows behind the pass's own workspace
  RET(m->sc->ws.ensure((np * (7 * D + F) + (size_t)n_log * V) * sizeof(float)));
  RET(m->sc->seg_buf.ensure(tab.size() * sizeof(int)));
  if (ao && ao->d_attn && ao->h_attn_off)          // the one host output, after the last refusal
    for (int b = 0; b < B; ++b) std::memcpy(&ao->h_attn_off[b], tab.data() + n_off + 2 * (size_t)b, sizeof(int64_t));
  SkScope sk_scope(m->sc->skws);
  CanonScope canon_scope(m->pack_invariant ? CANON_SEQ : CANON_NONE);
  hipStream_t s = (hipStream_t)stream;
  int* dt = (int*)m->sc->seg_buf.p;
  RET(upload(s, dt, tab));
  const int *d_self = dt, *d_cross = dt + 4 * B, *d_tail = dt + 8 * B, *d_tok = dt + 9 * B, *d_pos = d_tok + np, *d_frow = d_pos + np;
  RET(mt_cross_kv(m, s, d_enc_out, oe.total));
  const float* pfo = nullptr;
  RET(mt_prefix_pass(m, s, B, Np, op.mx, oe.total, d_tok, d_pos, d_self, d_cross, d_tail, nullptr, 0, &pfo));
  if (d_feats) RET(launch_scatter_rows(d_frow, pfo, D, d_feats, D, D, Np, B * feat_rows, s));
  if (so) {
    // the output projection of the searches' prefix rows (beam.hip), a chunk of state rows at a time: under CANON_SEQ a logits row
    // is a function of its state row alone, so neither the chunk boundaries nor the pack change a bit; [Np][V] never exists
    float* logits = m->sc->ws.f() + np * (7 * D + F);
    const int* d_tgt = dt + n_base;
    Lin proj{m->mt_emb, nullptr};
    for (int r0 = 0; r0 < Np; r0 += kMtScoreChunk) {
      const int rows = std::min(kMtScoreChunk, Np - r0);
      RET(linear(s, pfo + (size_t)r0 * D, D, rows, proj, V, D, logits, V));
      RET(launch_mt_token_scores(logits, V, rows, V, d_tgt + r0, so->d_stat + 2 * (size_t)r0, so->d_idx + 2 * (size_t)r0, s));
    }
    return SS_OK;
  }
  if (!ao) return SS_OK;
  // the last layer's cross-attention Q is still in the pass's q2 rows (mt_prefix_pass: x | h | q2 | ...; nothing after a layer's
  // cross-attention writes them), its K in the last slice of mt_cross
  AttnProbsArgs ap;
  ap.Q = m->sc->ws.f() + 2 * np * D; ap.ldq = D;
  ap.K = m->sc->mt_cross.f() + (size_t)(c.mt_layers - 1) * oe.total * 2 * D; ap.ldk = 2 * D;
  ap.H = c.dec_heads; ap.scale = 1.f;                                   // q is pre-scaled at pack time
  ap.segs = d_cross; ap.nseg = B;
  ap.q_first = dt + n_base; ap.row_off = dt + n_base + B;
  ap.p_off = reinterpret_cast<const long long*>(dt + n_off);
  ap.P = ao->d_attn; ap.peak = ao->d_peak; ap.stat = ao->d_stat; ap.max_rows = max_rows;
  return launch_attention_probs(ap, s);
}

// Decoder states of B fed rows in ONE ragged pass (the MT features the S2ST write path hands to T2U): row b feeds [</s>, tokens_b...,
// <pad> x n_tail_pad_b] over its encoder rows and gets the post-LN state of every position, as ss_mt_truncate + ss_mt_append(...,
// n_tail_pad) give them for one utterance: the trailing <pad> positions take the padding position and are masked as self-attention
// keys.  Nothing is projected onto the vocabulary.  d_feats [B][feat_rows][D]: row b's 1 + n_tokens_b + n_tail_pad_b states.
extern "C" int ss_batch_mt_features(ss_model* m, void* stream, int B, const float* d_enc_out, const int32_t* h_Tp,
                                    const int32_t* h_tokens, const int32_t* h_n_tokens, const int32_t* h_n_tail_pad, float* d_feats,
                                    int feat_rows) {
  if (!h_n_tail_pad || !d_feats) return SS_ERR_ARG;
  return batch_mt_features(m, stream, B, d_enc_out, h_Tp, h_tokens, h_n_tokens, h_n_tail_pad, d_feats, feat_rows, nullptr);
}

// The same pass without trailing <pad>, answering the head-averaged cross-attention of the last decoder layer over the fed positions
// h_first[b] .. n_tokens_b of every row (attn_probs.hip); d_feats optional (the bits ss_batch_mt_features writes).
extern "C" int ss_batch_mt_attention(ss_model* m, void* stream, int B, const float* d_enc_out, const int32_t* h_Tp,
                                     const int32_t* h_tokens, const int32_t* h_n_tokens, const int32_t* h_first, float* d_feats,
                                     int feat_rows, float* d_attn, int64_t* h_attn_off, int64_t attn_capacity, int32_t* d_peak,
                                     float* d_stat) {
  if (!d_peak || !d_stat || attn_capacity < 0) return SS_ERR_ARG;
  MtAttnOut ao;
  ao.h_first = h_first; ao.d_attn = d_attn; ao.h_attn_off = h_attn_off; ao.attn_capacity = attn_capacity;
  ao.d_peak = d_peak; ao.d_stat = d_stat;
  return batch_mt_features(m, stream, B, d_enc_out, h_Tp, h_tokens, h_n_tokens, nullptr, d_feats, feat_rows, &ao);
}

// The same pass answering how likely the decoder finds each GIVEN text (fairseq's SequenceScorer, --score-reference): row b feeds
// [</s>, tokens_b...] over the encoder rows of utterance h_src[b]; every position's state is projected onto the vocabulary and
// scored against the token it predicts (the last one: </s>).  d_feats optional (the bits ss_batch_mt_features writes).
extern "C" int ss_batch_mt_score(ss_model* m, void* stream, int U, const float* d_enc_out, const int32_t* h_Tp, int B,
                                 const int32_t* h_src, const int32_t* h_tokens, const int32_t* h_n_tokens, float* d_feats,
                                 int feat_rows, float* d_stat, int32_t* d_idx) {
  if (!d_stat || !d_idx) return SS_ERR_ARG;
  MtScoreOut so;
  so.U = U; so.h_src = h_src; so.d_stat = d_stat; so.d_idx = d_idx;
  return batch_mt_features(m, stream, B, d_enc_out, h_Tp, h_tokens, h_n_tokens, nullptr, d_feats, feat_rows, nullptr, &so);
}

// New fbank rows of many streaming sessions in ONE launch (the batched front-end of the text session pool): session b's frames
// h_first[b] .. h_first[b] + h_n[b] - 1 of its own 16-kHz sample history h_pcm[b] go to h_feat[b] (h_n[b] rows of 80).  The kernel of
// ss_fbank_cmvn with a segment table: a row is a function of its own 400 samples, so the rows are the same bits as there.
extern "C" int ss_batch_fbank_frames(ss_model* m, void* stream, int B, const float* const* h_pcm, const int32_t* h_first,
                                     const int32_t* h_n, float pcm_scale, float* const* h_feat) {
  if (!m || B <= 0 || B > 65535 || !h_pcm || !h_first || !h_n || !h_feat) return SS_ERR_ARG;   // (B is the grid's y extent)
  constexpr int kShift = 160;
  int mx = 0;
  for (int b = 0; b < B; ++b) {
    if (h_first[b] < 0 || h_n[b] < 0 || ((int64_t)h_first[b] + (int64_t)h_n[b]) * kShift > (int64_t)0x7fffffff) return SS_ERR_ARG;
    if (h_n[b] > 0 && (!h_pcm[b] || !h_feat[b])) return SS_ERR_ARG;
    mx = std::max(mx, h_n[b]);
  }
  if (mx == 0) return SS_OK;
  hipStream_t s = (hipStream_t)stream;
  // table: segs {pcm_start, n, 0} [3B], padded to 8 bytes, then the pcm and feature pointers [B] each
  const size_t n_seg = (3 * (size_t)B + 1) & ~(size_t)1;
  std::vector<int> tab(n_seg + 4 * (size_t)B, 0);
  int64_t* ptrs = reinterpret_cast<int64_t*>(tab.data() + n_seg);
  for (int b = 0; b < B; ++b) {
    tab[3 * b] = h_first[b] * kShift; tab[3 * b + 1] = h_n[b]; tab[3 * b + 2] = 0;
    ptrs[b] = (int64_t)(uintptr_t)h_pcm[b];
    ptrs[B + b] = (int64_t)(uintptr_t)h_feat[b];
  }
  RET(m->sc->seg_buf.ensure(tab.size() * sizeof(int)));
  int* dt = (int*)m->sc->seg_buf.p;
  RET(upload(s, dt, tab));
  const float* const* d_pcm = reinterpret_cast<const float* const*>(dt + n_seg);
  float* const* d_feat = reinterpret_cast<float* const*>(dt + n_seg + 2 * (size_t)B);
  return launch_fbank_cmvn_ptrs(d_pcm, d_feat, pcm_scale, m->fe_window, m->fe_melw, fe_tables(m), m->fe_mean, m->fe_std, dt, B, mx, s);
}

// ss_batch_fbank_frames for sessions at ANY source rate, from the source-rate histories directly (fbank.hip, fbank_cmvn_sr_kernel):
// session b's rows h_first[b] .. h_first[b] + h_n[b] - 1 of fbank(resample(h_pcm[b][0 .. h_n_in[b]))) go to h_feat[b], the bits of
// ss_resample + ss_fbank_cmvn over that history.  Every refusal is made here, for the whole call, before the launch; the ratio's
// come from fbank_sr_rows, the code ss_fbank_sr_rows exports.
extern "C" int ss_batch_fbank_frames_sr(ss_model* m, void* stream, int B, const float* const* h_pcm, const int32_t* h_n_in,
                                        const int32_t* h_up, const int32_t* h_down, const float* const* h_taps,
                                        const int32_t* h_half_len, const int32_t* h_first, const int32_t* h_n, float pcm_scale,
                                        float* const* h_feat) {
  if (!m || B <= 0 || B > 65535 || !h_pcm || !h_n_in || !h_up || !h_down || !h_taps || !h_half_len || !h_first || !h_n || !h_feat)
    return SS_ERR_ARG;                                                                           // (B is the grid's y extent)
  static_assert(sizeof(FbankSrSeg) % sizeof(int) == 0, "the segment table is uploaded as ints");
  constexpr size_t kSegInts = sizeof(FbankSrSeg) / sizeof(int);
  std::vector<int> tab(kSegInts * (size_t)B, 0);
  int mx = 0, max_taps = 0;
  for (int b = 0; b < B; ++b) {
    if (h_first[b] < 0 || h_n[b] < 0) return SS_ERR_ARG;
    FbankSrSeg sg{};                                  // h_n[b] = 0: n_rows 0, every workgroup of the segment exits
    if (h_n[b] > 0) {
      int rows = 0;
      RET(fbank_sr_rows(h_n_in[b], h_up[b], h_down[b], h_half_len[b], &rows, nullptr));
      if ((int64_t)h_first[b] + (int64_t)h_n[b] > (int64_t)rows) return SS_ERR_ARG;              // a row past what n_in resamples to
      const bool pass = h_up[b] == h_down[b];
      if (!h_pcm[b] || !h_feat[b] || (!pass && !h_taps[b])) return SS_ERR_ARG;
      sg.pcm = h_pcm[b]; sg.taps = h_taps[b]; sg.feat = h_feat[b];
      sg.n_in = h_n_in[b]; sg.up = h_up[b]; sg.down = h_down[b]; sg.half = h_half_len[b]; sg.first = h_first[b]; sg.n_rows = h_n[b];
      mx = std::max(mx, h_n[b]);
      if (!pass) max_taps = std::max(max_taps, 2 * h_half_len[b] + 1);
    }
    std::memcpy(tab.data() + kSegInts * (size_t)b, &sg, sizeof(sg));
  }
  if (mx == 0) return SS_OK;
  hipStream_t s = (hipStream_t)stream;
  RET(m->sc->seg_buf.ensure(tab.size() * sizeof(int)));
  int* dt = (int*)m->sc->seg_buf.p;
  RET(upload(s, dt, tab));
  return launch_fbank_cmvn_sr(reinterpret_cast<const FbankSrSeg*>(dt), B, mx, max_taps, pcm_scale, m->fe_window, m->fe_melw, fe_tables(m),
                              m->fe_mean, m->fe_std, s);
}

extern "C" int ss_fbank_sr_rows(int64_t n_in, int up, int down, int half_len, int32_t* h_n_rows, int32_t* h_n_final) {
  int rows = 0, fin = 0;
  RET(fbank_sr_rows(n_in, up, down, half_len, &rows, &fin));
  if (h_n_rows) *h_n_rows = rows;
  if (h_n_final) *h_n_final = fin;
  return SS_OK;
}
