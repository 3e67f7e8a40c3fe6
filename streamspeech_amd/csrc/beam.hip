// Ragged-batch beam search of the offline first-pass text decoder (ss_batch_mt_beam): B utterances x k hypothesis rows advance in
// lockstep from [</s>].  Reference: SequenceGenerator.generate_decoder (fairseq/examples/speech_to_speech/unity/sequence_generator.py
// :158-525) with BeamSearch.step (fairseq/fairseq/search.py:110-150) and finalize_hypos (fairseq/fairseq/sequence_generator.py:630-760).
// This unit holds the search driver and the ss_batch_mt_* entry points; beam.hpp names the units that hold the kernels and the host stage.
//
// Where fairseq reorders every layer's KV cache after each step, hypothesis slot r here writes its K/V row of step s at [r][s] and
// never overwrites it; the ancestry table anc[r][p] names the slot that holds position p of hypothesis r, and the decode attention
// reads keys and values through it (AttnArgs::anc).  A step then moves B*k*L ints instead of layers x B*k*L x 3D floats.  The tokens
// and cumulative scores fed at each step are kept step-major ([step][slot], never overwritten), so a hypothesis' tokens and scores are
// read through the same table.  Per step, after the decoder launches the greedy twin makes as they are, the top-2k kernel runs one
// workgroup per hypothesis row and the merge kernel one per utterance (beam_kernels.hip).  The host reads the done flags every
// kCheck steps, as ss_batch_mt_greedy does; nothing else synchronises per step.
//
// ss_batch_mt_beam_continue is the same search behind a forced prefix per utterance (the streaming write path): fairseq's
// prefix_tokens of that generator (_prefix_tokens, fairseq/fairseq/sequence_generator.py:596-623).  The forced positions run ONCE per
// utterance, as rows of the ragged prefix pass the greedy continuation uses (mt_prefix_pass, batch.hip); their K/V rows go to the
// utterance's slot 0, and anc[r][p] starts as "slot 0 of my utterance" for them, so nothing is copied into the other k - 1 slots.
// The prefix-score and prefix-chain kernels turn the pass' logits into the forced tokens' scores.  Lock-step index t of utterance b
// is the reference's step n_prefix[b] + t; row b's cache is shifted as in ss_batch_mt_continue, so every row writes cache index
// c0 + t at step t.  ss_batch_mt_beam is the call with no prefix anywhere (c0 = 0, no prefix pass).
//
// The *_opts entry points carry the reference generator's three further controls (ss_mt_search_opts): temperature and the no-repeat
// n-gram ban are the OPT variant of the top-2k kernel, the temperature also a variant of the prefix score kernel, the length penalty
// a variant of the merge kernel; the kernels' launchers choose them.  A forced prefix that itself repeats an n-gram is refused by
// the planner (beam_host.hip), so the prefix pass needs no ban; the agents' and pools' committed prefixes never trip that check,
// because each of their tokens was chosen under the same ban.
//
// ss_batch_mt_beam_cons is the search without a prefix under lexical constraints (fairseq's LexicallyConstrainedBeamSearch, ordered):
// the CONS variants of the same two kernels, and one int of state per slot beside the ancestry.  ss_batch_mt_sample is the same frame
// with the two sampling kernels (beam_sample.hip) where the top-2k and merge kernels stand.
#include <cmath>

#include "model_internal.hpp"
#include "beam.hpp"

namespace {

// d_feats row i = slot-major state row idx[i]; rows with idx < 0 (past the best hypothesis) are left as they are
__global__ __launch_bounds__(256) void beam_feat_gather_kernel(const int* __restrict__ idx, const float* __restrict__ src, int D,
                                                               int src_rows, float* __restrict__ dst) {
  const int r = idx[blockIdx.x];
  if (r < 0 || r >= src_rows) return;
  for (int c = threadIdx.x; c < D; c += 256) dst[(size_t)blockIdx.x * D + c] = src[(size_t)r * D + c];
}

// The search of every entry point; the checks of `P` are done.  With call.h_keys the same call samples: the sampling step and advance
// kernels stand where the top-2k and merge kernels stand, everything else is shared.
int beam_search(const SearchCall& call, const BcPlan& P) {
  ss_model* m = call.m;
  const ss_config& c = m->cfg;
  const bool smp = call.h_keys != nullptr;
  const std::vector<int>* cons_tab = call.cons_tab;
  const int B = call.B, k = call.beam, R = B * k, feat_rows = call.feat_rows, out_stride = call.out_stride;
  const int D = c.dec_dim, F = c.dec_ffn, V = c.tgt_vocab;
  const int Lc = P.Lc, Tn = P.Tn, c0 = P.c0, Np = P.Np;
  // the kernels' arguments that hold for the whole search, and the launchers' refusals before anything is booked
  ConsArgs ca;
  const ConsArgs* cons = cons_tab ? &ca : nullptr;
  TopkOpts to = topk_opts(call.so, R, Lc, c0, nullptr, nullptr, nullptr, nullptr);   // the tables: once they are booked
  SampleArgs sa = call.smp;
  sa.npad = sample_npad(sa, V);
  size_t lds;
  RET(beam_topk_lds(V, to, cons, lds));
  if (smp) RET(sample_step_lds(V, to, sa, lds));
  SkScope sk_scope(m->sc->skws);
  CanonScope canon_scope(m->pack_invariant ? CANON_SEQ : CANON_NONE);
  hipStream_t s = (hipStream_t)call.stream;
  const Offsets oe = prefix(call.h_Tp, B);
  // ---- scratch: everything booked before the first launch ----
  const size_t np = (size_t)Np;
  const size_t n_tok = (size_t)(Tn + 3) * R, n_anc = (size_t)2 * R * Lc, n_cand = (size_t)R * kMaxCand, n_fin = (size_t)B * k * Lc;
  const size_t n_fin_words = B + 2 * (size_t)B * k + 3 * n_fin;
  // constraints: states [2][R] (ping-pong, as the ancestry) | next-token scores and ids [R][2] each | the table
  const size_t n_cons = cons_tab ? 6 * (size_t)R + cons_tab->size() : 0;
  const size_t n_state = 2 * n_tok + n_anc + 2 * n_cand + R + 3 * (size_t)B + n_fin_words + n_cons;
  RET(m->sc->mt_cross.ensure((size_t)c.mt_layers * oe.total * 2 * D * sizeof(float)));
  RET(m->sc->bmt_self.ensure((size_t)c.mt_layers * R * Lc * 3 * D * sizeof(float)));
  RET(m->sc->bmb_feat.ensure((size_t)R * Lc * D * sizeof(float)));
  RET(m->sc->mt_ws.ensure((MtRowsWs::floats(R, D, F, V) + (P.pm ? (size_t)R * D : 0)) * sizeof(float)));
  RET(m->sc->bmb_state.ensure(n_state * sizeof(int)));
  // prefix pass: its workspace (mt_prefix_pass) | logits [Np][V] | forced log-probabilities [Np] | their positional scores [Np]
  if (Np > 0) RET(m->sc->ws.ensure((np * (7 * D + F) + np * V + 2 * np) * sizeof(float)));
  // int tables: the plan's tables | feature gather [B][feat_rows]
  const size_t o_keys = (P.tab.size() + (size_t)B * feat_rows + 1) / 2 * 2;   // sampling: the utterances' keys, 8-byte aligned
  RET(m->sc->seg_buf.ensure((smp ? o_keys + 2 * (size_t)B : P.tab.size() + (size_t)B * feat_rows) * sizeof(int)));

  RET(mt_cross_kv(m, s, call.d_enc_out, oe.total));
  float* feat = m->sc->bmb_feat.f();           // [R][Lc][D] post-LN decoder states of every slot and cache index
  const MtRowsWs rows_ws(m->sc->mt_ws.f(), R, D, F);
  float* logits = rows_ws.logits;
  float* last_rows = logits + (size_t)R * V;   // beam 1: each utterance's last prefix-pass state
  int* w = (int*)m->sc->bmb_state.p;
  BeamState st;
  st.tok = w; w += n_tok;
  st.cum = (float*)w; w += n_tok;
  st.anc = w; w += n_anc;
  st.cand_s = (float*)w; w += n_cand;
  st.cand_t = w; w += n_cand;
  st.ignore = w; w += R;
  st.done = w; w += B;
  st.max_len = w; w += B;
  st.npre = w; w += B;
  int* fin_base = w;
  st.fin_cnt = w; w += B;
  st.fin_score = (float*)w; w += (size_t)B * k;
  st.fin_len = w; w += (size_t)B * k;
  st.fin_tok = w; w += n_fin;
  st.fin_pos = (float*)w; w += n_fin;
  st.fin_anc = w; w += n_fin;
  int* cons_state = w;
  if (cons_tab) { ca.next_s = (float*)(w + 2 * R); ca.next_t = w + 4 * R; ca.tab = w + 6 * R; }
  int* d_tab = (int*)m->sc->seg_buf.p;
  const int* d_cross = d_tab;
  const int* d_self = d_tab + P.o_lself;
  const int* d_rowpos = d_tab + P.o_rowpos;
  const int* d_row0 = d_tab + P.o_row0;
  int* d_gather = d_tab + P.tab.size();
  to = topk_opts(call.so, R, Lc, c0, st.tok, st.anc, d_tab + P.o_ptok, d_row0);
  const std::vector<int> np0 = call.h_n_prefix ? std::vector<int>(call.h_n_prefix, call.h_n_prefix + B) : std::vector<int>(B, 0);   // lives to the end of the call
  SS_HIP_CHECK(hipMemsetAsync(m->sc->bmb_state.p, 0, n_state * sizeof(int), s));   // slot 0 / score 0 / nothing finalised everywhere
  {
    std::vector<int> a0((size_t)R * Lc), ml(call.h_max_len, call.h_max_len + B);
    for (int r = 0; r < R; ++r) {                // prefix-pass positions live in slot 0 of the utterance, the others in the slot itself
      std::fill(a0.begin() + (size_t)r * Lc, a0.begin() + (size_t)r * Lc + P.Smax, (r / k) * k);
      std::fill(a0.begin() + (size_t)r * Lc + P.Smax, a0.begin() + (size_t)(r + 1) * Lc, r);
    }
    RET(upload(s, st.tok, P.tok0)); RET(upload(s, st.max_len, ml)); RET(upload(s, d_tab, P.tab));
    RET(upload(s, st.anc, a0));
    if (smp) {                                   // the ancestry never changes: both halves hold it
      RET(upload(s, st.anc + (size_t)R * Lc, a0));
      SS_HIP_CHECK(hipMemcpyAsync(d_tab + o_keys, call.h_keys, (size_t)B * sizeof(int64_t), hipMemcpyHostToDevice, s));
      sa.keys = reinterpret_cast<const unsigned long long*>(d_tab + o_keys); sa.ignore = st.ignore;
      sa.out_ld = kMaxCand; sa.tok_out = st.cand_t; sa.score_out = st.cand_s;
    }
    if (call.h_n_prefix) RET(upload(s, st.npre, np0));
    if (cons_tab) {                              // every hypothesis starts at the root
      RET(upload(s, cons_state, std::vector<int>((size_t)2 * R, -1)));
      RET(upload(s, cons_state + 6 * R, *cons_tab));
    }
  }
  const float* d_prepos = nullptr;
  if (Np > 0) {
    // ---- the prefix pass: every forced position once per utterance, K/V into slot 0, then the forced tokens' scores ----
    const int* d_ptok = d_tab + P.o_ptok;
    const int *d_ppos = d_ptok + np, *d_pcache = d_ppos + np, *d_pfeat = d_pcache + np, *d_ftok = d_pfeat + np;
    const float* pfo = nullptr;
    RET(mt_prefix_pass(m, s, P.nseg, Np, P.np_max, oe.total, d_ptok, d_ppos, d_tab + P.o_pself, d_tab + P.o_pcross, nullptr, d_pcache,
                       R * Lc, &pfo));
    RET(launch_scatter_rows(d_pfeat, pfo, D, call.d_feats, D, D, Np, B * feat_rows, s));
    float* plog = m->sc->ws.f() + np * (7 * D + F);
    float* lp = plog + np * V;
    float* prepos = lp + np;
    Lin proj{m->mt_emb, nullptr};
    RET(linear(s, pfo, D, Np, proj, V, D, plog, V));
    RET(launch_beam_prefix_score(s, Np, plog, V, d_ftok, c.pad, c.unk, call.unk_penalty, lp, call.so.temp));
    RET(launch_beam_prefix_chain(s, lp, d_row0, st.npre, B, k, st.cum, prepos));
    if (P.pm) RET(launch_gather_rows(d_tab + P.o_plast, pfo, D, last_rows, B, s, Np));
    d_prepos = prepos;
  }
  std::vector<int> host_done(B, 0);
  int step = 0;                                // lock-step index
  constexpr int kCheck = 4;
  CanonScope decode_scope(m->pack_invariant ? CANON_SMALLM : CANON_NONE);   // the greedy twin's decode-row GEMM form
  while (true) {
    const int ci = c0 + step;                  // cache index every slot writes at this step
    if (P.pm && step == 0) {                   // beam 1: the first free step reads the last prefix-pass row, projected as a lock-step row
      Lin proj{m->mt_emb, nullptr};
      RET(linear(s, last_rows, D, R, proj, V, D, logits, V));
    } else {                                   // a slot's cache rows are written once and never reordered: the ancestor table finds them
      MtRowsStep a;
      a.rows = R; a.cache_ld = Lc; a.ci = ci; a.tok = st.tok + (size_t)step * R; a.row_pos = d_rowpos; a.row_pad = -1;
      a.self_segs = d_self + (size_t)step * 4 * R; a.cross_segs = d_cross; a.n_enc = oe.total;
      a.anc = st.anc + (size_t)(step & 1) * R * Lc; a.anc_ld = Lc; a.anc_slots = R;
      a.states = feat + (size_t)ci * D; a.states_ld = Lc * D;
      RET(mt_decode_rows(m, s, rows_ws, a));
    }
    const RowStep rs{logits, V, k, step, call.min_len, st.max_len, st.npre, st.done, smp ? nullptr : st.cum + (size_t)step * R, c.pad, c.unk, c.eos,
                     call.unk_penalty};
    if (smp) {                                 // to.anc: the ancestry never changes
      RET(launch_sample_step(s, R, rs, to, sa));
      RET(launch_sample_advance(s, B, st, k, Lc, step, c0, c.eos, call.normalize, call.so.len_penalty));
    } else {
      to.anc = st.anc + (size_t)(step & 1) * R * Lc;
      if (cons) { ca.state = cons_state + (size_t)(step & 1) * R; ca.state_nxt = cons_state + (size_t)((step + 1) & 1) * R; }
      RET(launch_beam_topk(s, R, rs, st.cand_s, st.cand_t, to, cons));
      RET(launch_beam_merge(s, B, st, k, Lc, V, step, c0, c.eos, call.normalize, call.so.len_penalty, cons));
    }
    const bool last = step >= Tn;              // every utterance is done at its max_len step
    ++step;
    if (last || step % kCheck == 0) {
      SS_HIP_CHECK(hipMemcpyAsync(host_done.data(), st.done, B * sizeof(int), hipMemcpyDeviceToHost, s));
      SS_HIP_CHECK(hipStreamSynchronize(s));
      bool all = true;
      for (int b = 0; b < B; ++b) all = all && host_done[b];
      if (all || last) break;
    }
  }
  // ---- results: the finalised tables, sorted by score (descending; ties keep finalisation order) ----
  std::vector<int> fin(n_fin_words);
  std::vector<float> prepos(np);
  SS_HIP_CHECK(hipMemcpyAsync(fin.data(), fin_base, n_fin_words * sizeof(int), hipMemcpyDeviceToHost, s));
  if (Np > 0) SS_HIP_CHECK(hipMemcpyAsync(prepos.data(), d_prepos, np * sizeof(float), hipMemcpyDeviceToHost, s));
  SS_HIP_CHECK(hipStreamSynchronize(s));
  const int* f_cnt = fin.data();
  const float* f_score = reinterpret_cast<const float*>(f_cnt + B);
  const int* f_len = f_cnt + B + (size_t)B * k;
  const int* f_tok = f_len + (size_t)B * k;
  const float* f_pos = reinterpret_cast<const float*>(f_tok + n_fin);
  const int* f_anc = f_tok + 2 * n_fin;
  const int* row0 = P.tab.data() + P.o_row0;
  std::vector<int> gidx((size_t)B * feat_rows, -1);
  for (int b = 0; b < B; ++b) {
    const int n = std::min(f_cnt[b], k), npre = call.h_n_prefix ? call.h_n_prefix[b] : 0, npp = npre + P.pm, sh = P.Smax - npp;
    std::vector<int> ord(n);
    for (int e = 0; e < n; ++e) ord[e] = e;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int e) { return f_score[b * k + a] > f_score[b * k + e]; });
    for (int i = 0; i < k; ++i) {
      const size_t o = (size_t)b * k + i;
      if (i >= n) { call.h_n_out[o] = 0; call.h_scores[o] = -INFINITY; continue; }
      const int e = ord[i], len = f_len[b * k + e];
      const size_t src = ((size_t)b * k + e) * Lc;
      call.h_n_out[o] = len;
      call.h_scores[o] = f_score[b * k + e];
      for (int p = 0; p < len; ++p) call.h_out_tokens[o * out_stride + p] = f_tok[src + p];
      if (call.h_pos_scores) {                 // the whole hypothesis: the forced tokens' scores, then the generated ones'
        for (int p = 0; p < npre; ++p) call.h_pos_scores[o * out_stride + p] = prepos[row0[b] + p];
        for (int p = 0; p < len; ++p) call.h_pos_scores[o * out_stride + npre + p] = f_pos[src + p];
      }
      if (i == 0)           // the best hypothesis' decoder states past the prefix pass: fed positions npp .. n_prefix + len - 1
        for (int q = npp; q < npre + len; ++q) gidx[(size_t)b * feat_rows + q] = f_anc[src + sh + q] * Lc + sh + q;
    }
  }
  RET(upload(s, d_gather, gidx));
  hipLaunchKernelGGL(beam_feat_gather_kernel, dim3(B * feat_rows), dim3(256), 0, s, d_gather, feat, D, R * Lc, call.d_feats);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// Batched beam search of the first-pass text decoder (include/streamspeech_hip.h): the search with no prefix anywhere, under the
// constraints of call.h_cons_off when it is given.
int mt_beam_entry(SearchCall& call) {
  RET(read_search_opts(call.opts, call.so));
  const int B = call.B, beam = call.beam;
  if (!call.m || B <= 0 || beam < 1 || beam > kMaxBeam || !call.d_feats || !call.h_out_tokens || !call.h_n_out || !call.h_scores)
    return SS_ERR_ARG;
  const ss_config& c = call.m->cfg;
  // The planner makes the refusals this entry documents next, in their order: the row limit, the vocabulary the top-2k kernel holds
  // in LDS, every utterance's lengths, then its capacity check.  What that check refuses is a subset of what the Lmax check below it
  // refuses, with the same code, so the pair answers as the Lmax check alone would.
  BcPlan P;
  RET(beam_continue_plan(B, beam, call.h_Tp, nullptr, nullptr, call.h_max_len, call.min_len, call.out_stride, call.feat_rows,
                         c.max_tgt_pos, c.tgt_vocab, c.eos, c.pad, 0, P));   // position 0 is a lock-step row at every beam (beam 1 is ss_batch_mt_greedy bit for bit)
  const int Lmax = *std::max_element(call.h_max_len, call.h_max_len + B);
  if (Lmax + 2 > call.feat_rows || Lmax + 4 > c.max_tgt_pos || call.out_stride < Lmax + 1) return SS_ERR_CAPACITY;
  std::vector<int> cons_tab;
  if (call.h_cons_off) {
    RET(cons_table(B, call.h_cons, call.h_cons_off, call.h_cons_end, c.tgt_vocab, c.pad, c.eos, call.h_max_len, cons_tab));
    call.cons_tab = &cons_tab;
  }
  return beam_search(call, P);
}

// The same search behind a forced prefix per utterance (include/streamspeech_hip.h).
int mt_beam_continue_entry(SearchCall& call) {
  RET(read_search_opts(call.opts, call.so));
  if (!call.m || !call.d_enc_out || !call.h_n_prefix || !call.d_feats || !call.h_out_tokens || !call.h_n_out || !call.h_scores)
    return SS_ERR_ARG;
  const ss_config& c = call.m->cfg;
  BcPlan P;
  RET(beam_continue_plan(call.B, call.beam, call.h_Tp, call.h_prefix, call.h_n_prefix, call.h_max_len, call.min_len, call.out_stride,
                         call.feat_rows, c.max_tgt_pos, c.tgt_vocab, c.eos, c.pad, call.beam == 1 ? 1 : 0, P, call.so.ngram));
  return beam_search(call, P);
}

// Sampling (include/streamspeech_hip.h at ss_mt_sample_opts): the sampling refusals, made before the entry's own.
int sample_entry_opts(SearchCall& call, const int64_t* h_keys, const ss_mt_sample_opts* sample) {
  RET(read_sample_opts(sample, h_keys, call.smp));
  if (!call.m) return SS_ERR_ARG;
  if (call.smp.topk > call.m->cfg.tgt_vocab) return SS_ERR_ARG;
  call.h_keys = h_keys;
  return SS_OK;
}

}  // namespace

extern "C" int ss_batch_mt_beam_opts(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                                     const int32_t* h_max_len, int min_len, float unk_penalty, int normalize, int32_t* h_out_tokens,
                                     int out_stride, int32_t* h_n_out, float* h_scores, float* h_pos_scores, float* d_feats,
                                     int feat_rows, const ss_mt_search_opts* opts) {
  SearchCall call{m, stream, B, beam, d_enc_out, h_Tp, nullptr, nullptr, h_max_len, min_len, unk_penalty, normalize, h_out_tokens,
                  out_stride, h_n_out, h_scores, h_pos_scores, d_feats, feat_rows, opts};
  return mt_beam_entry(call);
}

extern "C" int ss_batch_mt_beam(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                                const int32_t* h_max_len, int min_len, float unk_penalty, int normalize, int32_t* h_out_tokens,
                                int out_stride, int32_t* h_n_out, float* h_scores, float* h_pos_scores, float* d_feats,
                                int feat_rows) {
  return ss_batch_mt_beam_opts(m, stream, B, beam, d_enc_out, h_Tp, h_max_len, min_len, unk_penalty, normalize, h_out_tokens,
                               out_stride, h_n_out, h_scores, h_pos_scores, d_feats, feat_rows, nullptr);
}

extern "C" int ss_batch_mt_beam_cons(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                                     const int32_t* h_max_len, int min_len, float unk_penalty, int normalize, int32_t* h_out_tokens,
                                     int out_stride, int32_t* h_n_out, float* h_scores, float* h_pos_scores, float* d_feats,
                                     int feat_rows, const ss_mt_search_opts* opts, const int32_t* h_cons, const int32_t* h_cons_off,
                                     const int32_t* h_cons_end) {
  SearchCall call{m, stream, B, beam, d_enc_out, h_Tp, nullptr, nullptr, h_max_len, min_len, unk_penalty, normalize, h_out_tokens,
                  out_stride, h_n_out, h_scores, h_pos_scores, d_feats, feat_rows, opts, h_cons, h_cons_off, h_cons_end};
  if (!h_cons_off) return SS_ERR_ARG;
  return mt_beam_entry(call);
}

extern "C" int ss_batch_mt_sample(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                                  const int32_t* h_max_len, int min_len, float unk_penalty, int normalize, int32_t* h_out_tokens,
                                  int out_stride, int32_t* h_n_out, float* h_scores, float* h_pos_scores, float* d_feats,
                                  int feat_rows, const ss_mt_search_opts* opts, const int64_t* h_keys,
                                  const ss_mt_sample_opts* sample) {
  SearchCall call{m, stream, B, beam, d_enc_out, h_Tp, nullptr, nullptr, h_max_len, min_len, unk_penalty, normalize, h_out_tokens,
                  out_stride, h_n_out, h_scores, h_pos_scores, d_feats, feat_rows, opts};
  RET(sample_entry_opts(call, h_keys, sample));
  return mt_beam_entry(call);
}

extern "C" int ss_batch_mt_beam_continue_opts(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                                              const int32_t* h_prefix, const int32_t* h_n_prefix, const int32_t* h_max_len,
                                              int min_len, float unk_penalty, int normalize, int32_t* h_out_tokens, int out_stride,
                                              int32_t* h_n_out, float* h_scores, float* h_pos_scores, float* d_feats, int feat_rows,
                                              const ss_mt_search_opts* opts) {
  SearchCall call{m, stream, B, beam, d_enc_out, h_Tp, h_prefix, h_n_prefix, h_max_len, min_len, unk_penalty, normalize, h_out_tokens,
                  out_stride, h_n_out, h_scores, h_pos_scores, d_feats, feat_rows, opts};
  return mt_beam_continue_entry(call);
}

extern "C" int ss_batch_mt_beam_continue(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                                         const int32_t* h_prefix, const int32_t* h_n_prefix, const int32_t* h_max_len, int min_len,
                                         float unk_penalty, int normalize, int32_t* h_out_tokens, int out_stride, int32_t* h_n_out,
                                         float* h_scores, float* h_pos_scores, float* d_feats, int feat_rows) {
  return ss_batch_mt_beam_continue_opts(m, stream, B, beam, d_enc_out, h_Tp, h_prefix, h_n_prefix, h_max_len, min_len, unk_penalty,
                                        normalize, h_out_tokens, out_stride, h_n_out, h_scores, h_pos_scores, d_feats, feat_rows,
                                        nullptr);
}

extern "C" int ss_batch_mt_sample_continue(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                                           const int32_t* h_prefix, const int32_t* h_n_prefix, const int32_t* h_max_len, int min_len,
                                           float unk_penalty, int normalize, int32_t* h_out_tokens, int out_stride, int32_t* h_n_out,
                                           float* h_scores, float* h_pos_scores, float* d_feats, int feat_rows,
                                           const ss_mt_search_opts* opts, const int64_t* h_keys, const ss_mt_sample_opts* sample) {
  SearchCall call{m, stream, B, beam, d_enc_out, h_Tp, h_prefix, h_n_prefix, h_max_len, min_len, unk_penalty, normalize, h_out_tokens,
                  out_stride, h_n_out, h_scores, h_pos_scores, d_feats, feat_rows, opts};
  RET(sample_entry_opts(call, h_keys, sample));
  return mt_beam_continue_entry(call);
}
