// Ragged-batch beam search of the offline first-pass text decoder (ss_batch_mt_beam): B utterances x k hypothesis rows advance in
// lockstep from [</s>].  Reference: SequenceGenerator.generate_decoder (fairseq/examples/speech_to_speech/unity/sequence_generator.py
// :158-525) with BeamSearch.step (fairseq/fairseq/search.py:110-150) and finalize_hypos (fairseq/fairseq/sequence_generator.py:630-760).
//
// Where fairseq reorders every layer's KV cache after each step, hypothesis slot r here writes its K/V row of step s at [r][s] and
// never overwrites it; the ancestry table anc[r][p] names the slot that holds position p of hypothesis r, and the decode attention
// reads keys and values through it (AttnArgs::anc).  A step then moves B*k*L ints instead of layers x B*k*L x 3D floats.  The tokens
// and cumulative scores fed at each step are kept step-major ([step][slot], never overwritten), so a hypothesis' tokens and scores are
// read through the same table.  Per step, after the decoder launches the greedy twin makes as they are:
//   beam_topk_kernel   one workgroup per hypothesis row: log-softmax of the logits, the reference's masks, + cumulative score, the
//                      row's 2k best candidates (the global top 2k over beam x vocab is inside the union of the per-row lists)
//   beam_merge_kernel  one workgroup per utterance: the global top 2k in the reference's order (score, then flattened index), the
//                      finalisation into the utterance's table, the active hypotheses, next tokens / scores / ancestry, done flag
// The host reads the done flags every kCheck steps, as ss_batch_mt_greedy does; nothing else synchronises per step.
#include "model_internal.hpp"

namespace {

constexpr int kMaxBeam = 32, kMaxCand = 2 * kMaxBeam;

// a beats b: higher score, then lower flattened index (torch.topk order); index < 0 = no candidate
__device__ __forceinline__ bool beats(float a, int ia, float b, int ib) {
  return ib < 0 || (ia >= 0 && (a > b || (a == b && ia < ib)));
}

// Row r = b*k + j of the logits -> its 2k best (score, token), score = masked log-softmax + cumulative score of the hypothesis.
// Log-softmax numerics of log_softmax_kernel (elementwise.hip).  Masks in the reference's order (unity/sequence_generator.py:290-327):
// NaN -> -inf, pad -inf, unk -= unk_penalty, step >= max_len: all but </s> -inf, step < min_len: </s> -inf.
__global__ __launch_bounds__(256) void beam_topk_kernel(const float* __restrict__ logits, int V, int k, int step, int min_len,
                                                        const int* __restrict__ max_len, const int* __restrict__ done,
                                                        const float* __restrict__ cum, int pad, int unk, int eos, float unk_pen,
                                                        float* __restrict__ cand_s, int* __restrict__ cand_t) {
  extern __shared__ float vals[];                  // [V] candidate scores of the row; NaN = already taken
  __shared__ float sa[4];
  __shared__ int si[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int row = blockIdx.x, b = row / k, j = row - b * k;
  if (done[b] || (step == 0 && j != 0)) return;    // step 0: only beam 0 of each utterance takes part (lprobs[:, ::beam])
  const float* r = logits + (size_t)row * V;
  float mx = -INFINITY;
  for (int n = t; n < V; n += 256) mx = fmaxf(mx, r[n]);
  mx = wave_max(mx);
  if (lane == 0) sa[wave] = mx;
  __syncthreads();
  mx = fmaxf(fmaxf(sa[0], sa[1]), fmaxf(sa[2], sa[3]));
  __syncthreads();
  float sum = 0.f;
  for (int n = t; n < V; n += 256) sum += expf(r[n] - mx);
  sum = wave_sum(sum);
  if (lane == 0) sa[wave] = sum;
  __syncthreads();
  const float lse = logf((sa[0] + sa[1]) + (sa[2] + sa[3]));
  const bool at_max = step >= max_len[b];
  const float c = cum[row];
  float best = 0.f;
  int bi = -1;
  for (int n = t; n < V; n += 256) {
    float v = (r[n] - mx) - lse;
    if (v != v) v = -INFINITY;
    if (n == pad) v = -INFINITY;
    if (n == unk) v -= unk_pen;
    if (at_max && n != eos) v = -INFINITY;
    if (step < min_len && n == eos) v = -INFINITY;
    if (step > 0) v = v + c;
    vals[n] = v;
    if (beats(v, n, best, bi)) { best = v; bi = n; }
  }
  const int nc = min(2 * k, V - 1);
  for (int q = 0; q < nc; ++q) {
    float wb = best;
    int wi = bi;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ob = __shfl_xor(wb, o, 64);
      const int oi = __shfl_xor(wi, o, 64);
      if (beats(ob, oi, wb, wi)) { wb = ob; wi = oi; }
    }
    __syncthreads();                               // the previous round's readers of sa / si are done
    if (lane == 0) { sa[wave] = wb; si[wave] = wi; }
    __syncthreads();
    wb = sa[0]; wi = si[0];
    for (int w = 1; w < 4; ++w)
      if (beats(sa[w], si[w], wb, wi)) { wb = sa[w]; wi = si[w]; }
    if (t == 0) { cand_s[(size_t)row * kMaxCand + q] = wb; cand_t[(size_t)row * kMaxCand + q] = wi; }
    if (wi >= 0 && (wi & 255) == t) {              // the owner drops the winner and rescans its columns
      vals[wi] = __int_as_float(0x7fc00000);
      best = 0.f; bi = -1;
      for (int n = t; n < V; n += 256) {
        const float v = vals[n];
        if (v == v && beats(v, n, best, bi)) { best = v; bi = n; }
      }
    }
  }
}

struct BeamState {
  int* tok;        // [Lc + 1][R] token fed at position p by slot r
  float* cum;      // [Lc + 1][R] cumulative score of the hypothesis fed at position p by slot r
  int* anc;        // [2][R][Lc]  ping-pong ancestry: anc[s & 1] is read at step s
  float* cand_s;   // [R][kMaxCand]
  int* cand_t;     // [R][kMaxCand]
  int* ignore;     // [R] cands_to_ignore of the reference (per utterance, per candidate position < k)
  int* done;       // [B]
  int* max_len;    // [B]
  // finalised table: count [B], score [B][k] (normalised if asked), length [B][k] (tokens incl. the final </s>),
  // tokens / positional scores / ancestry [B][k][Lc]
  int* fin_cnt; float* fin_score; int* fin_len; int* fin_tok; float* fin_pos; int* fin_anc;
};

// One workgroup per utterance: merge the k sorted per-row lists into the global top 2k, then the step logic of
// unity/sequence_generator.py:329-470 and finalize_hypos.
__global__ __launch_bounds__(256) void beam_merge_kernel(BeamState st, int k, int R, int Lc, int V, int step, int eos, int normalize) {
  __shared__ float ms[kMaxBeam * kMaxCand];
  __shared__ int mt[kMaxBeam * kMaxCand];
  __shared__ float sel_s[kMaxCand];
  __shared__ int sel_t[kMaxCand], sel_beam[kMaxCand];
  __shared__ int fin_c[kMaxBeam], fin_e[kMaxBeam], act_c[kMaxBeam];
  __shared__ int eosm[kMaxCand], f[kMaxBeam];
  __shared__ int n_fin, is_done;
  const int t = threadIdx.x, b = blockIdx.x, r0 = b * k;
  const int* anc_cur = st.anc + (size_t)(step & 1) * R * Lc;
  int* anc_nxt = st.anc + (size_t)((step + 1) & 1) * R * Lc;
  int* tok_nxt = st.tok + (size_t)(step + 1) * R;
  float* cum_nxt = st.cum + (size_t)(step + 1) * R;
  if (st.done[b]) {                  // finished utterance: its rows keep decoding (lockstep) -- keep their tables valid, nothing else
    for (int i = t; i < k * (step + 2); i += 256) {
      const int j = i / (step + 2), p = i - j * (step + 2);
      anc_nxt[(size_t)(r0 + j) * Lc + p] = p <= step ? anc_cur[(size_t)(r0 + j) * Lc + p] : r0 + j;
    }
    if (t < k) { tok_nxt[r0 + t] = eos; cum_nxt[r0 + t] = 0.f; }
    return;
  }
  const int nl = step == 0 ? 1 : k, nc = 2 * k;
  for (int i = t; i < nl * nc; i += 256) {
    const int l = i / nc, q = i - l * nc;
    ms[i] = st.cand_s[(size_t)(r0 + l) * kMaxCand + q];
    mt[i] = st.cand_t[(size_t)(r0 + l) * kMaxCand + q];
  }
  __syncthreads();
  // rank of candidate (list l, position q) = q + the entries of the other lists that beat it; lists are sorted, so each count is a
  // binary search.  A list below l wins ties (lower flattened index), a list above loses them.
  for (int i = t; i < nl * nc; i += 256) {
    const int l = i / nc, q = i - l * nc;
    const float x = ms[i];
    int rank = q;
    for (int l2 = 0; l2 < nl && rank < nc; ++l2) {
      if (l2 == l) continue;
      const float* L = ms + l2 * nc;
      int lo = 0, hi = nc;                         // count of entries e with (l2 < l ? e >= x : e > x)
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (l2 < l ? L[mid] >= x : L[mid] > x) lo = mid + 1; else hi = mid;
      }
      rank += lo;
    }
    if (rank < nc) { sel_s[rank] = x; sel_t[rank] = mt[i]; sel_beam[rank] = l; }
  }
  __syncthreads();
  if (t == 0) {
    // finalisation: </s> candidates among the first k, finite, not ignored (unity/sequence_generator.py:345-372)
    for (int q = 0; q < nc; ++q) {
      eosm[q] = sel_t[q] == eos && sel_s[q] != -INFINITY;
      if (q < k && st.ignore[r0 + q]) eosm[q] = 0;
    }
    int cnt = st.fin_cnt[b], nf = 0;
    for (int q = 0; q < k; ++q)
      if (eosm[q] && cnt < k) {
        fin_c[nf] = q; fin_e[nf] = cnt; ++nf; ++cnt;
        st.fin_score[b * k + cnt - 1] = normalize ? sel_s[q] / (float)(step + 1) : sel_s[q];
        st.fin_len[b * k + cnt - 1] = step + 1;
      }
    bool any = false;
    for (int q = 0; q < k; ++q) any = any || eosm[q];
    st.fin_cnt[b] = cnt;
    n_fin = nf;
    const int dn = (any && (cnt == k || step == st.max_len[b])) || step >= st.max_len[b];   // is_finished (sequence_generator.py:762)
    is_done = dn;
    st.done[b] = dn;
    // active hypotheses: the first k candidates that are neither </s> nor ignored, then the others in order (topk of active_mask)
    int na = 0;
    for (int q = 0; q < nc && na < k; ++q)
      if (!(q < k ? (st.ignore[r0 + q] || eosm[q]) : eosm[q])) act_c[na++] = q;
    for (int q = 0; q < na; ++q) f[q] = 0;
    for (int q = 0; q < nc && na < k; ++q)
      if (q < k ? (st.ignore[r0 + q] || eosm[q]) : eosm[q]) { f[na] = 1; act_c[na++] = q; }
    if (!dn)
      for (int q = 0; q < k; ++q) st.ignore[r0 + q] = f[q];
  }
  __syncthreads();
  // finalised entries: tokens 1..step and </s>, positional scores (differences of the cumulative score), ancestry snapshot
  for (int e = 0; e < n_fin; ++e) {
    const int q = fin_c[e], slot = fin_e[e], pr = r0 + sel_beam[q];
    const int* a = anc_cur + (size_t)pr * Lc;
    const size_t o = ((size_t)b * k + slot) * Lc;
    for (int p = t; p <= step; p += 256) {
      st.fin_anc[o + p] = a[p];
      st.fin_tok[o + p] = p < step ? st.tok[(size_t)(p + 1) * R + a[p + 1]] : eos;
      const float cur = p < step ? st.cum[(size_t)(p + 1) * R + a[p + 1]] : sel_s[q];
      const float prv = p > 0 ? st.cum[(size_t)p * R + a[p]] : 0.f;
      st.fin_pos[o + p] = p > 0 ? cur - prv : cur;
    }
  }
  if (is_done) {                     // as for a finished utterance above: valid tables for the lockstep rows
    for (int i = t; i < k * (step + 2); i += 256) {
      const int j = i / (step + 2), p = i - j * (step + 2);
      anc_nxt[(size_t)(r0 + j) * Lc + p] = p <= step ? anc_cur[(size_t)(r0 + j) * Lc + p] : r0 + j;
    }
    if (t < k) { tok_nxt[r0 + t] = eos; cum_nxt[r0 + t] = 0.f; }
    return;
  }
  // next hypotheses: slot j continues candidate act_c[j] -- its ancestry is its parent's plus itself at step + 1
  if (t < k) {
    const int q = act_c[t];
    tok_nxt[r0 + t] = sel_t[q];
    cum_nxt[r0 + t] = sel_s[q];
  }
  for (int i = t; i < k * (step + 2); i += 256) {
    const int j = i / (step + 2), p = i - j * (step + 2);
    const int pr = r0 + sel_beam[act_c[j]];
    anc_nxt[(size_t)(r0 + j) * Lc + p] = p <= step ? anc_cur[(size_t)pr * Lc + p] : r0 + j;
  }
}

// d_feats row i = slot-major state row idx[i]; rows with idx < 0 (past the best hypothesis) are left as they are
__global__ __launch_bounds__(256) void beam_feat_gather_kernel(const int* __restrict__ idx, const float* __restrict__ src, int D,
                                                               int src_rows, float* __restrict__ dst) {
  const int r = idx[blockIdx.x];
  if (r < 0 || r >= src_rows) return;
  for (int c = threadIdx.x; c < D; c += 256) dst[(size_t)blockIdx.x * D + c] = src[(size_t)r * D + c];
}

}  // namespace

// Batched beam search of the first-pass text decoder (include/streamspeech_hip.h).
extern "C" int ss_batch_mt_beam(ss_model* m, void* stream, int B, int beam, const float* d_enc_out, const int32_t* h_Tp,
                                const int32_t* h_max_len, int min_len, float unk_penalty, int normalize, int32_t* h_out_tokens,
                                int out_stride, int32_t* h_n_out, float* h_scores, float* h_pos_scores, float* d_feats,
                                int feat_rows) {
  if (!m || B <= 0 || beam < 1 || beam > kMaxBeam || !d_feats || !h_out_tokens || !h_n_out || !h_scores) return SS_ERR_ARG;
  if ((long)B * beam > 256) return SS_ERR_CAPACITY;              // the row limit of the greedy twin (segment tables of the slab kernels)
  const ss_config& c = m->cfg;
  const int D = c.dec_dim, F = c.dec_ffn, V = c.tgt_vocab, H = c.dec_heads, k = beam, R = B * beam;
  if (V < 2 * k + 1 || (size_t)V * sizeof(float) > 65536) return SS_ERR_ARG;   // the top-2k kernel holds a row in LDS
  int Lmax = 0;
  for (int b = 0; b < B; ++b) {
    if (h_Tp[b] <= 0 || h_max_len[b] < 0 || min_len > h_max_len[b]) return SS_ERR_ARG;
    Lmax = std::max(Lmax, h_max_len[b]);
  }
  const int Lc = Lmax + 2;
  if (Lc > feat_rows || Lc + 2 > c.max_tgt_pos || out_stride < Lmax + 1) return SS_ERR_CAPACITY;
  SkScope sk_scope(m->sc->skws);
  CanonScope canon_scope(m->pack_invariant ? CANON_SEQ : CANON_NONE);
  hipStream_t s = (hipStream_t)stream;
  const Offsets oe = prefix(h_Tp, B);
  // ---- scratch: everything booked before the first launch ----
  const size_t n_tok = (size_t)(Lc + 1) * R, n_anc = (size_t)2 * R * Lc, n_cand = (size_t)R * kMaxCand, n_fin = (size_t)B * k * Lc;
  const size_t n_fin_words = B + 2 * (size_t)B * k + 3 * n_fin;
  const size_t n_state = 2 * n_tok + n_anc + 2 * n_cand + R + 2 * (size_t)B + n_fin_words;
  RET(m->sc->mt_cross.ensure((size_t)c.mt_layers * oe.total * 2 * D * sizeof(float)));
  RET(m->sc->bmt_self.ensure((size_t)c.mt_layers * R * Lc * 3 * D * sizeof(float)));
  RET(m->sc->bmb_feat.ensure((size_t)R * Lc * D * sizeof(float)));
  RET(m->sc->mt_ws.ensure(((size_t)R * (3 * D + F + V)) * sizeof(float)));
  RET(m->sc->bmb_state.ensure(n_state * sizeof(int)));
  // int tables: cross segs [R][4], self segs per step [Lc][R][4], feature gather [B][feat_rows]
  RET(m->sc->seg_buf.ensure((4 * (size_t)R + (size_t)Lc * 4 * R + (size_t)B * feat_rows) * sizeof(int)));

  for (int l = 0; l < c.mt_layers; ++l)
    RET(linear(s, d_enc_out, c.enc_dim, oe.total, m->mt[l].cross_kv, 2 * D, c.enc_dim,
               m->sc->mt_cross.f() + (size_t)l * oe.total * 2 * D, 2 * D));
  float* feat = m->sc->bmb_feat.f();           // [R][Lc][D] post-LN decoder states of every slot and step
  float* x = m->sc->mt_ws.f();
  float* h = x + (size_t)R * D;
  float* q2 = h + (size_t)R * D;
  float* ff = q2 + (size_t)R * D;
  float* logits = ff + (size_t)R * F;
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
  int* fin_base = w;
  st.fin_cnt = w; w += B;
  st.fin_score = (float*)w; w += (size_t)B * k;
  st.fin_len = w; w += (size_t)B * k;
  st.fin_tok = w; w += n_fin;
  st.fin_pos = (float*)w; w += n_fin;
  st.fin_anc = w; w += n_fin;
  int* d_cross = (int*)m->sc->seg_buf.p;
  int* d_self = d_cross + 4 * R;
  int* d_gather = d_self + (size_t)Lc * 4 * R;
  SS_HIP_CHECK(hipMemsetAsync(m->sc->bmb_state.p, 0, n_state * sizeof(int), s));   // slot 0 / score 0 / nothing finalised everywhere
  {
    std::vector<int> t0(R, c.eos), a0((size_t)R * Lc), ml(h_max_len, h_max_len + B), cs(4 * (size_t)R), ss((size_t)Lc * 4 * R);
    for (int r = 0; r < R; ++r) {
      const int b = r / k;
      std::fill(a0.begin() + (size_t)r * Lc, a0.begin() + (size_t)(r + 1) * Lc, r);
      cs[4 * r] = r; cs[4 * r + 1] = 1; cs[4 * r + 2] = oe.off[b]; cs[4 * r + 3] = h_Tp[b];
    }
    for (int p = 0; p < Lc; ++p)
      for (int r = 0; r < R; ++r) {
        int* e = &ss[((size_t)p * R + r) * 4];
        e[0] = r; e[1] = 1; e[2] = 0; e[3] = p + 1;
      }
    RET(upload(s, st.tok, t0)); RET(upload(s, st.max_len, ml)); RET(upload(s, d_cross, cs)); RET(upload(s, d_self, ss));
    RET(upload(s, st.anc, a0));      // anc[0][r][*] = r: position 0 of every hypothesis is its own row
  }
  std::vector<int> host_done(B, 0);
  int step = 0;
  constexpr int kCheck = 4;
  CanonScope decode_scope(m->pack_invariant ? CANON_SMALLM : CANON_NONE);   // the greedy twin's decode-row GEMM form
  while (true) {
    RET(launch_embed_tokens(st.tok + (size_t)step * R, m->mt_emb, m->mt_pos, sqrtf((float)D), step + c.pad + 1, x, R, D, s, 0, -1, V));
    for (int l = 0; l < c.mt_layers; ++l) {
      float* cache = m->sc->bmt_self.f() + (size_t)l * R * Lc * 3 * D;
      float* rows = cache + (size_t)step * 3 * D;                    // slot r at + r*Lc*3D: written once, never reordered
      AttnArgs at;
      at.Q = rows; at.ldq = Lc * 3 * D; at.K = cache + D; at.V = cache + 2 * D; at.ldk = at.ldv = 3 * D;
      at.O = h; at.ldo = D; at.H = H; at.scale = 1.f; at.causal = 0;
      at.segs = d_self + (size_t)step * 4 * R; at.nseg = R; at.max_q = 1;
      at.anc = st.anc + (size_t)(step & 1) * R * Lc; at.anc_ld = Lc; at.anc_slots = R;
      AttnArgs ac;
      ac.Q = q2; ac.ldq = D; ac.K = m->sc->mt_cross.f() + (size_t)l * oe.total * 2 * D; ac.V = ac.K + D; ac.ldk = ac.ldv = 2 * D;
      ac.O = h; ac.ldo = D; ac.H = H; ac.scale = 1.f; ac.segs = d_cross; ac.nseg = R; ac.max_q = 1;
      RET(dec_layer_ex(s, c, m->mt[l], x, R, rows, Lc * 3 * D, at, &ac, h, q2, ff));
    }
    float* frow = feat + (size_t)step * D;
    RET(launch_layernorm(x, D, frow, Lc * D, m->mt_ln.g, m->mt_ln.b, R, D, 1e-5f, s));
    Lin proj{m->mt_emb, nullptr};
    RET(linear(s, frow, Lc * D, R, proj, V, D, logits, V));
    hipLaunchKernelGGL(beam_topk_kernel, dim3(R), dim3(256), V * sizeof(float), s, logits, V, k, step, min_len, st.max_len,
                       st.done, st.cum + (size_t)step * R, c.pad, c.unk, c.eos, unk_penalty, st.cand_s, st.cand_t);
    SS_LAUNCH_CHECK();
    hipLaunchKernelGGL(beam_merge_kernel, dim3(B), dim3(256), 0, s, st, k, R, Lc, V, step, c.eos, normalize ? 1 : 0);
    SS_LAUNCH_CHECK();
    const bool last = step >= Lmax;            // every utterance is done at its max_len step
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
  SS_HIP_CHECK(hipMemcpyAsync(fin.data(), fin_base, n_fin_words * sizeof(int), hipMemcpyDeviceToHost, s));
  SS_HIP_CHECK(hipStreamSynchronize(s));
  const int* f_cnt = fin.data();
  const float* f_score = reinterpret_cast<const float*>(f_cnt + B);
  const int* f_len = f_cnt + B + (size_t)B * k;
  const int* f_tok = f_len + (size_t)B * k;
  const float* f_pos = reinterpret_cast<const float*>(f_tok + n_fin);
  const int* f_anc = f_tok + 2 * n_fin;
  std::vector<int> gidx((size_t)B * feat_rows, -1);
  for (int b = 0; b < B; ++b) {
    const int n = std::min(f_cnt[b], k);
    std::vector<int> ord(n);
    for (int e = 0; e < n; ++e) ord[e] = e;
    std::stable_sort(ord.begin(), ord.end(), [&](int a, int e) { return f_score[b * k + a] > f_score[b * k + e]; });
    for (int i = 0; i < k; ++i) {
      const size_t o = (size_t)b * k + i;
      if (i >= n) { h_n_out[o] = 0; h_scores[o] = -INFINITY; continue; }
      const int e = ord[i], len = f_len[b * k + e];
      const size_t src = ((size_t)b * k + e) * Lc;
      h_n_out[o] = len;
      h_scores[o] = f_score[b * k + e];
      for (int p = 0; p < len; ++p) h_out_tokens[o * out_stride + p] = f_tok[src + p];
      if (h_pos_scores)
        for (int p = 0; p < len; ++p) h_pos_scores[o * out_stride + p] = f_pos[src + p];
      if (i == 0)           // the best hypothesis' decoder states: </s> + its tokens without the final </s>
        for (int p = 0; p < len; ++p) gidx[(size_t)b * feat_rows + p] = f_anc[src + p] * Lc + p;
    }
  }
  RET(upload(s, d_gather, gidx));
  hipLaunchKernelGGL(beam_feat_gather_kernel, dim3(B * feat_rows), dim3(256), 0, s, d_gather, feat, D, R * Lc, d_feats);
  SS_LAUNCH_CHECK();
  return SS_OK;
}
