// Op-level unit-test entry points (ss_op_*), test / A-B hooks (ss_debug_*) and the profiler's C ABI (ss_prof_*).
#include "model_internal.hpp"
#include "ctc_align.hpp"
#include "ctc_beam.hpp"

// =================================================================================================
// op-level entry points
// =================================================================================================
// unit-test path of the Winograd form (the model makes the transformed weights once per context): made here per call
// (one buffer per stream of the calling thread: a re-pack for a launch on stream B must not overwrite the weights a kernel
//  queued on stream A is still reading -- ADVICE r4)
static int op_bind_wino(GemmArgs& a, void* stream) {
  static thread_local std::map<hipStream_t, DevBuf> wino_tmps;
  DevBuf& wino_tmp = wino_tmps[(hipStream_t)stream];
  const int N = a.N, Cin = a.Cin, taps = a.taps;
  if ((conv_c64w_enabled() && N == 64 && Cin == 64 && taps >= 3 && conv_c64_eligible(a)) ||
      (conv_c128w_enabled() && N == 128 && Cin == 128 && taps >= 3 && a.same_rows && !a.glu) ||
      (conv_c256w_enabled() && N == 256 && Cin == 256 && taps >= 3 && a.same_rows && !a.glu) ||
      (conv_c32w_enabled() && N == 32 && Cin == 32 && taps >= 3 && conv_c32_eligible(a))) {
    RET(wino_tmp.ensure((size_t)N * ((taps + 2) / 3) * 4 * N * sizeof(float)));
    RET(launch_wino_pack(a.W, wino_tmp.f(), N, taps, (hipStream_t)stream));
    a.Wwino = wino_tmp.f();
  }
  return SS_OK;
}

extern "C" int ss_op_conv_gemm(void* stream, const float* dA, int lda, const float* dW, const float* dbias,
                               const float* dR, int ldr, const float* dR2, int ldr2, float* dC, int ldc, int M,
                               int N, int Cin, int taps, int dil, int stride, int pad, int in_len, int chunk,
                               int in_act, float in_slope, int act, float alpha, float div, int glu) {
  GemmArgs a;
  a.A = dA; a.lda = lda; a.W = dW; a.bias = dbias; a.R = dR; a.ldr = ldr; a.R2 = dR2; a.ldr2 = ldr2; a.C = dC; a.ldc = ldc;
  a.M = M; a.N = N; a.Cin = Cin; a.taps = taps; a.dil = dil; a.stride = stride; a.pad = pad; a.in_len = in_len;
  a.chunk = chunk; a.in_act = in_act; a.in_slope = in_slope; a.act = act; a.alpha = alpha; a.div = div; a.glu = glu;
  a.same_rows = (stride == 1 && M == in_len) ? 1 : 0;
  RET(op_bind_wino(a, stream));
  return launch_conv_gemm(a, (hipStream_t)stream);
}

// every field of GemmArgs a caller of the conv launcher can set, as the caller set it (ragged packs, the pre-activated twin, the
// epilogue slope, same_rows): what launch_conv_gemm answers is what the caller sees.  The Winograd weight pack is made per call, as above.
static void op_fill_conv(GemmArgs& a, const ss_op_conv_args* x) {
  a.A = x->A; a.W = x->W; a.bias = x->bias; a.R = x->R; a.R2 = x->R2; a.C = x->C; a.C2 = x->C2;
  a.lda = x->lda; a.ldc = x->ldc; a.ldr = x->ldr; a.ldr2 = x->ldr2; a.ldc2 = x->ldc2;
  a.M = x->M; a.N = x->N; a.Cin = x->Cin; a.taps = x->taps; a.dil = x->dil; a.stride = x->stride; a.pad = x->pad;
  a.in_len = x->in_len; a.chunk = x->chunk;
  a.in_act = x->in_act; a.in_slope = x->in_slope; a.act = x->act; a.act_slope = x->act_slope; a.alpha = x->alpha; a.div = x->div;
  a.c2_slope = x->c2_slope; a.glu = x->glu;
  a.segs = x->segs; a.nseg = x->nseg; a.max_seg_out = x->max_seg_out; a.same_rows = x->same_rows;
}
extern "C" int ss_op_conv_gemm_ex(void* stream, const ss_op_conv_args* x) {
  if (!x) return SS_ERR_ARG;
  GemmArgs a;
  op_fill_conv(a, x);
  if (a.W && a.N > 0 && a.taps > 0) RET(op_bind_wino(a, stream));
  return launch_conv_gemm(a, (hipStream_t)stream);
}
// ... plus the four fields only the streaming encoder sets: the first row of a single utterance's launch (m_begin), the per-segment
// {first row, chunk} and input pointers of the session pool's ragged subsampler (seg_mb [2 nseg] / seg_A [nseg], device arrays), and
// the arithmetic mode of THIS launch (canon: 0 the calling thread's, 1 CANON_SEQ, 2 CANON_SMALLM)
extern "C" int ss_op_conv_gemm_rows(void* stream, const ss_op_conv_args* x, int m_begin, const int32_t* seg_mb,
                                    const float* const* seg_A, int canon) {
  if (!x || canon < 0 || canon > 2) return SS_ERR_ARG;
  GemmArgs a;
  op_fill_conv(a, x);
  a.m_begin = m_begin; a.seg_mb = seg_mb; a.seg_A = seg_A; a.canon = canon;
  if (a.W && a.N > 0 && a.taps > 0) RET(op_bind_wino(a, stream));
  return launch_conv_gemm(a, (hipStream_t)stream);
}
// The fused ResBlock half and the fused ResBlock of the narrow vocoder stages (conv_slab.hip, resblock.hip): the launchers with the
// caller's arguments unchanged.  W1 / B1 / W2 / B2 / dil of the ResBlock: HOST arrays of three (device pointers / dilations).
extern "C" int ss_op_conv_pair(void* stream, const float* dA, int lda, const float* dW1, const float* db1, const float* dW2,
                               const float* db2, float* dC, int ldc, const float* dR2, int ldr2, float div, float* dC2, int ldc2,
                               float c2_slope, int Cch, int taps, int dil, int M, int in_len, float slope, const int32_t* d_segs,
                               int nseg) {
  return launch_conv_pair(dA, lda, dW1, db1, dW2, db2, dC, ldc, dR2, ldr2, div, dC2, ldc2, c2_slope, Cch, taps, dil, M, in_len, slope,
                          d_segs, nseg, (hipStream_t)stream);
}
extern "C" int ss_op_resblock_fused(void* stream, const float* dX, int ldx, const float* const* dW1, const float* const* dB1,
                                    const float* const* dW2, const float* const* dB2, const int32_t* dil, float* dY, int ldy,
                                    const float* dR2, int ldr2, float div, int Cch, int taps, int M, float slope,
                                    const int32_t* d_segs, int nseg) {
  if (!dW1 || !dB1 || !dW2 || !dB2 || !dil) return SS_ERR_ARG;      // (host arrays: the launcher reads them)
  return launch_resblock_fused(dX, ldx, dW1, dB1, dW2, dB2, dil, dY, ldy, dR2, ldr2, div, Cch, taps, M, slope, d_segs, nseg,
                               (hipStream_t)stream);
}
// Test hook of the slab kernels' shared walk (slab_common.hpp): grid > 0 caps their persistent grids (every workgroup then walks many
// blocks, across utterance edges, whatever the row count), 0 lifts the cap; min_rows >= 0 replaces the five row thresholds below which
// conv_c16 / c32 / c64 and the wide Winograd forms refuse a launch, min_rows < 0 puts the defaults back.
extern "C" int ss_debug_slab(int grid, long long min_rows) {
  if (grid < 0) return SS_ERR_ARG;
  slab_debug(grid, min_rows);
  return SS_OK;
}

// FP16 form of a wide-stage ResBlock conv (conv_f16.hip; the model packs the weights once per blob, here per call into one buffer per
// stream of the calling thread, as the Winograd form above)
extern "C" int ss_op_conv_f16(void* stream, const float* dA, const float* dW, const float* dbias, const float* dR, const float* dR2,
                              float* dC, float* dC2, int M, int Cch, int taps, int dil, int in_act, float in_slope, int act, float div,
                              const int32_t* d_segs, int nseg) {
  if (!dA || !dW || !dC || M <= 0 || taps < 1 || dil < 1 || nseg < 0 || (nseg > 0 && !d_segs)) return SS_ERR_ARG;
  if (!(Cch == 64 || Cch == 128 || Cch == 256)) return SS_ERR_ARG;
  static thread_local std::map<hipStream_t, DevBuf> f16_tmps;
  DevBuf& wh = f16_tmps[(hipStream_t)stream];
  RET(wh.ensure(f16_pack_halves(Cch, taps) * sizeof(uint16_t)));
  RET(launch_f16_pack(dW, wh.p, Cch, taps, (hipStream_t)stream));
  GemmArgs a;
  a.A = dA; a.lda = Cch; a.W = dW; a.Wf16 = wh.p; a.bias = dbias; a.R = dR; a.ldr = Cch; a.R2 = dR2; a.ldr2 = Cch;
  a.C = dC; a.ldc = Cch; a.C2 = dC2; a.ldc2 = Cch; a.c2_slope = 0.1f;
  a.M = M; a.N = Cch; a.Cin = Cch; a.taps = taps; a.dil = dil; a.stride = 1; a.pad = dil * (taps - 1) / 2; a.in_len = M;
  a.same_rows = 1; a.in_act = in_act; a.in_slope = in_slope; a.act = act; a.act_slope = 0.1f; a.div = div;
  a.segs = d_segs; a.nseg = nseg;
  return launch_conv_f16(a, (hipStream_t)stream);
}

extern "C" int ss_debug_last_logits(ss_model* m, void* stream, float* d_out, int64_t cap_floats, int* h_rows, int* h_cols) {
  if (!m || !h_rows || !h_cols) return SS_ERR_ARG;
  *h_rows = m->sc->dbg_rows; *h_cols = m->sc->dbg_cols;
  if (!d_out) return SS_OK;                                   // size query
  if (!m->sc->dbg_logits || cap_floats < (int64_t)m->sc->dbg_rows * m->sc->dbg_cols) return SS_ERR_CAPACITY;
  SS_HIP_CHECK(hipMemcpyAsync(d_out, m->sc->dbg_logits, (size_t)m->sc->dbg_rows * m->sc->dbg_cols * sizeof(float), hipMemcpyDeviceToDevice,
                              (hipStream_t)stream));
  return SS_OK;
}

extern "C" int ss_op_ffn_fused(void* stream, const float* dX, int ldx, float* dY, int ldy, const float* ln_g, const float* ln_b,
                               const float* dW1, const float* db1, const float* dW2, const float* db2, float alpha,
                               const float* ln2_g, const float* ln2_b, int M, int D, int F) {
  return launch_ffn_fused(dX, ldx, dY, ldy, ln_g, ln_b, dW1, db1, dW2, db2, alpha, ln2_g, ln2_b, M, D, F, (hipStream_t)stream,
                          canon_mode() == CANON_SEQ);
}
// Test hook: the arithmetic mode of the ss_op_* entry points called from this thread (0 fastest kernel per shape, 1 the pack-invariant
// one-chain form, 2 the fixed small-M form of the lock-step decode rows); the model entry points set their own.
extern "C" int ss_debug_canon(int mode) {
  if (mode < 0 || mode > 2) return SS_ERR_ARG;
  canon_debug_set(mode);
  return SS_OK;
}
extern "C" int ss_op_ln_linear(void* stream, const float* dX, int ldx, const float* ln_g, const float* ln_b, const float* dW,
                               const float* dbias, const float* dR, int ldr, float* dC, int ldc, int M, int N, int K, int act,
                               float alpha, int glu) {
  GemmArgs a;
  a.A = dX; a.lda = ldx; a.W = dW; a.bias = dbias; a.R = dR; a.ldr = ldr; a.C = dC; a.ldc = ldc;
  a.M = M; a.N = N; a.Cin = K; a.in_len = M; a.act = act; a.alpha = alpha; a.glu = glu; a.same_rows = 1;
  a.ln_g = ln_g; a.ln_b = ln_b;
  return launch_conv_gemm(a, (hipStream_t)stream);       // SS_ERR_ARG when no kernel with a LayerNorm prologue takes the shape
}
// ... plus the two fields that entry cannot say: ln_out (the normalised rows as a second output, row stride K: the last launch of an MT
// decode step) and the arithmetic mode of THIS launch (canon, as ss_op_conv_gemm_rows).  ln_g / ln_b may both be null: a plain linear,
// which has no normalised rows to publish
extern "C" int ss_op_ln_linear_ex(void* stream, const float* dX, int ldx, const float* ln_g, const float* ln_b, float* ln_out,
                                  const float* dW, const float* dbias, const float* dR, int ldr, float* dC, int ldc, int M, int N, int K,
                                  int act, float alpha, int glu, int canon) {
  if (canon < 0 || canon > 2 || (ln_g == nullptr) != (ln_b == nullptr) || (ln_out && !ln_g)) return SS_ERR_ARG;
  GemmArgs a;
  a.A = dX; a.lda = ldx; a.W = dW; a.bias = dbias; a.R = dR; a.ldr = ldr; a.C = dC; a.ldc = ldc;
  a.M = M; a.N = N; a.Cin = K; a.in_len = M; a.act = act; a.alpha = alpha; a.glu = glu; a.same_rows = 1;
  a.ln_g = ln_g; a.ln_b = ln_b; a.ln_out = ln_out; a.canon = canon;
  return launch_conv_gemm(a, (hipStream_t)stream);
}
// enable 0 / 1: the stage on conv_sk2<64> / on the slab kernels; 4 / 5: its Winograd form (conv_c64w.hip) off / on (the slab kernels stay on);
// 6 / 7: the 128-channel stage on conv_sk2<128> / on the Winograd slab kernel
extern "C" int ss_debug_conv_c64(int enable) {
  if (enable == 4 || enable == 5) { conv_c64w_debug(enable == 5); return SS_OK; }
  if (enable == 6 || enable == 7) { conv_c128w_debug(enable == 7); return SS_OK; }     // the 128-channel stage: conv_sk2<128> + twins / Winograd slab
  if (enable == 8 || enable == 9) { conv_c256w_debug(enable == 9); return SS_OK; }     // the 256-channel stage: conv_sk2<128> + twins / Winograd slab (two phases)
  conv_c64_debug(enable);
  return SS_OK;
}
// block height of the 256-channel Winograd form (conv_c64w.hip): 128 / 256 rows, 0 puts the default back
extern "C" int ss_debug_conv_c256_rows(int rows) { return conv_c256w_rows_debug(rows); }
extern "C" int ss_debug_conv_c32(int enable) {      // 0 / 1: the per-conv slab kernel off / on; 4 / 5: its Winograd form off / on
  if (enable == 4 || enable == 5) { conv_c32w_debug(enable == 5); return SS_OK; }
  conv_c32_debug(enable);
  return SS_OK;
}
extern "C" int ss_debug_conv_c16(int enable) { conv_c16_debug(enable); return SS_OK; }
extern "C" int64_t ss_debug_enc_step_launches(void) { return (int64_t)enc_step_launch_count(); }
// The booking contract of a scratch set: every buffer is booked under the set's own account, and what the account says is held is what
// the buffers hold.  Outputs are written either way; SS_ERR_ARG when a buffer is booked elsewhere (or nowhere).
extern "C" int ss_debug_scratch_audit(ss_scratch* sc, size_t* booked, size_t* held) {
  if (!sc || !booked || !held) return SS_ERR_ARG;
  size_t sum = 0;
  bool foreign = false;
  for (DevBuf* b : sc->all()) {
    sum += b->bytes;
    if (b->acct != &sc->acct) foreign = true;
  }
  *booked = sc->acct.used;
  *held = sum;
  return foreign ? SS_ERR_ARG : SS_OK;
}
extern "C" int ss_debug_rtlin(int grid, int enable) {
  if (grid < 0) return SS_ERR_ARG;
  rtlin_debug(grid, enable);
  return SS_OK;
}
extern "C" int ss_debug_rtlin_kb(int uw, int order) {
  if (!(uw == 0 || uw == 1 || uw == 2 || uw == 4) || order < -1 || order > 2) return SS_ERR_ARG;
  rtlin_kb_debug(uw, order);
  return SS_OK;
}
extern "C" int ss_debug_rtlin_kb_last(int32_t out[4]) {
  if (!out) return SS_ERR_ARG;
  int v[4];
  rtlin_kb_last(v);
  for (int i = 0; i < 4; ++i) out[i] = v[i];
  return SS_OK;
}
// A/B + test hooks of the two "work nobody reads" paths: on = 1 / 0 the unit decoder's first-layer QKV over the distinct rows / over
// all upsampled rows (batch.hip); dense = 1 / 0 the fbank mel walk over all 257 bins with in-kernel twiddles / over the model's
// tables (fbank.hip).  -1 puts the process default (SS_UNIT_L0_DISTINCT, SS_FBANK_DENSE) back.
extern "C" int ss_debug_unit_l0_distinct(int on) {
  if (on < -1 || on > 1) return SS_ERR_ARG;
  dispatch_edit([on](Dispatch& d) { d.unit_l0_distinct = on < 0 ? (getenv("SS_UNIT_L0_DISTINCT") ? atoi(getenv("SS_UNIT_L0_DISTINCT")) != 0 : 1) : on; });
  return SS_OK;
}
extern "C" int ss_debug_fbank_dense(int dense) {
  if (dense < -1 || dense > 1) return SS_ERR_ARG;
  dispatch_edit([dense](Dispatch& d) { d.fbank_dense = dense < 0 ? (getenv("SS_FBANK_DENSE") ? atoi(getenv("SS_FBANK_DENSE")) != 0 : 0) : dense; });
  return SS_OK;
}
extern "C" int ss_debug_ffn(int grid, int row_tiles_per_wave, int enable) {
  if (grid < 0 || row_tiles_per_wave < -1 || row_tiles_per_wave > 4) return SS_ERR_ARG;     // row tiles: 1..4 force, 0 process default, -1 keep
  ffn_fused_debug_grid(grid);
  ffn_fused_debug_rows(row_tiles_per_wave);
  if (enable >= 0) dispatch_edit([enable](Dispatch& d) { d.ffn_fusion = enable ? 1 : 0; });
  return SS_OK;
}

extern "C" int ss_op_layernorm(void* stream, const float* dx, int ldx, float* dy, int ldy, const float* dg,
                               const float* db, int M, int D, float eps) {
  return launch_layernorm(dx, ldx, dy, ldy, dg, db, M, D, eps, (hipStream_t)stream);
}

// The decode glue kernels of elementwise.hip, each launcher with the caller's arguments unchanged (tests/test_glue_ops_gpu.py)
extern "C" int ss_op_masked_argmax(void* stream, const float* logits, int ld, int M, int N, int mask0, int mask1, int mask2, int force,
                                   int32_t* ids, const int32_t* row_max_len, int step, int force_id, const int32_t* row_min_len,
                                   int ban_id) {
  return launch_masked_argmax(logits, ld, M, N, mask0, mask1, mask2, force, ids, (hipStream_t)stream, row_max_len, step, force_id,
                              row_min_len, ban_id);
}
extern "C" int ss_op_ctc_collapse(void* stream, const int32_t* raw, int T, int blank, int pad, int32_t* tokens, int32_t* index,
                                  int32_t* count, const int32_t* segs, int nseg) {
  return launch_ctc_collapse(raw, T, blank, pad, tokens, index, count, (hipStream_t)stream, segs, nseg);
}
extern "C" int ss_op_masked_argmax_lprob(void* stream, const float* logits, int ld, int M, int N, int mask0, int mask1, int mask2,
                                         int32_t* ids, float* lprob) {
  return launch_masked_argmax_lprob(logits, ld, M, N, mask0, mask1, mask2, ids, lprob, (hipStream_t)stream);
}
// the token score kernel of ss_batch_mt_score (mt_score.hip); ss_debug_mt_score_form(1) forces its two-read strided form
static int g_mt_score_form = 0;
extern "C" int ss_debug_mt_score_form(int v) { g_mt_score_form = v ? 1 : 0; return SS_OK; }
extern "C" int ss_op_mt_token_scores(void* stream, const float* d_logits, int ld, int rows, int V, const int32_t* d_target,
                                     float* d_stat, int32_t* d_idx) {
  return launch_mt_token_scores(d_logits, ld, rows, V, d_target, d_stat, d_idx, (hipStream_t)stream, g_mt_score_form);
}
extern "C" int ss_op_ctc_collapse_spans(void* stream, const int32_t* raw, const float* lprob, int T, int blank, int pad, int32_t* tokens,
                                        int32_t* index, int32_t* last, float* tok_lprob, int32_t* count, const int32_t* segs, int nseg) {
  return launch_ctc_collapse_spans(raw, lprob, T, blank, pad, tokens, index, last, tok_lprob, count, (hipStream_t)stream, segs, nseg);
}
// the two alignment kernels on the caller's logits; their scratch made here, one pair of buffers per stream of the calling thread
// (as op_bind_wino's: a launch queued on another stream may still be reading the other pair)
extern "C" int ss_op_ctc_align(void* stream, const float* d_logits, int ld, int V, int pad, int B, const int32_t* h_T,
                               const int32_t* h_targets, const int32_t* h_n_targets, ss_ctc_align_result* d_results, int32_t* d_path,
                               int32_t* d_first, int32_t* d_last, float* d_tok_lprob, float* d_frame_lprob) {
  if (!d_logits || ld < V || !d_results) return SS_ERR_ARG;
  CtcAlignPlan plan;
  RET(ctc_align_plan(V, pad, B, h_T, h_targets, h_n_targets, plan));
  if (plan.labels > 0 && (!d_first || !d_last || !d_tok_lprob)) return SS_ERR_ARG;
  static thread_local std::map<hipStream_t, std::pair<DevBuf, DevBuf>> tmps;
  auto& tmp = tmps[(hipStream_t)stream];
  RET(tmp.first.ensure(ctc_align_table_bytes(plan)));
  RET(tmp.second.ensure(plan.work_bytes()));
  return launch_ctc_align(d_logits, ld, V, plan, h_targets, tmp.first.p, tmp.second.p, d_results, d_path, d_first, d_last, d_tok_lprob,
                          d_frame_lprob, (hipStream_t)stream);
}
// the two prefix-search kernels on the caller's logits; scratch as ss_op_ctc_align's.  with_lm: the LM form and its refusals;
// with_bias: a bias form (with a model when lm is given) and its refusals.
static int op_ctc_beam(void* stream, const float* d_logits, int ld, int V, int pad, int unk, int B, const int32_t* h_T, int beam, int cand,
                       int nbest, void* d_hyps, int32_t* d_tokens, int out_stride, float* d_den, int32_t* d_cand_id, bool with_lm,
                       const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts, bool with_bias = false, const ss_ctc_bias* bias = nullptr,
                       const ss_ctc_bias_opts* bopts = nullptr) {
  if (!d_logits || ld < V || !d_hyps || !d_tokens) return SS_ERR_ARG;
  CtcBeamPlan plan;
  RET(ctc_beam_plan(V, B, h_T, beam, cand, nbest, out_stride, plan));
  if (with_bias) RET(ctc_beam_bias_check(bias, V, pad, unk, bopts, lm, opts));
  if (with_lm) RET(ctc_beam_lm_check(lm, V, opts));
  static thread_local std::map<hipStream_t, std::pair<DevBuf, DevBuf>> tmps;
  auto& tmp = tmps[(hipStream_t)stream];
  RET(tmp.first.ensure(ctc_beam_table_bytes(plan)));
  RET(tmp.second.ensure(plan.work_bytes_form((with_lm ? CTC_FORM_LM : 0) | (with_bias ? CTC_FORM_BIAS : 0))));
  return launch_ctc_beam(d_logits, ld, V, pad, unk, plan, tmp.first.p, tmp.second.p, lm, opts, d_hyps, d_tokens, out_stride, d_den,
                         d_cand_id, (hipStream_t)stream, bias, bopts);
}
extern "C" int ss_op_ctc_beam(void* stream, const float* d_logits, int ld, int V, int pad, int unk, int B, const int32_t* h_T, int beam,
                              int cand, int nbest, ss_ctc_beam_hyp* d_hyps, int32_t* d_tokens, int out_stride, float* d_den,
                              int32_t* d_cand_id) {
  return op_ctc_beam(stream, d_logits, ld, V, pad, unk, B, h_T, beam, cand, nbest, d_hyps, d_tokens, out_stride, d_den, d_cand_id, false,
                     nullptr, nullptr);
}
extern "C" int ss_op_ctc_beam_lm(void* stream, const float* d_logits, int ld, int V, int pad, int unk, int B, const int32_t* h_T, int beam,
                                 int cand, int nbest, ss_ctc_beam_lm_hyp* d_hyps, int32_t* d_tokens, int out_stride, float* d_den,
                                 int32_t* d_cand_id, const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts) {
  return op_ctc_beam(stream, d_logits, ld, V, pad, unk, B, h_T, beam, cand, nbest, d_hyps, d_tokens, out_stride, d_den, d_cand_id, true,
                     lm, opts);
}
extern "C" int ss_op_ctc_beam_bias(void* stream, const float* d_logits, int ld, int V, int pad, int unk, int B, const int32_t* h_T,
                                   int beam, int cand, int nbest, ss_ctc_beam_bias_hyp* d_hyps, int32_t* d_tokens, int out_stride,
                                   float* d_den, int32_t* d_cand_id, const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts,
                                   const ss_ctc_bias* bias, const ss_ctc_bias_opts* bias_opts) {
  return op_ctc_beam(stream, d_logits, ld, V, pad, unk, B, h_T, beam, cand, nbest, d_hyps, d_tokens, out_stride, d_den, d_cand_id,
                     lm != nullptr, lm, opts, true, bias, bias_opts);
}
extern "C" int ss_op_ctc_bias_score(void* stream, const ss_ctc_bias* bias, int B, const int32_t* d_tokens, const int32_t* h_n, int finish,
                                    double* d_delta, int32_t* d_state, double* d_sum) {
  if (!bias || B <= 0 || !h_n || !d_sum) return SS_ERR_ARG;
  static thread_local std::map<hipStream_t, DevBuf> tmps;
  DevBuf& tmp = tmps[(hipStream_t)stream];
  RET(tmp.ensure(bias_score_table_bytes(B)));
  return launch_bias_score(bias, B, d_tokens, h_n, finish, d_delta, d_state, d_sum, tmp.p, (hipStream_t)stream);
}
extern "C" int ss_op_ngram_score(void* stream, const ss_ngram_lm* lm, int B, const int32_t* d_tokens, const int32_t* h_n, int with_eos,
                                 double* d_lp, int32_t* d_state) {
  if (!lm || B <= 0 || !h_n || !d_lp) return SS_ERR_ARG;
  static thread_local std::map<hipStream_t, DevBuf> tmps;
  DevBuf& tmp = tmps[(hipStream_t)stream];
  RET(tmp.ensure(ngram_score_table_bytes(B)));
  return launch_ngram_score(lm, B, d_tokens, h_n, with_eos, d_lp, d_state, tmp.p, (hipStream_t)stream);
}
extern "C" int ss_op_dur_predict(void* stream, const float* logdur, const int32_t* forced, int K, int32_t* dur, int32_t* cum,
                                 const int32_t* segs, int nseg) {
  return launch_dur_predict(logdur, forced, K, dur, cum, (hipStream_t)stream, segs, nseg);
}
extern "C" int ss_op_repeat_rows(void* stream, const float* emb, const int32_t* cum, int K, int D, float* out, int F,
                                 const int32_t* segs, int nseg) {
  return launch_repeat_rows(emb, cum, K, D, out, F, (hipStream_t)stream, segs, nseg);
}
extern "C" int ss_op_embed_tokens(void* stream, const int32_t* tok, const float* emb, const float* pos_table, float scale, int pos0,
                                  float* out, int n, int D, int pos_stride, int pad_id, int vocab) {
  return launch_embed_tokens(tok, emb, pos_table, scale, pos0, out, n, D, (hipStream_t)stream, pos_stride, pad_id, vocab);
}
extern "C" int ss_op_embed_tokens_rows(void* stream, const int32_t* tok, const float* emb, const float* pos_table, int pos_rows,
                                       float scale, int pos0, const int32_t* row_pos, float* out, int n, int D, int pad_id, int vocab) {
  return launch_embed_tokens_rows(tok, emb, pos_table, pos_rows, scale, pos0, row_pos, out, n, D, (hipStream_t)stream, pad_id, vocab);
}
extern "C" int ss_op_upsample_add_pos(void* stream, const float* src, int n, int up, const float* pos_row, float pad_value, float* out,
                                      int D) {
  return launch_upsample_add_pos(src, n, up, pos_row, pad_value, out, D, (hipStream_t)stream);
}
extern "C" int ss_op_gather_rows(void* stream, const int32_t* idx, const float* table, int D, float* out, int n, int rows) {
  return launch_gather_rows(idx, table, D, out, n, (hipStream_t)stream, rows);
}
extern "C" int ss_op_scatter_rows(void* stream, const int32_t* dst_row, const float* src, int lds, float* dst, int ldd, int D, int n,
                                  int dst_rows) {
  return launch_scatter_rows(dst_row, src, lds, dst, ldd, D, n, dst_rows, (hipStream_t)stream);
}
extern "C" int ss_op_conv_post_tanh(void* stream, const float* x, int T, int C, const float* w, const float* bias, float slope,
                                    float* wav, const int32_t* segs, int nseg) {
  return launch_conv_post_tanh(x, T, C, w, bias, slope, wav, (hipStream_t)stream, segs, nseg);
}
extern "C" int ss_op_conv_post_tanh_crop(void* stream, const float* x, int C, const float* w, const float* bias, float slope, float* wav,
                                         const int32_t* segs, int nseg, int max_keep) {
  return launch_conv_post_tanh_crop(x, C, w, bias, slope, wav, segs, nseg, max_keep, (hipStream_t)stream);
}
extern "C" int ss_op_spkr_pre_add(void* stream, const float* x, float* y, int ld, int C0, const float* table, const int32_t* spkr,
                                   int spkr0, const int32_t* segs, int nseg, int max_seg_out, int M, int act, float slope) {
  return launch_spkr_pre_add(x, y, ld, C0, table, spkr, spkr0, segs, nseg, max_seg_out, M, act, slope, (hipStream_t)stream);
}

// test ops: one process-wide key-split scratch (callers are serial), counters zero before the first launch
static int op_attn_bind_split(AttnArgs& a) {
  static void* scratch = nullptr;
  if (!scratch) {
    SS_HIP_CHECK(hipMalloc(&scratch, attention_split_bytes()));
    SS_HIP_CHECK(hipMemset(scratch, 0, attention_split_bytes()));
  }
  attention_bind_split(a, scratch);
  return SS_OK;
}

extern "C" int ss_op_attention(void* stream, const float* dQ, int ldq, const float* dK, int ldk, const float* dV,
                               int ldv, float* dO, int ldo, int Tq, int Tk, int H, float scale, int causal, int chunk,
                               const float* dP, int ldp, const float* du, const float* dv) {
  AttnArgs a;
  a.Q = dQ; a.ldq = ldq; a.K = dK; a.ldk = ldk; a.V = dV; a.ldv = ldv; a.O = dO; a.ldo = ldo;
  a.Tq = Tq; a.Tk = Tk; a.H = H; a.scale = scale; a.causal = causal; a.chunk = chunk;
  a.P = dP; a.ldp = ldp; a.bias_u = du; a.bias_v = dv;
  if (dP) RET(op_attn_bind_split(a));
  return launch_attention(a, (hipStream_t)stream);
}

// every field of AttnArgs a caller can set, as the caller set it: what launch_attention answers is what the caller sees
extern "C" int ss_op_attention_ex(void* stream, const ss_op_attn_args* x) {
  if (!x) return SS_ERR_ARG;
  AttnArgs a;
  a.Q = x->Q; a.K = x->K; a.V = x->V; a.O = x->O;
  a.ldq = x->ldq; a.ldk = x->ldk; a.ldv = x->ldv; a.ldo = x->ldo;
  a.Tq = x->Tq; a.Tk = x->Tk; a.H = x->H; a.scale = x->scale;
  a.causal = x->causal; a.chunk = x->chunk; a.q0 = x->q0; a.k_mask_tail = x->k_mask_tail;
  a.P = x->P; a.ldp = x->ldp; a.bias_u = x->bias_u; a.bias_v = x->bias_v;
  a.segs = x->segs; a.nseg = x->nseg; a.max_q = x->max_q; a.p_tmax = x->p_tmax;
  a.seg_tail = x->seg_tail;
  a.no_decode_kernel = x->no_decode_kernel;
  a.anc = x->anc; a.anc_ld = x->anc_ld; a.anc_slots = x->anc_slots;
  if (x->use_split) RET(op_attn_bind_split(a));
  return launch_attention(a, (hipStream_t)stream);
}

extern "C" int ss_op_attention_probs(void* stream, const ss_op_attn_probs_args* x) {
  if (!x) return SS_ERR_ARG;
  AttnProbsArgs a;
  a.Q = x->Q; a.K = x->K; a.ldq = x->ldq; a.ldk = x->ldk; a.H = x->H; a.scale = x->scale;
  a.segs = x->segs; a.nseg = x->nseg; a.q_first = x->q_first; a.row_off = x->row_off;
  a.p_off = reinterpret_cast<const long long*>(x->p_off);
  a.P = x->P; a.peak = x->peak; a.stat = x->stat; a.max_rows = x->max_rows;
  return launch_attention_probs(a, (hipStream_t)stream);
}

extern "C" int ss_op_attention_pool(void* stream, const ss_op_pool_attn_args* x) {
  if (!x) return SS_ERR_ARG;
  PoolAttnArgs a;
  a.Qs = x->Qs; a.cache = x->cache; a.O = x->O;
  a.ld = x->ld; a.ldo = x->ldo; a.slot_rows = x->slot_rows;
  a.P = x->P; a.ldp = x->ldp; a.p_tmax = x->p_tmax;
  a.bias_u = x->bias_u; a.bias_v = x->bias_v;
  a.sess = x->sess; a.qt_pre = x->qt_pre;
  a.nsess = x->nsess; a.qtiles = x->qtiles; a.H = x->H; a.scale = x->scale;
  return launch_attention_pool(a, (hipStream_t)stream);
}

extern "C" int ss_debug_attention_split(int v) { attention_debug_split(v); return SS_OK; }
extern "C" int ss_debug_attention_q16(int v) { attention_debug_q16(v); return SS_OK; }
extern "C" int ss_debug_attention_no_mfma(int v) { attention_debug_no_mfma(v); return SS_OK; }

extern "C" int ss_op_dwconv_bn_silu(void* stream, const float* dx, int ldx, float* dy, int ldy, const float* dwt,
                                    int K, const float* mean, const float* var, const float* gamma,
                                    const float* beta, float eps, int T, int C, int chunk) {
  return launch_dwconv_bn_silu(dx, ldx, dy, ldy, dwt, K, mean, var, gamma, beta, eps, T, C, chunk, (hipStream_t)stream);
}

// ... with the ragged pack (segs: nseg x {row_start, len}, T = the longest len) and the first row of a row range (t_begin)
extern "C" int ss_op_dwconv_bn_silu_ex(void* stream, const float* dx, int ldx, float* dy, int ldy, const float* dwt, int K,
                                       const float* mean, const float* var, const float* gamma, const float* beta, float eps, int T,
                                       int C, int chunk, const int32_t* segs, int nseg, int t_begin) {
  return launch_dwconv_bn_silu(dx, ldx, dy, ldy, dwt, K, mean, var, gamma, beta, eps, T, C, chunk, (hipStream_t)stream, segs, nseg,
                               t_begin);
}

extern "C" int ss_prof_enable(int cls_mask) { prof_enable(cls_mask); return SS_OK; }
extern "C" int ss_prof_enable_hi(int cls_mask) { prof_enable_hi(cls_mask); return SS_OK; }
extern "C" int ss_prof_reset(void) { prof_reset(); return SS_OK; }
extern "C" int ss_prof_read(int cls, double* ms, double* flops, int64_t* launches, double* bytes) {
  long long n = 0;
  int rc = prof_read(cls, ms, flops, &n, bytes);
  if (launches) *launches = n;
  return rc;
}
extern "C" int ss_prof_totals(int cls, double* flops, double* bytes, int64_t* launches) {
  long long n = 0;
  int rc = prof_totals(cls, flops, bytes, &n);
  if (launches) *launches = n;
  return rc;
}
extern "C" int ss_prof_read_issued(int cls, double* issued_flops) { return prof_read_issued(cls, issued_flops); }
extern "C" int ss_prof_shape_log(int on) { prof_shape_log(on); return SS_OK; }
extern "C" int ss_prof_shape_dump(char* buf, int cap) { return prof_shape_dump(buf, cap); }
extern "C" int ss_prof_num_classes(void) { return kNumTileCfg; }
extern "C" const char* ss_prof_class_name(int cls) { return prof_cfg_name(cls); }

extern "C" int ss_debug_force_tile(int bm, int bn, int ks) {
  // 0 heuristic | 1 first-generation stream-K (bn = 8: XCD groups, ks = grid) | 2 no slab kernel | 3 narrow-stage pairs as two
  // launches | 4 second-generation stream-K (ks = grid) | 5 its split-bf16 form | 6 narrow-stage ResBlocks as separate launches |
  // 32 / 64 / 128 a forced tile of the LDS-tiled kernel (tools/conv_bench.py); anything else is a caller's mistake.
  // (Round 3 had booked BOTH the conv_sk2 hook and the ResBlock A/B on 4, so (4, 0, G) never reached the stream-K launcher.)
  if (!(bm >= 0 && bm <= 6) && bm != 32 && bm != 64 && bm != 128) return SS_ERR_ARG;
  if (bm == 6 || bm == 0) dispatch_edit([bm](Dispatch& d) { d.no_resblock_fusion = (bm == 6); });        // bm = 6: narrow-stage ResBlocks as separate launches (A/B of resblock.hip)
  if (bm == 3 || bm == 0) dispatch_edit([bm](Dispatch& d) { d.no_pair_fusion = (bm == 3); });            // bm = 3: narrow-stage resblock pairs as two launches (A/B of the fused kernel)
  debug_force_tile((bm == 3 || bm == 6) ? 0 : bm, bn, ks);
  return SS_OK;
}
extern "C" int ss_debug_sk_errors(void) { return conv_sk_error_count() + conv_sk2_error_count() + g_mt_timeouts.load(std::memory_order_relaxed); }

