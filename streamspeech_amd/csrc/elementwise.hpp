// Row-wise / pointwise kernels of the S2ST path (LayerNorm, chunk-causal depthwise conv + BN + SiLU,
// embeddings, masked argmax, CTC collapse, vocoder glue).
#pragma once
#include "common.hpp"

struct ss_ctc_align_result;          // include/streamspeech_hip.h
struct ss_ctc_beam_hyp;
struct ss_ctc_beam_lm_hyp;
struct ss_ctc_lm_opts;
struct ss_ngram_lm;
struct ss_ctc_bias;
struct ss_ctc_bias_opts;

namespace ss {

// y[m,:] = LayerNorm(x[m,:]) * gamma + beta   (eps 1e-5; torch.nn.LayerNorm semantics:
// biased variance of deviations from the mean).  D multiple of 64, D <= 1024.
int launch_layernorm(const float* x, int ldx, float* y, int ldy, const float* gamma, const float* beta,
                     int M, int D, float eps, hipStream_t stream);

// Conformer ConvolutionModule middle (reference chunk_unity/modules/conformer_layer.py:108-113):
// y[t,c] = SiLU(BN_eval(sum_j w[j,c] * x[t+j-K/2, c]))  with the ChunkCausalConv1d visibility rule
// (positions >= (t/chunk+1)*chunk and outside [0,T) read as zero; chunk = 0 -> plain "same" conv).
// wt is the depthwise weight transposed to [K][C].
int launch_dwconv_bn_silu(const float* x, int ldx, float* y, int ldy, const float* wt, int K,
                          const float* bn_mean, const float* bn_var, const float* bn_gamma,
                          const float* bn_beta, float bn_eps, int T, int C, int chunk, hipStream_t stream,
                          const int* segs = nullptr, int nseg = 0,   // segs {row_start,len}; T = max len
                          int t_begin = 0);   // single utterance: only rows t_begin..T-1 are computed (rows before are context)

// out[i,:] = scale * emb[tok[i],:] + pos_table[pos0 + i, :]     (MT decoder input embedding,
// reference ctc_unity/modules/transformer_decoder.py:297-326)
int launch_embed_tokens(const int* tok, const float* emb, const float* pos_table, float scale, int pos0,
                        float* out, int n, int D, hipStream_t stream, int pos_stride, int pad_id, int vocab);
// pos_stride 0: same position for all rows; pad_id: token that takes position pad_id (-1: none); ids outside [0, vocab) read row 0
// Per-row positions: row i takes position pos0 + row_pos[i] (device array; the ragged lock-step search of ss_batch_mt_continue),
// clamped to the pos_rows rows of the table (a row whose search is over keeps being fed and must not read past it)
int launch_embed_tokens_rows(const int* tok, const float* emb, const float* pos_table, int pos_rows, float scale, int pos0,
                             const int* row_pos, float* out, int n, int D, hipStream_t stream, int pad_id, int vocab);

// out[u,:] = src[u/up,:] + (src[u/up,0] != pad_value ? pos_row : 0)   (CTC unit decoder input,
// reference ctc_unity/modules/ctc_transformer_unit_decoder.py:153-181)
int launch_upsample_add_pos(const float* src, int n, int up, const float* pos_row, float pad_value,
                            float* out, int D, hipStream_t stream);

// out[u,:] = src[u/up,:] for u < n * up: every row of src [n, D] written `up` times in a row (the unit decoder's first-layer QKV rows,
// computed once per distinct input row: batch.hip).  D % 4 == 0, both buffers 16-byte aligned, n * up < 2^31; else SS_ERR_ARG.
int launch_upsample_rows(const float* src, int n, int up, float* out, int D, hipStream_t stream);

// ids[m] = argmax_n logits[m,n] over n not in {mask0,mask1,mask2} (first max wins);
// if force >= 0 the result is `force` (beam-search max-length rule).  Optionally max value out.
int launch_masked_argmax(const float* logits, int ld, int M, int N, int mask0, int mask1, int mask2,
                         int force, int* ids, hipStream_t stream, const int* row_max_len = nullptr, int step = 0,
                         int force_id = -1,   // row_max_len: force `force_id` on rows with step >= row_max_len[row]
                         const int* row_min_len = nullptr, int ban_id = -1);   // row_min_len: mask1 = ban_id on rows with step < row_min_len[row]

// out[m] = max_{n not in masks} log_softmax(logits[m,:])[n]   (researches/ctc_unity/ctc_generator.py:55-63)
int launch_log_softmax(const float* logits, int ld, int M, int N, int mask0, int mask1, int as_probs, float* out, int ldo,
                       hipStream_t stream);
int launch_row_max_logprob(const float* logits, int ld, int M, int N, int mask0, int mask1, int mask2, float* out,
                           hipStream_t stream);

// CTC collapse (reference agent/ctc_decoder.py:66-88): drop repeats, then drop `blank` and `pad`.
// tokens/index get the survivors and their frame index; *count their number.  Single workgroup.
int launch_ctc_collapse(const int* raw, int T, int blank, int pad, int* tokens, int* index, int* count,
                        hipStream_t stream, const int* segs = nullptr, int nseg = 0);  // segs {start,len}: count[s]

// Scored twins of the two launchers above for the text CTC heads (ctc_scores.hip; reference agent/ctc_decoder.py:52-62,
// `positional_scores`): ids as launch_masked_argmax without force / row lengths, lprob[m] as launch_row_max_logprob from the same
// read of the row; tokens / index / count as launch_ctc_collapse, plus per kept token the last frame of its run of equal raw ids
// and the float32 sum of lprob over that run, added in ascending frame order.
int launch_masked_argmax_lprob(const float* logits, int ld, int M, int N, int mask0, int mask1, int mask2, int* ids, float* lprob,
                               hipStream_t stream);
int launch_ctc_collapse_spans(const int* raw, const float* lprob, int T, int blank, int pad, int* tokens, int* index, int* last,
                              float* tok_lprob, int* count, hipStream_t stream, const int* segs = nullptr, int nseg = 0);

// Score of a GIVEN token per logits row (mt_score.hip; fairseq's SequenceScorer on the first-pass text decoder): for row r with
// target[r] = tk in [0, N): stat[2r] = log_softmax(row)[tk], stat[2r + 1] = the arg-max log-probability, idx[2r] = the arg-max id
// (lowest index of a tie), idx[2r + 1] = tk's rank (columns above it, plus equal columns below index tk).  log_softmax_kernel's
// arithmetic, so both values are the bits launch_log_softmax writes at those columns.  tk outside [0, N): the row writes nothing.
// A row whose values go NaN (a NaN or +inf column, or all -inf): NaN, NaN, -1, -1.  form: 0 = by width, 1 = force the two-read
// strided form (tests).  M <= MT_SCORE_MAX_ROWS (the grid's x extent times 256 threads stays below 2^32).
constexpr int MT_SCORE_MAX_ROWS = 16777215;
constexpr int MT_SCORE_MAX_REG_N = 8192;          // widest row the register form holds (PER = 32)
int launch_mt_token_scores(const float* logits, int ld, int M, int N, const int* target, float* stat, int* idx, hipStream_t stream,
                           int form = 0);

// CTC forced alignment of given labels (ctc_align.hip; the plan, its checks and its limits: ctc_align.hpp).  Two launches over a
// checked plan: per packed frame row the plain log-softmax at the utterance's states (lp, float32, the denominator of ctc_row.hpp),
// then one workgroup per utterance for the forward sum, the max-plus pass with 2-bit back-pointers, the
// back-trace and each label's first / last frame and float32 sum of lp over its run in ascending frame order.  d_table
// (ctc_align_table_bytes) and d_work (plan.work_bytes()) are the caller's scratch; path and frame_lprob (the path's lp per frame) may
// be null.  An utterance's outputs are the same bits alone and at any place of any pack.
struct CtcAlignPlan;
size_t ctc_align_table_bytes(const CtcAlignPlan& p);
int launch_ctc_align(const float* logits, int ld, int V, const CtcAlignPlan& p, const int32_t* h_targets, void* d_table, void* d_work,
                     ss_ctc_align_result* results, int* path, int* first, int* last, float* tok_lprob, float* frame_lprob,
                     hipStream_t stream);

// CTC prefix beam search (ctc_beam.hip; the plan, its checks, its limits and the search's definition: ctc_beam.hpp).  A fill of the
// child tables and two launches over a checked plan: per packed frame row the log-softmax denominator (den [rows][2]: max, log-sum,
// ctc_row.hpp) and the ids of the plan's `cand` largest unmasked non-blank logits (cand_id [rows][cand], -1 where there are fewer),
// then one workgroup per utterance for the search and the back-trace of its n-best.  lm == nullptr: the plain form, hyps an
// ss_ctc_beam_hyp array, d_work holds plan.work_bytes(); else the LM form (ctc_beam.hpp, ngram_lm.hpp), hyps an ss_ctc_beam_lm_hyp
// array, d_work holds plan.work_bytes_lm(), and ctc_beam_lm_check is every refusal it adds.  d_table (ctc_beam_table_bytes) and
// d_work are the caller's scratch; den_out / cand_out, when given, receive the first kernel's outputs instead of d_work.  An
// utterance's outputs are the same bits alone and at any place of any pack.  bias != nullptr: a bias form (ctc_bias.hpp), with a
// model or without (lm and opts both NULL), hyps an ss_ctc_beam_bias_hyp array, d_work holds plan.work_bytes_form(form), and
// ctc_beam_bias_check is every refusal it adds to the model's.
struct CtcBeamPlan;
size_t ctc_beam_table_bytes(const CtcBeamPlan& p);
int ctc_beam_lm_check(const ss_ngram_lm* lm, int V, const ss_ctc_lm_opts* opts);
int ctc_beam_bias_check(const ss_ctc_bias* bias, int V, int pad, int unk, const ss_ctc_bias_opts* bopts, const ss_ngram_lm* lm,
                        const ss_ctc_lm_opts* opts);
int launch_ctc_beam(const float* logits, int ld, int V, int pad, int unk, const CtcBeamPlan& p, void* d_table, void* d_work,
                    const ss_ngram_lm* lm, const ss_ctc_lm_opts* opts, void* hyps, int* tokens, int out_stride, float* den_out,
                    int* cand_out, hipStream_t stream, const ss_ctc_bias* bias = nullptr, const ss_ctc_bias_opts* bopts = nullptr);
// The score kernel of ngram_lm.hip: d_table (ngram_score_table_bytes) is the caller's scratch.
size_t ngram_score_table_bytes(int B);
int launch_ngram_score(const ss_ngram_lm* lm, int B, const int32_t* d_tokens, const int32_t* h_n, int with_eos, double* d_lp,
                       int32_t* d_state, void* d_table, hipStream_t stream);
// The score kernel of ctc_bias.hip, likewise.
size_t bias_score_table_bytes(int B);
int launch_bias_score(const ss_ctc_bias* bias, int B, const int32_t* d_tokens, const int32_t* h_n, int finish, double* d_delta,
                      int32_t* d_state, double* d_sum, void* d_table, hipStream_t stream);

// emb_out[k,:] = table[codes[k],:]
int launch_gather_rows(const int* idx, const float* table, int D, float* out, int n, hipStream_t stream, int rows);  // ids outside [0, rows) read row 0
// dst[dst_row[k] * ldd + c] = src[k * lds + c] for c < D; rows outside [0, dst_rows) are skipped
int launch_scatter_rows(const int* dst_row, const float* src, int lds, float* dst, int ldd, int D, int n, int dst_rows,
                        hipStream_t stream);

// dur[k] = clamp(round_half_even(exp(logdur[k]) - 1), min 1)   (reference agent/tts/codehifigan.py:61-64);
// forced != null overrides the prediction.  cum[0..K] = exclusive prefix sum (cum[K] = total frames).
// Single workgroup.
int launch_dur_predict(const float* logdur, const int* forced, int K, int* dur, int* cum, hipStream_t stream,
                       const int* segs = nullptr, int nseg = 0);  // segs {start,len}; cum of s at start+s

// out[f,:] = emb[k(f),:], k(f) = the unit whose [cum[k], cum[k+1]) holds f  (torch.repeat_interleave)
int launch_repeat_rows(const float* emb, const int* cum, int K, int D, float* out, int F, hipStream_t stream,
                       const int* segs = nullptr, int nseg = 0);  // segs {unit_start,n_units,frame_start,n_frames}; F = max

// wav[t] = tanh(b + sum_{j<7,c<C} w[j*C+c] * lrelu(x[t+j-3, c], slope))   (HiFi-GAN conv_post,
// reference fairseq/models/text_to_speech/hifigan.py:166-168; slope = 0.01)
int launch_conv_post_tanh(const float* x, int T, int C, const float* w, const float* bias, float slope,
                          float* wav, hipStream_t stream, const int* segs = nullptr, int nseg = 0);  // {start,len}; T = max
// The same conv_post + tanh computing only a tail of each segment: segs[4 s] = {sample_start, n_samples, first, out_start}; samples
// first .. n_samples - 1 of segment s (the same arithmetic as above, whose segment it is) go to wav[out_start ..].  max_keep = the
// longest kept tail (grid sizing).
int launch_conv_post_tanh_crop(const float* x, int C, const float* w, const float* bias, float slope, float* wav, const int* segs,
                               int nseg, int max_keep, hipStream_t stream);

// Speaker term of a multi-speaker conv_pre, added to its code-half output: for row t of a segment of L rows
// y[row, c] = act(x[row, c] + table[speaker][4 * lo + (hi - 3)][c]), lo = max(0, 3 - t), hi = min(6, L + 2 - t) (the taps of the 7-tap
// "same" conv that fall inside the segment); table [num_speakers][16][C0] (weights.py speaker_table).  act != 0: leaky-ReLU(slope).
// y may be x.  segs: conv segs {out_start, out_len, ., .} [nseg], spkr [nseg] the segments' speakers (device), max_seg_out the longest
// segment; nseg = 0: one segment of M rows with speaker spkr0.  Rows outside every segment are not touched.  C0 and ld multiples of 4.
int launch_spkr_pre_add(const float* x, float* y, int ld, int C0, const float* table, const int* spkr, int spkr0, const int* segs,
                        int nseg, int max_seg_out, int M, int act, float slope, hipStream_t stream);

}  // namespace ss
