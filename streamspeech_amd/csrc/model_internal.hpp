// Internals shared by the stage / batch / vocoder / debug translation units of the C ABI (include/streamspeech_hip.h): the context
// structs (ss_model, ss_vocoder: weights by slot name, scratch, caches, per-context settings) and the small host helpers every stage
// uses.  Round 5 split the 1 900-line model.hip into
//   model.hip     context creation / weights, front-end, single-utterance stages (encoder, streaming encoder, CTC, MT, T2U)
//   batch.hip     the ragged-batch twins of those stages (ss_batch_*)
//   vocoder.hip   the unit HiFi-GAN: context, generator stack, single-utterance and ragged-batch forward
//   debug_ops.hip op-level unit-test entry points (ss_op_*), test hooks (ss_debug_*), the profiler's C ABI (ss_prof_*)
#pragma once
#include <algorithm>
#include <atomic>
#include <map>
#include <mutex>
#include <string>
#include <tuple>
#include <unordered_map>
#include <vector>

#include "../../include/streamspeech_hip.h"
#include "attention.hpp"
#include "attn_probs.hpp"
#include "common.hpp"
#include "elementwise.hpp"
#include "fbank.hpp"
#include "gemm.hpp"
#include "mt_step.hpp"
#include "enc_step.hpp"

using namespace ss;

namespace {

struct Slot { const float* p = nullptr; int64_t n = 0; };

struct WeightTable {
  std::unordered_map<std::string, Slot> map;
  std::string missing;
  int build(const float* blob, size_t blob_floats, const char* const* names, const int64_t* offs,
            const int64_t* numels, int n) {
    for (int i = 0; i < n; ++i) {
      if (offs[i] < 0 || (size_t)(offs[i] + numels[i]) > blob_floats) return SS_ERR_ARG;
      map[names[i]] = Slot{blob + offs[i], numels[i]};
    }
    return SS_OK;
  }
  const float* get(const std::string& name, int64_t expect) {
    auto it = map.find(name);
    if (it == map.end() || (expect > 0 && it->second.n != expect)) {
      if (missing.empty()) {
        missing = name;
        fprintf(stderr, "[streamspeech_hip] weight slot '%s' missing or wrong size (want %lld, have %lld)\n",
                name.c_str(), (long long)expect, it == map.end() ? -1LL : (long long)it->second.n);
      }
      return nullptr;
    }
    return it->second.p;
  }
};

// Bytes held by the buffers of one scratch set (ss_scratch): `cap` > 0 bounds them (ss_scratch_set_cap)
struct ScratchAcct { size_t cap = 0, used = 0; };

// Not copyable: a copy would share `p` and overwrite the destination's `acct`, taking the buffer off its set's books.  Ownership
// moves with swap(), which exchanges the memory and re-books it -- each side keeps its own `acct`.
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  ScratchAcct* acct = nullptr;       // the scratch set this buffer is booked under (null: a weight-side buffer, not capped)
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  void swap(DevBuf& o) {
    if (acct) acct->used = acct->used - bytes + o.bytes;
    if (o.acct) o.acct->used = o.acct->used - o.bytes + bytes;
    std::swap(p, o.p);
    std::swap(bytes, o.bytes);
  }
  int ensure(size_t need, bool exact = false) {      // exact: no growth slack (fixed pieces whose size is known up front)
    if (need <= bytes) return SS_OK;
    size_t cap = exact ? need : need + std::min(need / 4, (size_t)256 << 20) + 4096;   // growth slack: a quarter, at most 256 MB (a pack's activations run to 12 GB)
    if (acct && acct->cap) {
      const size_t others = acct->used - bytes;
      if (others + cap > acct->cap) cap = need;                          // no slack under a cap ...
      if (others + cap > acct->cap) return SS_ERR_SCRATCH_CAP;           // ... and a clean error past it (nothing was freed)
    }
    if (p) { SS_HIP_CHECK(hipDeviceSynchronize()); SS_HIP_CHECK(hipFree(p)); p = nullptr; if (acct) acct->used -= bytes; bytes = 0; }
    SS_HIP_CHECK(hipMalloc(&p, cap));
    bytes = cap;
    if (acct) acct->used += cap;
    return SS_OK;
  }
  void release() { if (p) { (void)hipFree(p); p = nullptr; if (acct) acct->used -= bytes; bytes = 0; } }
  float* f() const { return reinterpret_cast<float*>(p); }
};

struct Lin { const float* w = nullptr; const float* b = nullptr; };
struct LN { const float* g = nullptr; const float* b = nullptr; };

static int mt_persistent_env() {
  const char* e = getenv("SS_MT_PERSISTENT");
  const int v = e ? atoi(e) : 0;
  return (v == 64 || v == 128 || v == 256) ? v : 0;       // anything else: the launch-per-op form
}
static const int g_mt_persistent_default = mt_persistent_env();   // default of ss_mt_set_persistent for new contexts (0: launch-per-op decode step)
static const int g_no_mt_device_loop = getenv("SS_NO_MT_DEVICE_LOOP") ? atoi(getenv("SS_NO_MT_DEVICE_LOOP")) : 0;   // A/B knob: one persistent launch per TOKEN (round 3) instead of one per search
static const int g_no_enc_step = getenv("SS_NO_ENC_STEP") ? atoi(getenv("SS_NO_ENC_STEP")) : 0;   // A/B knob: the streaming encoder's layers as one launch per op even on a persistent context
static const int g_no_mt_ln_fusion = getenv("SS_NO_MT_LN_FUSION") ? atoi(getenv("SS_NO_MT_LN_FUSION")) : 0;   // A/B knob: separate final LayerNorm launch in the MT decode step

[[maybe_unused]] int linear(hipStream_t s, const float* A, int lda, int M, const Lin& l, int N, int K, float* C, int ldc,
           int act = ACT_NONE, float alpha = 1.f, const float* R = nullptr, int ldr = 0, int glu = 0) {
  GemmArgs a;
  a.A = A; a.lda = lda; a.W = l.w; a.bias = l.b; a.C = C; a.ldc = ldc; a.R = R; a.ldr = ldr;
  a.M = M; a.N = N; a.Cin = K; a.in_len = M; a.act = act; a.alpha = alpha; a.glu = glu;
  a.same_rows = 1;   // a linear layer maps row m to row m
  return launch_conv_gemm(a, s);
}

[[maybe_unused]] int layernorm(hipStream_t s, const float* x, float* y, const LN& ln, int M, int D) {
  return launch_layernorm(x, D, y, D, ln.g, ln.b, M, D, 1e-5f, s);
}

// C = epilogue(LayerNorm(x) @ W^T): fused into the GEMM prologue on the small-M path, otherwise a
// LayerNorm launch into `h` followed by the GEMM.
[[maybe_unused]] int ln_linear(hipStream_t s, const float* x, int M, const LN& ln, const Lin& l, int N, int K, float* C, int ldc,
              float* h, int act = ACT_NONE, float alpha = 1.f, int glu = 0) {
  GemmArgs a;
  a.A = x; a.lda = K; a.W = l.w; a.bias = l.b; a.C = C; a.ldc = ldc;
  a.M = M; a.N = N; a.Cin = K; a.in_len = M; a.act = act; a.alpha = alpha; a.glu = glu;
  a.same_rows = 1;
  const int canon = debug_tile_forced() ? CANON_NONE : canon_mode();
  if (canon == CANON_SMALLM) {                // lock-step MT decode rows: LayerNorm in the small-M kernel's prologue, always
    a.ln_g = ln.g; a.ln_b = ln.b;
    return launch_conv_gemm(a, s);
  }
  if (canon == CANON_SEQ) {
    // pack-invariant: the LayerNorm form must not change with the row count -- K = 256 layers always take the row-tile kernel's
    // (rtlin.hip), the others always the LayerNorm kernel + a GEMM
    GemmArgs b = a;
    b.ln_g = ln.g; b.ln_b = ln.b;
    if (rtlin_shape_ok(b)) return launch_conv_gemm(b, s);
    int rc = layernorm(s, x, h, ln, M, K);
    if (rc != SS_OK) return rc;
    a.A = h;
    return launch_conv_gemm(a, s);
  }
  if (smallm_eligible(a) && K <= 512) {
    a.ln_g = ln.g; a.ln_b = ln.b;
    return launch_conv_gemm(a, s);
  }
  if (!debug_tile_forced()) {                 // (a forced tile keeps launch_conv_gemm off the row-tile kernel: ADVICE r4)
    GemmArgs b = a;
    b.ln_g = ln.g; b.ln_b = ln.b;
    if (rtlin_eligible(b)) return launch_conv_gemm(b, s);      // LayerNorm in the row tile's way into LDS (rtlin.hip)
  }
  int rc = layernorm(s, x, h, ln, M, K);
  if (rc != SS_OK) return rc;
  a.A = h;
  return launch_conv_gemm(a, s);
}

}  // namespace

static const int g_pack_invariant_default = getenv("SS_PACK_INVARIANT") ? atoi(getenv("SS_PACK_INVARIANT")) : 1;   // A/B knob: default of ss_model_set_pack_invariant for new contexts

// =================================================================================================
// model
// =================================================================================================
struct EncLayer {
  LN ffn1_ln, attn_ln, conv_ln, ffn2_ln, final_ln;
  Lin ffn1_w1, ffn1_w2, ffn2_w1, ffn2_w2, qkv, out, pw1, pw2;
  const float *u, *v, *dw_wt, *bn_mean, *bn_var, *bn_g, *bn_b;
};
struct DecLayer {
  LN self_ln, cross_ln, ffn_ln;
  Lin self_qkv, self_out, cross_q, cross_kv, cross_out, fc1, fc2;
  bool has_cross = false;
};

// Everything a call MUTATES: activations, KV caches, the stream-K hand-off state, streaming-encoder state, the token chain.
// One per concurrent stream (ss_scratch_create); any number of weight handles (ss_model / ss_vocoder: one per language, cheap) may be
// bound to it one after the other (ss_model_bind_scratch / ss_vocoder_bind_scratch) -- round 5 welded a scratch set into every weight
// handle, so L languages on S streams cost L x S scratch sets.  Ref-counted: freed when the creator and
// every bound handle have let go.
struct ss_scratch {
  std::atomic<int> refs{1};
  ScratchAcct acct;
  SkWorkspace* skws = nullptr;       // stream-K hand-off state of this context
  // ---- model side ----
  DevBuf ws;            // encoder / t2u / unit scratch
  DevBuf mt_cross;      // [mt_layers][Tp][2*D]
  DevBuf mt_self;       // [mt_layers][max_tgt_pos][3*D]
  DevBuf mt_ws;         // per-append scratch
  int mt_Tp = 0;
  int mt_len = 0;
  const float* mt_enc = nullptr;
  DevBuf attn_split;             // key-split scratch of the single-utterance rel-pos attention (attention.hpp); counters zeroed once
  DevBuf mt_gran;                // persistent decode step (mt_step.hip): granule region, zeroed once; the epoch grows per launch
  unsigned mt_epoch = 0;
  hipStream_t mt_last_stream = nullptr;   // stream of the last persistent-step launch (mt_collect_errors reads / clears the error word there)
  int mt_inject_timeout = 0;     // ss_debug_mt_inject_timeout: the next persistent launch reports a time-out
  int mt_persistent = g_mt_persistent_default;   // workgroups of the persistent decode step (ss_mt_set_persistent); 0 = launch-per-op
  DevBuf mt_tok;                 // device token chain [max_tgt_pos] (greedy search feeds itself)
  DevBuf seg_buf;                // ragged-batch segment tables / batched token chain
  DevBuf bmt_self;               // batched MT self-attention cache [layer][B][Lcap][3D] (beam search: [layer][B*k][Lcap][3D])
  DevBuf bmb_feat;               // beam search: post-LN decoder states of every slot and step [B*k][Lcap][D]
  DevBuf bmb_state;              // beam search: token / score / ancestry tables, candidates, finalised hypotheses (beam.hip)
  int32_t* mt_tok_host = nullptr;  // pinned staging of the same
  size_t mt_tok_host_n = 0;
  // incremental streaming encoder (ss_encoder_stream_*): per-layer fused q|k|v rows and GLU outputs
  // of every frame so far + the finished output rows; rows < es_final are final
  DevBuf es_qkv;        // [layers][es_cap][3d]
  DevBuf es_glu;        // [layers][es_cap][d]
  DevBuf es_out;        // [es_cap][d]
  DevBuf es_step;       // persistent layer launches (enc_step.hip): partial FFN outputs, depthwise output, arrival counter + error word (zeroed once)
  unsigned es_bar = 0;  // value of the arrival counter when the next launch starts
  int es_step_off = 0;  // 1 after a time-out: this scratch set stays on one launch per op
  int es_deferred = 0;  // ss_encoder_stream_set_deferred: the persistent form's time-out check is left to ss_encoder_stream_status
  int es_pending = 0;   // a deferred check is outstanding (the last forward's output must not be trusted yet)
  int es_final_prev = 0;   // es_final before that forward (restored when the check fails)
  int es_inject = 0;    // test hook: the next check reports a time-out
  unsigned* es_err_host = nullptr;   // pinned host word the persistent layer launches bump on a time-out (next to the device word the workgroups poll):
                                     // the host reads it after its stream synchronisation -- no device-to-host copy per call
  int es_cap = 0, es_final = 0, es_achunk = -1, es_cchunk = -1;
  int es_tail = 0;                                  // trailing fbank frames that may still change (resampler edge)
  // ss_debug_last_logits: where the last batched argmax stage of this context left its dense logits (scratch, valid until the
  // next call that uses the same scratch buffer)
  const float* dbg_logits = nullptr;
  int dbg_rows = 0, dbg_cols = 0;
  // ---- vocoder side ----
  DevBuf v_ws, v_small, v_segs;
  ss_scratch() {
    for (DevBuf* b : all()) b->acct = &acct;
    skws = sk_workspace_new();
  }
  ~ss_scratch() {
    for (DevBuf* b : all()) b->release();
    if (mt_tok_host) (void)hipHostFree(mt_tok_host);
    if (es_err_host) (void)hipHostFree(es_err_host);
    sk_workspace_free(skws);
  }
  // fixed pieces that live outside the set but are booked in it: the slot state of streaming session pools made against this set
  // (ss_stream_pool_create; they register here and leave with the pool).  Never trimmed.
  std::vector<DevBuf*> extra;
  std::vector<DevBuf*> all() {
    std::vector<DevBuf*> v = {&ws, &mt_cross, &mt_self, &mt_ws, &attn_split, &mt_gran, &mt_tok, &seg_buf, &bmt_self, &bmb_feat, &bmb_state, &es_qkv, &es_glu, &es_out, &es_step, &v_ws, &v_small, &v_segs};
    v.insert(v.end(), extra.begin(), extra.end());
    return v;
  }
  // what ss_scratch_trim may let go: buffers every entry point re-sizes before use (the zero-initialised ones and the KV cache stay)
  std::vector<DevBuf*> trimmable() { return {&ws, &mt_cross, &mt_ws, &seg_buf, &bmt_self, &bmb_feat, &bmb_state, &es_qkv, &es_glu, &es_out, &v_ws, &v_small, &v_segs}; }
};
[[maybe_unused]] static void scratch_unref(ss_scratch* sc) { if (sc && sc->refs.fetch_sub(1) == 1) delete sc; }
// the fixed-size pieces a model of configuration `c` needs in the scratch set it runs on: the MT self-attention cache, the token chain
[[maybe_unused]] static int scratch_fit_model(ss_scratch* sc, const ss_config& c) {
  int rc = sc->mt_self.ensure((size_t)c.mt_layers * c.max_tgt_pos * 3 * c.dec_dim * sizeof(float));
  if (rc == SS_OK) rc = sc->mt_tok.ensure((size_t)c.max_tgt_pos * sizeof(int32_t));
  if (rc == SS_OK && sc->mt_tok_host_n < (size_t)c.max_tgt_pos) {
    if (sc->mt_tok_host) (void)hipHostFree(sc->mt_tok_host);
    sc->mt_tok_host = nullptr; sc->mt_tok_host_n = 0;
    if (hipHostMalloc((void**)&sc->mt_tok_host, (size_t)c.max_tgt_pos * sizeof(int32_t)) != hipSuccess) return SS_ERR_HIP;
    sc->mt_tok_host_n = (size_t)c.max_tgt_pos;
  }
  return rc;
}

struct ss_model {
  ss_config cfg;
  WeightTable wt;
  ss_scratch* sc = nullptr;          // the scratch set this handle is bound to (its own unless ss_model_bind_scratch said otherwise)
  // encoder
  Lin sub0, sub1, enc_linear, ctc_asr, ctc_st;
  std::vector<EncLayer> enc;
  const float* pos_table = nullptr;  // [2*Tmax-1, d]
  const float* pos_w = nullptr;      // [L*d, d]
  const float* pos_proj = nullptr;   // [2*Tmax-1, L*d]: a function of the blob -- ONE buffer per blob and device, shared by every handle over it (model.hip)
  int pos_key_dev = 0;
  // front-end
  const float *fe_window = nullptr, *fe_melw = nullptr, *fe_mean = nullptr, *fe_std = nullptr;
  DevBuf fe_tab;                     // FbankTables of this model, made once at creation: mel ranges int [80][2], then twiddles float [512]
  FbankTables fe_tables;             // pointers into fe_tab
  // decoders
  const float* mt_emb = nullptr; const float* mt_pos = nullptr; LN mt_ln;
  std::vector<DecLayer> mt, t2u, unit;
  LN t2u_ln, unit_ln;
  Lin unit_out;
  const float* unit_pos_row = nullptr;
  // ss_model_set_pack_invariant: 1 = every ss_batch_* stage upstream of an arg-max computes a packed utterance with arithmetic that
  // is a function of that utterance alone (same bits alone, in any pack, at any position); 0 = fastest kernel per shape (round-4 routes)
  int pack_invariant = g_pack_invariant_default;
};

// The tables every fbank launch of this model passes on: the model's own, or none (the dense mel walk and the in-kernel twiddles:
// SS_FBANK_DENSE / ss_debug_fbank_dense -- the same bits, kept for A/B and for the test that says so).
[[maybe_unused]] static FbankTables fe_tables(const ss_model* m) { return disp().fbank_dense ? FbankTables{} : m->fe_tables; }

// Key-split scratch of this context for the single-utterance rel-pos attention: allocated and zeroed on first use (the
// counters must read zero; the stream is synchronised once so that a later call on another stream sees them).
[[maybe_unused]] static int bind_attn_split(ss_model* m, AttnArgs& at, hipStream_t s) {
  if (!m->sc->attn_split.p) {
    RET(m->sc->attn_split.ensure(attention_split_bytes()));
    SS_HIP_CHECK(hipMemsetAsync(m->sc->attn_split.p, 0, attention_split_bytes(), s));
    SS_HIP_CHECK(hipStreamSynchronize(s));
  }
  attention_bind_split(at, m->sc->attn_split.p);
  return SS_OK;
}

[[maybe_unused]] static int conv_out_len(int L, int k, int stride) { return (L + 2 * (k / 2) - k) / stride + 1; }

// The encoder's chunk arguments: a conv chunk outside (0, 999) is none (chunk_causal_conv1d.py:40), an attention chunk outside
// (0, 999999) is full attention; attn_chunk_in: the attention chunk as it acts on T2 rows (a chunk of T2 or more rows is none)
[[maybe_unused]] static int conv_chunk_cfg(int chunk) { return (chunk > 0 && chunk < 999) ? chunk : 0; }
[[maybe_unused]] static int attn_chunk_cfg(int chunk) { return (chunk > 0 && chunk < 999999) ? chunk : 0; }
[[maybe_unused]] static int attn_chunk_in(int chunk, int T2) { return (chunk > 0 && chunk < T2) ? chunk : 0; }

// ---- incremental streaming encoder (ss_encoder_stream_forward, the session pool of stream_pool.hip) ----------------------------
// Finality: a frame i of the 40-ms grid reaches, in one layer, keys up to the end of its attention
// chunk and conv taps up to min(i+15, end of its conv chunk); through the subsampler it reaches
// conv1 rows a(i) = min(2i+2, chunk end) and fbank rows b(a(i)).  The final prefix [0, n) is the
// largest one that is closed under "reaches" and whose subsampler inputs all exist.
[[maybe_unused]] static int stream_final_rows(int T, int T1, int T2, int k, int achunk, int cchunk, int dwk, int tail) {
  if (achunk <= 0) return 0;                       // full attention: every frame sees the future
  auto reach = [&](int i, int half, int stride) {  // last input row a stride-`stride` conv output i can read
    int r = i * stride + half;
    if (cchunk > 0) r = std::min(r, ((i * stride) / cchunk + 1) * cchunk - 1);
    return r;
  };
  int n = 0;
  for (int i = 0; i < T2; ++i) {                   // subsampler level: frames whose whole cone exists
    const int a = reach(i, k / 2, 2);
    if (a > T1 - 1) break;
    if (reach(a, k / 2, 2) > T - 1 - tail) break;   // the last `tail` fbank frames are not settled yet
    n = i + 1;
  }
  while (n > 0) {                                  // closure under one layer's reach (monotone in i)
    const int i = n - 1;
    const int e_att = (i / achunk + 1) * achunk - 1;
    const int e_conv = reach(i, dwk / 2, 1);
    if (std::max(e_att, e_conv) <= n - 1) break;
    --n;
  }
  return n;
}

// The rows of one streaming call (ss_encoder_stream_forward, pool_plan): rows below `fin` are final from the previous call, made with
// the chunks prev_achunk / prev_cchunk (configured values); a chunk change or a shorter input starts the stream over.  Rows [r0, T2)
// are computed (n of them), rows below nf are final afterwards, and conv 1 of the subsampler starts at row mb1, the first one conv 2
// reads for its row r0.  false: T2 outside [1, max_rows] (nothing else is set).
struct StreamRows { int T1, T2, cchunk, achunk_cfg, achunk, r0, n, nf, mb1; };
[[maybe_unused]] static bool stream_rows(const ss_config& c, int T, int attn_chunk, int conv_chunk, int fin, int prev_achunk,
                                         int prev_cchunk, int tail, int max_rows, StreamRows& r) {
  const int k = c.conv_kernel;
  r.T1 = conv_out_len(T, k, 2); r.T2 = conv_out_len(r.T1, k, 2);
  if (r.T2 <= 0 || r.T2 > max_rows) return false;
  r.cchunk = conv_chunk_cfg(conv_chunk);
  r.achunk_cfg = attn_chunk_cfg(attn_chunk);
  r.achunk = attn_chunk_in(r.achunk_cfg, r.T2);
  if (prev_achunk != r.achunk_cfg || prev_cchunk != r.cchunk) fin = 0;   // chunk change: a new stream
  if (fin > r.T2) fin = 0;                                               // shorter input: a new utterance without reset
  r.r0 = fin; r.n = r.T2 - fin;
  r.nf = std::max(r.r0, stream_final_rows(T, r.T1, r.T2, k, r.achunk_cfg, r.cchunk, c.dw_kernel, tail));
  r.mb1 = std::min(std::max(0, 2 * r.r0 - k / 2), r.T1 - 1);
  return true;
}

// ---- transformer layers shared by MT decoder / T2U encoder / unit decoder ----------------------
// x [n, D] in place.  self K/V cache rows live in `selfbuf` ([*, 3D], row = absolute position).
// One pre-LN transformer layer on the residual stream x [n, D].  The fused QKV rows are written to
// `qkv_rows` with row stride ld_qkv (straight into a KV cache when decoding); the caller prepares
// the attention descriptors (single utterance or ragged batch) -- their O is `h`, cross Q is `q2`.
// The layer in two steps, for a caller that has a cheaper way to the same fused QKV rows (batch_t2u: the unit decoder's first layer):
// dec_layer_qkv writes them for the n rows of x, dec_layer_rest is everything after them.  dec_layer_ex is the two in a row.
[[maybe_unused]] static int dec_layer_qkv(hipStream_t s, const ss_config& c, const DecLayer& L, const float* x, int n, float* qkv_rows,
                         int ld_qkv, float* h) {
  const int D = c.dec_dim;
  return ln_linear(s, x, n, L.self_ln, L.self_qkv, 3 * D, D, qkv_rows, ld_qkv, h);   // q (pre-scaled at pack time), k, v
}
[[maybe_unused]] static int dec_layer_rest(hipStream_t s, const ss_config& c, const DecLayer& L, float* x, int n, const AttnArgs& self_at,
                          const AttnArgs* cross_at, float* h, float* q2, float* ff) {
  const int D = c.dec_dim, F = c.dec_ffn;
  RET(launch_attention(self_at, s));
  RET(linear(s, h, D, n, L.self_out, D, D, x, D, ACT_NONE, 1.f, x, D));
  if (L.has_cross && cross_at) {
    RET(ln_linear(s, x, n, L.cross_ln, L.cross_q, D, D, q2, D, h));
    RET(launch_attention(*cross_at, s));
    RET(linear(s, h, D, n, L.cross_out, D, D, x, D, ACT_NONE, 1.f, x, D));
  }
  RET(ln_linear(s, x, n, L.ffn_ln, L.fc1, F, D, ff, F, h, ACT_RELU));
  RET(linear(s, ff, F, n, L.fc2, D, F, x, D, ACT_NONE, 1.f, x, D));
  return SS_OK;
}
[[maybe_unused]] static int dec_layer_ex(hipStream_t s, const ss_config& c, const DecLayer& L, float* x, int n, float* qkv_rows,
                        int ld_qkv, const AttnArgs& self_at, const AttnArgs* cross_at, float* h, float* q2, float* ff) {
  RET(dec_layer_qkv(s, c, L, x, n, qkv_rows, ld_qkv, h));
  return dec_layer_rest(s, c, L, x, n, self_at, cross_at, h, q2, ff);
}

// single utterance: self K/V cache rows live in `selfbuf` ([*, 3D], row = absolute position)
[[maybe_unused]] static int dec_layer(hipStream_t s, const ss_config& c, const DecLayer& L, float* x, int n, int pos0,
                     float* selfbuf, bool causal, const float* crossKV, int Tk_cross, float* h, float* q2,
                     float* ff, int self_tail_pad = 0, int cross_tail_pad = 0) {
  const int D = c.dec_dim, H = c.dec_heads;
  float* rows = selfbuf + (size_t)pos0 * 3 * D;
  AttnArgs at;
  at.Q = rows; at.ldq = 3 * D; at.K = selfbuf + D; at.V = selfbuf + 2 * D; at.ldk = at.ldv = 3 * D;
  at.O = h; at.ldo = D; at.Tq = n; at.Tk = pos0 + n; at.H = H; at.scale = 1.f; at.causal = causal ? 1 : 0;
  at.k_mask_tail = self_tail_pad;
  AttnArgs ac;
  if (L.has_cross) {
    ac.Q = q2; ac.ldq = D; ac.K = crossKV; ac.V = crossKV + D; ac.ldk = ac.ldv = 2 * D;
    ac.O = h; ac.ldo = D; ac.Tq = n; ac.Tk = Tk_cross; ac.H = H; ac.scale = 1.f; ac.k_mask_tail = cross_tail_pad;
  }
  return dec_layer_ex(s, c, L, x, n, rows, 3 * D, at, L.has_cross ? &ac : nullptr, h, q2, ff);
}

// ---- the Conformer layer shared by the full, batched, streaming and session-pool encoders -----------------------------------------
// Conv1dSubsampler (convolution.py:81-89): the fields of its two stride-2 chunk-causal conv-GEMMs (-> GLU) every encoder shares;
// conv 1 reads `fbank` into `h1`, conv 2 reads `h1` into `out`.  The caller sets the rows (M, in_len, m_begin, segment tables) and
// the chunk.
[[maybe_unused]] static void subsampler_args(const ss_model* m, const float* fbank, float* h1, float* out, GemmArgs& a, GemmArgs& b) {
  const ss_config& c = m->cfg;
  const int k = c.conv_kernel, C1 = c.conv_channels / 2;
  a.A = fbank; a.lda = c.input_feat; a.W = m->sub0.w; a.bias = m->sub0.b; a.C = h1; a.ldc = C1;
  a.N = c.conv_channels; a.Cin = c.input_feat; a.taps = k; a.stride = 2; a.pad = k / 2; a.glu = 1;
  b.A = h1; b.lda = C1; b.W = m->sub1.w; b.bias = m->sub1.b; b.C = out; b.ldc = c.enc_dim;
  b.N = 2 * c.enc_dim; b.Cin = C1; b.taps = k; b.stride = 2; b.pad = k / 2; b.glu = 1;
}

// Macaron FFN half on n rows of x [n, d] in place: x += 0.5 * W2 SiLU(W1 LN(x)), then x = LN_fin(x) when `fin` is given.  `fused`:
// ONE launch_ffn_fused (its whole-tile form when `canon`); otherwise ln_linear + linear through the hidden rows `ff` [n, f] (+ a
// LayerNorm launch), `h` [n, d] the LayerNorm rows ln_linear may need.
[[maybe_unused]] static int enc_ffn_half(hipStream_t s, const ss_config& c, float* x, int n, const LN& ln, const Lin& w1, const Lin& w2,
                                         const LN* fin, bool fused, bool canon, float* h, float* ff) {
  const int d = c.enc_dim, f = c.enc_ffn;
  if (fused)
    return launch_ffn_fused(x, d, x, d, ln.g, ln.b, w1.w, w1.b, w2.w, w2.b, 0.5f, fin ? fin->g : nullptr, fin ? fin->b : nullptr,
                            n, d, f, s, canon);
  RET(ln_linear(s, x, n, ln, w1, f, d, ff, f, h, ACT_SILU));
  RET(linear(s, ff, f, n, w2, d, f, x, d, ACT_NONE, 0.5f, x, d));
  return fin ? layernorm(s, x, x, *fin, n, d) : SS_OK;
}

// One Conformer layer on n rows of the residual stream x [n, d] in place: FFN1 half -> RelPosMHA -> conv module -> FFN2 half + the
// final LayerNorm.  The QKV projection writes its rows to `qkv_rows` (ld 3d), the GLU point-wise conv to `glu_rows` (ld d), and the
// second point-wise conv reads the depthwise output at `dw_rows` (ld d).  The caller's attention() and dwconv() launch the two steps
// that differ between the encoders (their input and output rows are the caller's); `h` [n, d] is the attention context and the
// LayerNorm scratch, `ff` the FFN hidden rows (two-launch form).
template <typename Attention, typename DwConv>
static int enc_layer_ex(hipStream_t s, const ss_config& c, const EncLayer& e, float* x, int n, float* h, float* ff, float* qkv_rows,
                        float* glu_rows, const float* dw_rows, bool ffn_fused, bool canon, Attention&& attention, DwConv&& dwconv) {
  const int d = c.enc_dim;
  RET(enc_ffn_half(s, c, x, n, e.ffn1_ln, e.ffn1_w1, e.ffn1_w2, nullptr, ffn_fused, canon, h, ff));
  RET(ln_linear(s, x, n, e.attn_ln, e.qkv, 3 * d, d, qkv_rows, 3 * d, h));
  RET(attention());
  RET(linear(s, h, d, n, e.out, d, d, x, d, ACT_NONE, 1.f, x, d));
  RET(ln_linear(s, x, n, e.conv_ln, e.pw1, 2 * d, d, glu_rows, d, h, ACT_NONE, 1.f, 1));
  RET(dwconv());
  RET(linear(s, dw_rows, d, n, e.pw2, d, d, x, d, ACT_NONE, 1.f, x, d));
  return enc_ffn_half(s, c, x, n, e.ffn2_ln, e.ffn2_w1, e.ffn2_w2, &e.final_ln, ffn_fused, canon, h, ff);
}

// The ragged prefix pass of the MT decoder (batch.hip): shared by ss_batch_mt_continue, ss_batch_mt_features and the beam search behind
// a forced prefix (beam.hip).
int mt_prefix_pass(ss_model* m, hipStream_t s, int B, int Np, int np_max, int n_enc, const int* d_ptok, const int* d_ppos,
                   const int* d_pself, const int* d_pcross, const int* d_ptail, const int* d_pcache, int cache_rows, const float** out);

// Cross-attention K/V of every MT layer over n_rows (packed) encoder rows into mt_cross, layer l at + l * n_rows * 2D (model.hip).  The
// caller has booked mt_cross: (mt_layers * n_rows * 2D) floats.
int mt_cross_kv(ss_model* m, hipStream_t s, const float* d_enc_out, int n_rows);

// The head step of everything that reads a text CTC head (model.hip): logits [rows][V] = x [rows][enc_dim, ld ldx] through ctc_asr
// (head 0) or ctc_st (head 1), V that head's vocabulary.  *logits == nullptr: into mt_ws, ensured here and returned; else into the
// caller's buffer.  record: the debug logits fields point at the result (the batch calls; the pools and the stream advance leave
// them alone).  A caller that books other scratch too ensures mt_ws itself, in the order its refusals have always come (the ensure
// here is then a no-op).  SkScope and CanonScope are the caller's.
int ctc_head_logits(ss_model* m, hipStream_t s, int head, const float* x, int ldx, int rows, bool record, float** logits, int* V = nullptr);

// The decode rows' workspace of the lock-step text searches, carved from mt_ws: x | h | q2 | ffn | (gap floats) | logits, one row per
// search row.  floats() is what the five parts take; a search with rows behind the logits books them on top.
struct MtRowsWs {
  float *x, *h, *q2, *ff, *logits;
  static size_t floats(int rows, int D, int F, int V, size_t gap = 0) { return (size_t)rows * (3 * D + F + V) + gap; }
  MtRowsWs(float* base, int rows, int D, int F, size_t gap = 0)
      : x(base), h(x + (size_t)rows * D), q2(h + (size_t)rows * D), ff(q2 + (size_t)rows * D), logits(ff + (size_t)rows * F + gap) {}
};

// One lock-step decode step of a text search (batch.hip): every row feeds one token at cache index `ci`.
struct MtRowsStep {
  int rows = 0;                      // search rows (utterances, or utterances x beam)
  int cache_ld = 0, ci = 0;          // rows of one search row's self-attention cache (bmt_self: [layer][rows][cache_ld][3D]); index fed
  const int* tok = nullptr;          // [rows] the tokens fed
  const int* row_pos = nullptr;      // null: every row at position ci (launch_embed_tokens); else row r at ci + row_pos[r], and
  int row_pad = -1;                  // the pad argument of launch_embed_tokens_rows
  const int* self_segs = nullptr;    // this step's self-attention segments [rows][4]
  const int* cross_segs = nullptr;   // cross-attention segments [rows][4] over the n_enc packed encoder rows of mt_cross
  int n_enc = 0;
  const int* anc = nullptr; int anc_ld = 0, anc_slots = 0;   // the beam's ancestor table (AttnArgs), or none
  float* states = nullptr; int states_ld = 0;                // post-LN states out: row r at + r * states_ld
};
// Embedding -> every MT layer (QKV rows straight into the cache) -> final LayerNorm -> tied vocabulary projection into w.logits.  The
// CanonScope of the decode rows is the caller's.
int mt_decode_rows(ss_model* m, hipStream_t s, const MtRowsWs& w, const MtRowsStep& a);

extern std::atomic<int> g_mt_timeouts;      // bounded-wait time-outs of persistent MT decode steps, process-wide (model.hip)

struct ConvW { const float* w = nullptr; const float* b = nullptr; const float* ww = nullptr;   // ww: Winograd form (64-channel stage ResBlock convs)
               const void* wh = nullptr; };                                                         // wh: FP16 fragment form (conv_f16.hip; ss_vocoder_set_f16)
struct ss_vocoder {
  ss_vocoder_config cfg;
  WeightTable wt;
  ss_scratch* sc = nullptr;          // the scratch set this handle is bound to (ss_vocoder_bind_scratch; its own by default)
  const float* dict = nullptr;
  ConvW dur_c1, dur_c2, dur_proj, pre, post;
  LN dur_ln1, dur_ln2;
  std::vector<ConvW> ups;
  std::vector<ConvW> rb_c1, rb_c2;  // [(stage*n_res + j)*3 + d]
  float* wino = nullptr;             // Winograd F(2,3) forms of the 32- / 64- / 128-channel stages' ResBlock conv weights (conv_c64w.hip):
  const float* wino_key = nullptr;   // ONE buffer per weight blob, shared by every context over that blob (wino_share below)
  int x3 = 0;          // split-bf16 contraction of the C >= 64 generator convs (ss_vocoder_set_bf16x3); default off = exact f32
  int f16 = 0;         // FP16-operand ResBlock convs of the 64- / 128- / 256-channel stages (ss_vocoder_set_f16); wins over x3; default off
  const float* blob = nullptr;       // the weight blob this handle was made over
  void* f16w = nullptr;              // their FP16 weight fragments: ONE buffer per weight blob, shared like `wino` (made on the first switch-on)
  const float* spk_table = nullptr;  // multi-speaker blob ("voc.spkr.table"): the speaker term of conv_pre [n_spk][16][C0] (weights.py speaker_table)
  int n_spk = 0;                     // 0: single-speaker handle
};

namespace {

// small int tables for the kernels: pageable -> device copies are staged by the runtime before
// hipMemcpyAsync returns, so the std::vector may die right after the call
[[maybe_unused]] int upload(hipStream_t s, int* dst, const std::vector<int>& v) {
  SS_HIP_CHECK(hipMemcpyAsync(dst, v.data(), v.size() * sizeof(int), hipMemcpyHostToDevice, s));
  return SS_OK;
}

struct Offsets { std::vector<int> off; int total = 0, mx = 0; };
[[maybe_unused]] Offsets prefix(const int* len, int B) {
  Offsets o; o.off.resize(B + 1); o.off[0] = 0;
  for (int b = 0; b < B; ++b) { o.off[b + 1] = o.off[b] + len[b]; o.mx = std::max(o.mx, len[b]); }
  o.total = o.off[B];
  return o;
}

}  // namespace
