// Streaming session pool (ss_stream_pool_*): the incremental-encoder state of many independent streams in slots of one pool, and
// ONE batched step for all of them.  Per slot the semantics are exactly those of ss_encoder_stream_forward (model.hip): each session
// passes the fbank of all its audio so far, rows final at its previous call come from the slot's cache, only the rest runs through
// the layers.  What is new is where rows of different sessions meet: the tail rows of every session of a call are stacked into ONE
// row pack, and every op runs once per layer for the whole pack --
//   subsampler     both conv-GEMMs as one ragged launch each (per-segment input pointer and first row, GemmArgs::seg_A / seg_mb)
//   linears / FFNs the pack-invariant (CANON_SEQ) routes: a row's bits do not depend on the row count or on its neighbours
//   attention      attention_pool_kernel (attention.hip): tail queries of every session over that session's keys, K/V rows below
//                  the first tail row from the slot cache; it writes the new q|k|v rows to the slot cache on the way
//   depthwise conv pool_dwconv_kernel below: GLU rows below the tail from the slot cache, writes the new GLU rows there on the way
//   output         pool_gather_kernel: the packed output from cached final rows + the new rows, newly final rows into the cache
// Ordinary launches only: no persistent form, no arrival counters, no time-out protocol.  A session's bits are a function of that
// session alone: the same alone, in any pack, at any position in it.
#include "model_internal.hpp"

// ---- kernels -----------------------------------------------------------------------------------------------------------------
namespace {

// last z in [0, n) with pre[z] <= v (pre ascending, pre[0] = 0)
__device__ __forceinline__ int seg_find(const int* pre, int n, int v) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (pre[mid] <= v) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// Chunk-causal depthwise conv + BatchNorm + SiLU of the tail rows of every session (the arithmetic of dwconv_bn_silu_kernel,
// elementwise.hip).  Workgroup (64-channel tile, 32-row tile, session z); sess[8 z] = {q_start, n, r0, T2, slot, -, cchunk, -}.
// Input row t of session z: the slot cache (glu + slot * slot_rows * C) for t < r0, the stacked GLU rows gs for t >= r0.  The
// workgroup also copies its own stacked rows into the slot cache (rows >= r0: nobody in this launch reads them from there).
constexpr int PDW_TT = 32, PDW_TC = 64, PDW_KMAX = 31;
__global__ __launch_bounds__(256) void pool_dwconv_kernel(const float* __restrict__ gs, float* cache, int slot_rows, float* y,
                                                          const float* __restrict__ wt, int K, const float* __restrict__ bn_mean,
                                                          const float* __restrict__ bn_var, const float* __restrict__ bn_gamma,
                                                          const float* __restrict__ bn_beta, float bn_eps, int C, const int* sess) {
  __shared__ float slab[(PDW_TT + PDW_KMAX - 1) * PDW_TC];
  const int* se = sess + 8 * blockIdx.z;
  const int q_start = se[0], n = se[1], r0 = se[2], T = se[3], slot = se[4], chunk = se[6];
  const int t0 = r0 + blockIdx.y * PDW_TT;
  if (t0 >= r0 + n) return;
  const float* xs = gs + (size_t)q_start * C;               // stacked row t - r0 <-> absolute row t
  float* xc = cache + (size_t)slot * slot_rows * C;
  const int c0 = blockIdx.x * PDW_TC;
  const int tid = threadIdx.x, cl = tid & (PDW_TC - 1), rg = tid >> 6;
  const int half = K / 2;
  const int rows = PDW_TT + K - 1;
  {
    constexpr int NL = ((PDW_TT + PDW_KMAX - 1) * PDW_TC + 255) / 256;
    float v[NL];
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int idx = tid + i * 256;
      const int sr = idx / PDW_TC, cc = idx - sr * PDW_TC;
      const int tin = t0 - half + sr;
      const float* src = tin < r0 ? xc + (size_t)tin * C : xs + (size_t)(tin - r0) * C;
      v[i] = (sr < rows && tin >= 0 && tin < T && c0 + cc < C) ? src[c0 + cc] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < NL; ++i) {
      const int idx = tid + i * 256;
      if (idx < (PDW_TT + PDW_KMAX - 1) * PDW_TC) slab[idx] = v[i];
    }
  }
  const int c = c0 + cl;
  float w[PDW_KMAX];
#pragma unroll
  for (int j = 0; j < PDW_KMAX; ++j) w[j] = (j < K && c < C) ? wt[j * C + c] : 0.f;
  __syncthreads();
  if (c >= C) return;
  const float mean = bn_mean[c], rstd = 1.0f / sqrtf(bn_var[c] + bn_eps), gam = bn_gamma[c], bet = bn_beta[c];
  constexpr int NR = PDW_TT / 4, NV = NR + PDW_KMAX - 1;
  float sv[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) sv[i] = slab[(rg * NR + i) * PDW_TC + cl];
#pragma unroll
  for (int u = 0; u < NR; ++u) {
    const int t = t0 + rg * NR + u;
    int lim = T;
    if (chunk > 0) { const int cl_end = (t / chunk + 1) * chunk; if (cl_end < lim) lim = cl_end; }
    const int jmax = min(K, lim - (t - half));
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < PDW_KMAX; ++j) {
      const float a2 = fmaf(w[j], sv[u + j], acc);
      acc = (j < jmax) ? a2 : acc;
    }
    const float v = (acc - mean) * rstd * gam + bet;
    if (t < T) {
      y[(size_t)(q_start + t - r0) * C + c] = v / (1.0f + expf(-v));
      xc[(size_t)t * C + c] = slab[(rg * NR + u + half) * PDW_TC + cl];     // this row's GLU output into the slot cache
    }
  }
}

// Row assembly over the packed layout of a call (sessions in call order, session z at rows pre[z] .. pre[z] + len).  tab[6 z] =
// {-, len, k0, nf, slot, s_start}: row j of session z comes from the slot cache (cache + (slot * slot_rows + j) * W) for j < k0,
// from the stacked rows (stk + (s_start + j - k0) * W) otherwise; rows k0 <= j < nf are also written to the slot cache.
// W = 256 floats (encoder rows, 64 threads per row) or 1 int (CTC arg-max, one thread per row).
template <typename E, int W>
__global__ __launch_bounds__(256) void pool_gather_kernel(E* out, const E* stk, E* cache, int slot_rows, const int* tab,
                                                          const int* pre, int nsess, int total) {
  constexpr int TPR = W >= 4 ? W / 4 : 1;                  // threads per row
  constexpr int RPB = 256 / TPR;
  const int row = blockIdx.x * RPB + threadIdx.x / TPR;
  if (row >= total) return;
  const int z = seg_find(pre, nsess, row);
  const int* e = tab + 6 * z;
  const int j = row - pre[z], k0 = e[2], nf = e[3], slot = e[4], s0 = e[5];
  E* crow = cache + ((size_t)slot * slot_rows + j) * W;
  if constexpr (W >= 4) {
    using f32x4 = __attribute__((ext_vector_type(4))) float;
    const int c = (threadIdx.x % TPR) * 4;
    if (j < k0) {
      *reinterpret_cast<f32x4*>(out + (size_t)row * W + c) = *reinterpret_cast<const f32x4*>(crow + c);
    } else {
      const f32x4 v = *reinterpret_cast<const f32x4*>(stk + (size_t)(s0 + j - k0) * W + c);
      *reinterpret_cast<f32x4*>(out + (size_t)row * W + c) = v;
      if (j < nf) *reinterpret_cast<f32x4*>(crow + c) = v;
    }
  } else {
    if (j < k0) {
      out[row] = crow[0];
    } else {
      const E v = stk[s0 + j - k0];
      out[row] = v;
      if (j < nf) crow[0] = v;
    }
  }
}

// Stack the rows the CTC heads still have to see: stacked row r of segment z (rows pre[z] ..) is packed row src[z] + r - pre[z].
__global__ __launch_bounds__(256) void pool_stack_rows_kernel(float* out, const float* enc, int W, const int* src, const int* pre,
                                                              int nsess, int total) {
  using f32x4 = __attribute__((ext_vector_type(4))) float;
  const int tpr = W / 4, rpb = 256 / tpr;
  const int row = blockIdx.x * rpb + threadIdx.x / tpr;
  if (row >= total || (int)threadIdx.x >= rpb * tpr) return;
  const int z = seg_find(pre, nsess, row);
  const int c = (threadIdx.x % tpr) * 4;
  *reinterpret_cast<f32x4*>(out + (size_t)row * W + c) =
      *reinterpret_cast<const f32x4*>(enc + (size_t)(src[z] + row - pre[z]) * W + c);
}

}  // namespace

// ---- launchers (the pool step below and the ss_op_pool_* entry points at the foot share them) ----------------------------------
// max_n: the most tail rows of any session of the call (grid sizing); sess: nsess x 8 ints as pool_dwconv_kernel reads them
static int launch_pool_dwconv(const float* gs, float* cache, int slot_rows, float* y, const float* wt, int K, const float* bn_mean,
                              const float* bn_var, const float* bn_gamma, const float* bn_beta, float bn_eps, int C, const int* sess,
                              int nsess, int max_n, hipStream_t s) {
  if (K > PDW_KMAX || (K & 1) == 0 || nsess <= 0 || C <= 0 || slot_rows <= 0) return SS_ERR_ARG;
  if (max_n <= 0) return SS_OK;
  hipLaunchKernelGGL(pool_dwconv_kernel, dim3(cdiv(C, PDW_TC), cdiv(max_n, PDW_TT), nsess), dim3(256), 0, s, gs, cache, slot_rows, y, wt,
                     K, bn_mean, bn_var, bn_gamma, bn_beta, bn_eps, C, sess);
  SS_LAUNCH_CHECK();
  return SS_OK;
}
// float rows of W = 256 (the only width the kernel is instantiated for) / one int32 per row
static int launch_pool_gather_rows(float* out, const float* stk, float* cache, int slot_rows, int W, const int* tab, const int* pre,
                                   int nsess, int total, hipStream_t s) {
  if (W != 256 || nsess <= 0 || slot_rows <= 0) return SS_ERR_ARG;
  if (total <= 0) return SS_OK;
  hipLaunchKernelGGL((pool_gather_kernel<float, 256>), dim3(cdiv(total, 4)), dim3(256), 0, s, out, stk, cache, slot_rows, tab, pre, nsess,
                     total);
  SS_LAUNCH_CHECK();
  return SS_OK;
}
static int launch_pool_gather_ids(int32_t* out, const int32_t* stk, int32_t* cache, int slot_rows, const int* tab, const int* pre,
                                  int nsess, int total, hipStream_t s) {
  if (nsess <= 0 || slot_rows <= 0) return SS_ERR_ARG;
  if (total <= 0) return SS_OK;
  hipLaunchKernelGGL((pool_gather_kernel<int32_t, 1>), dim3(cdiv(total, 256)), dim3(256), 0, s, out, stk, cache, slot_rows, tab, pre,
                     nsess, total);
  SS_LAUNCH_CHECK();
  return SS_OK;
}
// W floats per row: whole float4s, at most one 256-thread workgroup per row (also ctc_stream.hip's: the rows a search has not consumed)
int launch_pool_stack_rows(float* out, const float* enc, int W, const int* src, const int* pre, int nsess, int total,
                                  hipStream_t s) {
  if (W <= 0 || (W & 3) != 0 || W > 1024 || nsess <= 0) return SS_ERR_ARG;
  if (total <= 0) return SS_OK;
  hipLaunchKernelGGL(pool_stack_rows_kernel, dim3(cdiv(total, 256 / (W / 4))), dim3(256), 0, s, out, enc, W, src, pre, nsess, total);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// ---- the pool ----------------------------------------------------------------------------------------------------------------
struct PoolSlot {
  int fin = 0, achunk = -1, cchunk = -1, tail = 0;   // as ss_scratch::es_final / es_achunk / es_cchunk / es_tail
  int T2 = 0, nf = 0;                                  // rows of the last forward's output and the final ones among them (CTC calls)
  int cfin[2] = {0, 0};                                // rows whose raw CTC arg-max of head h the slot holds
  int lfin[2] = {0, 0};                                // ... and whose arg-max log-probability it holds (ss_stream_pool_set_scores)
};

struct ss_stream_pool {
  ss_scratch* sc = nullptr;
  int S = 0, R = 0, L = 0, d = 0;
  DevBuf qkv, glu, out, raw;        // [L][S][R][3d], [L][S][R][d], [S][R][d], [2][S][R] (int32)
  DevBuf lp;                        // [2][S][R] float: the arg-max log-probability of the rows in raw (booked by ss_stream_pool_set_scores)
  bool scores = false;
  std::vector<PoolSlot> slot;
  long long launches = 0, head_rows = 0;
  hipEvent_t done = nullptr;        // recorded behind the last call's work: what ss_stream_pool_destroy waits for
  bool recorded = false;
};

// GEMM-family launches of the process so far (the launchers' own census, prof.hip prof_begin): one per kernel actually launched
static long long gemm_census() {
  long long t = 0;
  for (int c = 0; c < kNumTileCfg; ++c) { long long n = 0; prof_totals(c, nullptr, nullptr, &n); t += n; }
  return t;
}
static int pool_mark(ss_stream_pool* p, hipStream_t s) {
  SS_HIP_CHECK(hipEventRecord(p->done, s));
  p->recorded = true;
  return SS_OK;
}

static void pool_free(ss_stream_pool* p) {
  DevBuf* bufs[5] = {&p->qkv, &p->glu, &p->out, &p->raw, &p->lp};
  for (DevBuf* b : bufs) {
    b->release();
    auto& ex = p->sc->extra;
    ex.erase(std::remove(ex.begin(), ex.end(), b), ex.end());
  }
}

extern "C" int ss_stream_pool_create(ss_model* m, int max_sessions, int max_rows, ss_stream_pool** out) {
  if (!m || !out || max_sessions <= 0 || max_rows <= 0 || max_rows > m->cfg.max_rel_pos || max_sessions > (1 << 16)) return SS_ERR_ARG;
  *out = nullptr;
  const ss_config& c = m->cfg;
  ss_stream_pool* p = new ss_stream_pool();
  p->sc = m->sc; p->S = max_sessions; p->R = max_rows; p->L = c.enc_layers; p->d = c.enc_dim;
  p->slot.resize(max_sessions);
  const size_t rows = (size_t)max_sessions * max_rows;
  DevBuf* bufs[4] = {&p->qkv, &p->glu, &p->out, &p->raw};
  const size_t bytes[4] = {(size_t)p->L * rows * 3 * p->d * sizeof(float), (size_t)p->L * rows * p->d * sizeof(float),
                           rows * p->d * sizeof(float), 2 * rows * sizeof(int32_t)};
  int rc = SS_OK;
  for (int i = 0; i < 4 && rc == SS_OK; ++i) {
    bufs[i]->acct = &p->sc->acct;
    p->sc->extra.push_back(bufs[i]);
    rc = bufs[i]->ensure(bytes[i], true);  // exact sizes: what the header promises per slot and row
  }
  if (rc == SS_OK && hipEventCreateWithFlags(&p->done, hipEventDisableTiming) != hipSuccess) rc = SS_ERR_HIP;
  if (rc != SS_OK) {                       // refused on the cap (or the device): the set is left as it was
    pool_free(p);
    delete p;
    return rc;
  }
  p->sc->refs.fetch_add(1);               // the set lives as long as a pool booked in it
  *out = p;
  return SS_OK;
}

extern "C" void ss_stream_pool_destroy(ss_stream_pool* p) {
  if (!p) return;
  if (p->recorded) (void)hipEventSynchronize(p->done);    // nothing the pool queued may still read or write the slots
  if (p->done) (void)hipEventDestroy(p->done);
  pool_free(p);
  scratch_unref(p->sc);
  delete p;
}

extern "C" int ss_stream_pool_reset(ss_stream_pool* p, int slot) {
  if (!p || slot < 0 || slot >= p->S) return SS_ERR_ARG;
  const int tail = p->slot[slot].tail;
  p->slot[slot] = PoolSlot();
  p->slot[slot].tail = tail;               // (as ss_encoder_stream_reset: the front-end's setting stays)
  return SS_OK;
}

extern "C" int ss_stream_pool_set_tail(ss_stream_pool* p, int slot, int unsettled_fbank_frames) {
  if (!p || slot < 0 || slot >= p->S || unsettled_fbank_frames < 0) return SS_ERR_ARG;
  p->slot[slot].tail = unsettled_fbank_frames;
  return SS_OK;
}

extern "C" int ss_stream_pool_stats(ss_stream_pool* p, int64_t* launches, int64_t* head_rows) {
  if (!p) return SS_ERR_ARG;
  if (launches) *launches = p->launches;
  if (head_rows) *head_rows = p->head_rows;
  return SS_OK;
}

// the layout of one step, planned on the host before anything touches the device
struct PoolPlan {
  struct Sess : StreamRows { int slot, T, q_start, off, h1_off; };
  std::vector<Sess> s;
  std::vector<int> act;       // indices (into s) of the sessions with rows to compute, in call order
  int M = 0, total = 0, H1 = 0, qtiles = 0;
};

static int pool_plan(const ss_stream_pool* p, const ss_config& c, int n, const int32_t* h_slots, const float* const* h_fbank,
                     const int32_t* h_T, const int32_t* h_attn_chunk, const int32_t* h_conv_chunk, PoolPlan& pl) {
  if (n <= 0 || n > p->S || !h_slots || !h_fbank || !h_T || !h_attn_chunk || !h_conv_chunk) return SS_ERR_ARG;
  std::vector<char> seen(p->S, 0);
  pl.s.resize(n);
  for (int i = 0; i < n; ++i) {
    PoolPlan::Sess& e = pl.s[i];
    e.slot = h_slots[i];
    if (e.slot < 0 || e.slot >= p->S || seen[e.slot] || !h_fbank[i] || h_T[i] <= 0) return SS_ERR_ARG;
    seen[e.slot] = 1;
    const PoolSlot& st = p->slot[e.slot];
    e.T = h_T[i];
    if (!stream_rows(c, e.T, h_attn_chunk[i], h_conv_chunk[i], st.fin, st.achunk, st.cchunk, st.tail, p->R, e))
      return SS_ERR_ARG;                                                 // past the pool's rows per slot: the whole call is refused
    e.off = pl.total; pl.total += e.T2;
    e.q_start = pl.M; e.h1_off = pl.H1;
    if (e.n > 0) {
      pl.act.push_back(i);
      pl.M += e.n; pl.H1 += e.T1 - e.mb1; pl.qtiles += cdiv(e.n, 16);
    }
  }
  return SS_OK;
}

extern "C" int ss_encoder_stream_forward_batch(ss_model* m, void* stream, ss_stream_pool* p, int n, const int32_t* h_slots,
                                               const float* const* h_fbank, const int32_t* h_T, const int32_t* h_attn_chunk,
                                               const int32_t* h_conv_chunk, float* d_enc_packed, int32_t* h_n_final,
                                               int32_t* h_n_computed) {
  if (!m || !p || !d_enc_packed || p->sc != m->sc) return SS_ERR_ARG;
  const ss_config& c = m->cfg;
  if (c.enc_layers != p->L || c.enc_dim != p->d || c.enc_heads * 64 != c.enc_dim || c.dw_kernel > PDW_KMAX ||
      (c.dw_kernel & 1) == 0 || c.enc_dim != 256)      // (what launch_pool_dwconv / launch_pool_gather_rows refuse: before anything is queued)
    return SS_ERR_ARG;
  PoolPlan pl;
  RET(pool_plan(p, c, n, h_slots, h_fbank, h_T, h_attn_chunk, h_conv_chunk, pl));
  SkScope sk_scope(m->sc->skws);
  CanonScope canon_scope(CANON_SEQ);        // every row-wise op: a row's bits are a function of that row alone
  hipStream_t s = (hipStream_t)stream;
  const int d = c.enc_dim, f = c.enc_ffn, Ld = c.enc_layers * d, L = c.enc_layers;
  const int Na = (int)pl.act.size(), M = pl.M;

  // ---- tables: one upload.  Pointers first (seg_A), then int32 tables ----
  const size_t n_ptr = Na;
  const size_t n_int = 4 * Na + 2 * Na + 4 * Na + 2 * Na + 8 * Na + (Na + 1) + 6 * n + (n + 1);
  std::vector<unsigned char> blob(n_ptr * sizeof(void*) + n_int * sizeof(int));
  const float** tA = reinterpret_cast<const float**>(blob.data());
  int* ti = reinterpret_cast<int*>(blob.data() + n_ptr * sizeof(void*));
  int *c1 = ti, *mb1 = c1 + 4 * Na, *c2 = mb1 + 2 * Na, *mb2 = c2 + 4 * Na, *ss = mb2 + 2 * Na, *qtp = ss + 8 * Na, *gt = qtp + Na + 1, *gp = gt + 6 * n;
  int mx1 = 0, mx2 = 0, qt = 0;
  for (int a = 0; a < Na; ++a) {
    const PoolPlan::Sess& e = pl.s[pl.act[a]];
    tA[a] = h_fbank[pl.act[a]];
    // conv 1: rows [mb1, T1) of the session into h1 rows h1_off .. (out_start may be negative: rows below mb1 are never written)
    c1[4 * a] = e.h1_off - e.mb1; c1[4 * a + 1] = e.T1; c1[4 * a + 2] = 0; c1[4 * a + 3] = e.T; mb1[2 * a] = e.mb1; mb1[2 * a + 1] = e.cchunk;
    // conv 2: rows [r0, T2) into the stacked tail rows, reading conv 1's rows where conv 1 put them
    c2[4 * a] = e.q_start - e.r0; c2[4 * a + 1] = e.T2; c2[4 * a + 2] = e.h1_off - e.mb1; c2[4 * a + 3] = e.T1; mb2[2 * a] = e.r0; mb2[2 * a + 1] = e.cchunk;
    mx1 = std::max(mx1, e.T1 - e.mb1); mx2 = std::max(mx2, e.n);
    int* r = ss + 8 * a;
    r[0] = e.q_start; r[1] = e.n; r[2] = e.r0; r[3] = e.T2; r[4] = e.slot; r[5] = e.achunk; r[6] = e.cchunk; r[7] = 0;
    qtp[a] = qt; qt += cdiv(e.n, 16);
  }
  qtp[Na] = qt;
  for (int i = 0; i < n; ++i) {
    const PoolPlan::Sess& e = pl.s[i];
    int* r = gt + 6 * i;
    r[0] = e.off; r[1] = e.T2; r[2] = e.r0; r[3] = e.nf; r[4] = e.slot; r[5] = e.q_start;
    gp[i] = e.off;
  }
  gp[n] = pl.total;

  // ---- scratch (grown before anything is queued: a call refused on the cap changes nothing) ----
  const int C1 = c.conv_channels / 2;
  const size_t n_h1 = (size_t)pl.H1 * C1, n_x = (size_t)M * d;
  RET(m->sc->seg_buf.ensure(blob.size()));
  RET(m->sc->ws.ensure((n_h1 + 7 * n_x + (size_t)M * f) * sizeof(float)));
  unsigned char* dblob = reinterpret_cast<unsigned char*>(m->sc->seg_buf.p);
  const float* const* dA = reinterpret_cast<const float* const*>(dblob);
  const int* di = reinterpret_cast<const int*>(dblob + n_ptr * sizeof(void*));
  const int *dc1 = di, *dmb1 = dc1 + 4 * Na, *dc2 = dmb1 + 2 * Na, *dmb2 = dc2 + 4 * Na, *dss = dmb2 + 2 * Na, *dqtp = dss + 8 * Na,
            *dgt = dqtp + Na + 1, *dgp = dgt + 6 * n;
  float* h1 = m->sc->ws.f();
  float* x = h1 + n_h1;                 // running activations of the stacked tail rows
  float* h = x + n_x;                   // subsampler output / LN output / attention context
  float* qkv = h + n_x;                 // stacked q|k|v rows [M][3d]
  float* glu = qkv + 3 * n_x;           // stacked GLU rows
  float* g2 = glu + n_x;                // depthwise output
  float* ff = g2 + n_x;                 // FFN hidden [M][f]
  SS_HIP_CHECK(hipMemcpyAsync(dblob, blob.data(), blob.size(), hipMemcpyHostToDevice, s));
  long long nl = 0;
  const long long g0 = gemm_census();   // the GEMM-family launches of the step are counted where they are launched (below: the others)

  if (M > 0) {
    GemmArgs a, b;
    subsampler_args(m, h_fbank[pl.act[0]], h1, h, a, b);
    a.segs = dc1; a.nseg = Na; a.seg_mb = dmb1; a.seg_A = dA; a.max_seg_out = mx1; a.M = pl.H1; a.in_len = 1; a.canon = CANON_SEQ;
    b.segs = dc2; b.nseg = Na; b.seg_mb = dmb2; b.max_seg_out = mx2; b.M = M; b.in_len = 1; b.canon = CANON_SEQ;
    RET(launch_conv_gemm(a, s));
    RET(launch_conv_gemm(b, s));
    RET(linear(s, h, d, M, m->enc_linear, d, d, x, d));
    PoolAttnArgs at;
    at.Qs = qkv; at.O = h; at.ld = 3 * d; at.ldo = d; at.slot_rows = p->R;
    at.ldp = Ld; at.p_tmax = c.max_rel_pos; at.sess = dss; at.qt_pre = dqtp; at.nsess = Na; at.qtiles = pl.qtiles;
    at.H = c.enc_heads; at.scale = 0.125f;
    const size_t lay_q = (size_t)p->S * p->R * 3 * d, lay_g = (size_t)p->S * p->R * d;
    for (int l = 0; l < L; ++l) {
      const EncLayer& e = m->enc[l];
      auto attention = [&]() -> int {
        at.cache = p->qkv.f() + (size_t)l * lay_q;
        at.P = m->pos_proj + (size_t)l * d; at.bias_u = e.u; at.bias_v = e.v;
        RET(launch_attention_pool(at, s));
        ++nl;
        return SS_OK;
      };
      auto dwconv = [&]() -> int {
        RET(launch_pool_dwconv(glu, p->glu.f() + (size_t)l * lay_g, p->R, g2, e.dw_wt, c.dw_kernel, e.bn_mean, e.bn_var, e.bn_g, e.bn_b,
                               1e-5f, d, dss, Na, mx2, s));
        ++nl;
        return SS_OK;
      };
      RET(enc_layer_ex(s, c, e, x, M, h, ff, qkv, glu, g2, false, false, attention, dwconv));
      ++nl;                                 // (the layer's final LayerNorm)
    }
  }
  if (pl.total > 0) {
    RET(launch_pool_gather_rows(d_enc_packed, x, p->out.f(), p->R, d, dgt, dgp, n, pl.total, s));
    ++nl;
  }
  p->launches += nl + (gemm_census() - g0);
  RET(pool_mark(p, s));
  for (int i = 0; i < n; ++i) {             // commit: the call went through
    const PoolPlan::Sess& e = pl.s[i];
    PoolSlot& st = p->slot[e.slot];
    st.fin = e.nf; st.achunk = e.achunk_cfg; st.cchunk = e.cchunk;
    st.T2 = e.T2; st.nf = e.nf;
    for (int hd = 0; hd < 2; ++hd) {                                             // cached arg-max rows stay valid while final
      st.cfin[hd] = std::min(st.cfin[hd], e.r0);
      st.lfin[hd] = std::min(st.lfin[hd], e.r0);
    }
    if (h_n_final) h_n_final[i] = e.nf;
    if (h_n_computed) h_n_computed[i] = e.n;
  }
  return SS_OK;
}

extern "C" int ss_stream_pool_ctc(ss_model* m, void* stream, ss_stream_pool* p, int head, int n, const int32_t* h_slots,
                                  const float* d_enc_packed, int32_t* d_raw, int32_t* d_tokens, int32_t* d_index,
                                  int32_t* d_counts) {
  if (!m || !p || p->sc != m->sc || head < 0 || head > 1 || n <= 0 || n > p->S || !h_slots || !d_enc_packed || !d_raw || !d_tokens ||
      !d_index || !d_counts || m->cfg.enc_dim != p->d)
    return SS_ERR_ARG;
  const ss_config& c = m->cfg;
  const int d = c.enc_dim, V = head == 0 ? c.src_vocab : c.tgt_vocab;
  std::vector<char> seen(p->S, 0);
  // tables: gather {off, T2, c0, nf, slot, s_start} [6 n], prefix [n + 1], stack src [n], stack prefix [n + 1], collapse {off, T2} [2 n]
  std::vector<int> ti(6 * n + (n + 1) + n + (n + 1) + 2 * n);
  int *gt = ti.data(), *gp = gt + 6 * n, *src = gp + n + 1, *sp = src + n, *cs = sp + n + 1;
  int total = 0, Mc = 0;
  for (int i = 0; i < n; ++i) {
    const int sl = h_slots[i];
    if (sl < 0 || sl >= p->S || seen[sl] || p->slot[sl].T2 <= 0) return SS_ERR_ARG;   // (a slot without a forward since its reset)
    seen[sl] = 1;
    const PoolSlot& st = p->slot[sl];
    const int c0 = std::min(st.cfin[head], st.nf);
    int* r = gt + 6 * i;
    r[0] = total; r[1] = st.T2; r[2] = c0; r[3] = st.nf; r[4] = sl; r[5] = Mc;
    gp[i] = total;
    src[i] = total + c0; sp[i] = Mc;
    cs[2 * i] = total; cs[2 * i + 1] = st.T2;
    total += st.T2; Mc += st.T2 - c0;
  }
  gp[n] = total; sp[n] = Mc;
  SkScope sk_scope(m->sc->skws);
  CanonScope canon_scope(CANON_SEQ);
  hipStream_t s = (hipStream_t)stream;
  RET(m->sc->seg_buf.ensure(ti.size() * sizeof(int)));
  RET(m->sc->mt_ws.ensure((size_t)Mc * V * sizeof(float)));
  RET(m->sc->ws.ensure((size_t)Mc * d * sizeof(float) + (size_t)Mc * sizeof(int32_t)));
  int* dt = (int*)m->sc->seg_buf.p;
  RET(upload(s, dt, ti));
  const int *dgt = dt, *dgp = dgt + 6 * n, *dsrc = dgp + n + 1, *dsp = dsrc + n, *dcs = dsp + n + 1;
  float* stk = m->sc->ws.f();
  int32_t* raw_stk = reinterpret_cast<int32_t*>(stk + (size_t)Mc * d);
  long long nl = 0;
  const long long g0 = gemm_census();
  if (Mc > 0) {              // the rows whose arg-max the slots do not hold yet: stacked, through the head, arg-max
    RET(launch_pool_stack_rows(stk, d_enc_packed, d, dsrc, dsp, n, Mc, s));
    float* logits = nullptr;
    RET(ctc_head_logits(m, s, head, stk, d, Mc, false, &logits));
    RET(launch_masked_argmax(logits, V, Mc, V, c.pad, c.unk, -1, -1, raw_stk, s));
    nl += 2;                 // (the head GEMM: counted by the census)
  }
  RET(launch_pool_gather_ids(d_raw, raw_stk, reinterpret_cast<int32_t*>(p->raw.p) + (size_t)head * p->S * p->R, p->R, dgt, dgp, n, total,
                             s));
  RET(launch_ctc_collapse(d_raw, 0, 0, c.pad, d_tokens, d_index, d_counts, s, dcs, n));
  nl += 2;
  p->launches += nl + (gemm_census() - g0);
  RET(pool_mark(p, s));
  p->head_rows += Mc;
  for (int i = 0; i < n; ++i) { PoolSlot& st = p->slot[h_slots[i]]; st.cfin[head] = st.nf; }
  return SS_OK;
}

// Scores on: the float cache beside p->raw, booked on the pool's scratch set (exact size; refused on the cap, the set as it was).
// Only while no slot holds rows: a slot's cached arg-max rows and their log-probabilities are filled together or not at all.
extern "C" int ss_stream_pool_set_scores(ss_stream_pool* p, int on) {
  if (!p) return SS_ERR_ARG;
  if ((on != 0) == p->scores) return SS_OK;
  for (const PoolSlot& st : p->slot)
    if (st.fin > 0 || st.T2 > 0) return SS_ERR_ARG;
  if (on) {
    p->lp.acct = &p->sc->acct;
    RET(p->lp.ensure(2 * (size_t)p->S * p->R * sizeof(float), true));
    p->sc->extra.push_back(&p->lp);
  } else {
    if (p->recorded) (void)hipEventSynchronize(p->done);
    p->lp.release();
    auto& ex = p->sc->extra;
    ex.erase(std::remove(ex.begin(), ex.end(), &p->lp), ex.end());
  }
  p->scores = on != 0;
  return SS_OK;
}

// ss_stream_pool_ctc with scores: rows below a slot's n_final take their arg-max AND its log-probability from the slot, the rest go
// through the head and the scored arg-max; the float cache goes through the id gather as raw bits (one launch more than the unscored
// call, whatever n), the collapse is the span form.
extern "C" int ss_stream_pool_ctc_scored(ss_model* m, void* stream, ss_stream_pool* p, int head, int n, const int32_t* h_slots,
                                         const float* d_enc_packed, int32_t* d_raw, int32_t* d_tokens, int32_t* d_index,
                                         int32_t* d_counts, float* d_lprob, int32_t* d_last, float* d_tok_lprob) {
  if (!m || !p || p->sc != m->sc || head < 0 || head > 1 || n <= 0 || n > p->S || !h_slots || !d_enc_packed || !d_raw || !d_tokens ||
      !d_index || !d_counts || !d_lprob || !d_last || !d_tok_lprob || m->cfg.enc_dim != p->d || !p->scores)
    return SS_ERR_ARG;
  const ss_config& c = m->cfg;
  const int d = c.enc_dim, V = head == 0 ? c.src_vocab : c.tgt_vocab;
  std::vector<char> seen(p->S, 0);
  // tables as ss_stream_pool_ctc: gather [6 n], prefix [n + 1], stack src [n], stack prefix [n + 1], collapse {off, T2} [2 n]
  std::vector<int> ti(6 * n + (n + 1) + n + (n + 1) + 2 * n);
  int *gt = ti.data(), *gp = gt + 6 * n, *src = gp + n + 1, *sp = src + n, *cs = sp + n + 1;
  int total = 0, Mc = 0;
  for (int i = 0; i < n; ++i) {
    const int sl = h_slots[i];
    if (sl < 0 || sl >= p->S || seen[sl] || p->slot[sl].T2 <= 0) return SS_ERR_ARG;
    seen[sl] = 1;
    const PoolSlot& st = p->slot[sl];
    const int c0 = std::min(std::min(st.cfin[head], st.lfin[head]), st.nf);   // rows the slot holds BOTH values of
    int* r = gt + 6 * i;
    r[0] = total; r[1] = st.T2; r[2] = c0; r[3] = st.nf; r[4] = sl; r[5] = Mc;
    gp[i] = total;
    src[i] = total + c0; sp[i] = Mc;
    cs[2 * i] = total; cs[2 * i + 1] = st.T2;
    total += st.T2; Mc += st.T2 - c0;
  }
  gp[n] = total; sp[n] = Mc;
  SkScope sk_scope(m->sc->skws);
  CanonScope canon_scope(CANON_SEQ);
  hipStream_t s = (hipStream_t)stream;
  RET(m->sc->seg_buf.ensure(ti.size() * sizeof(int)));
  RET(m->sc->mt_ws.ensure((size_t)Mc * V * sizeof(float)));
  RET(m->sc->ws.ensure((size_t)Mc * d * sizeof(float) + (size_t)Mc * (sizeof(int32_t) + sizeof(float))));
  int* dt = (int*)m->sc->seg_buf.p;
  RET(upload(s, dt, ti));
  const int *dgt = dt, *dgp = dgt + 6 * n, *dsrc = dgp + n + 1, *dsp = dsrc + n, *dcs = dsp + n + 1;
  float* stk = m->sc->ws.f();
  int32_t* raw_stk = reinterpret_cast<int32_t*>(stk + (size_t)Mc * d);
  float* lp_stk = reinterpret_cast<float*>(raw_stk + Mc);
  long long nl = 0;
  const long long g0 = gemm_census();
  if (Mc > 0) {
    RET(launch_pool_stack_rows(stk, d_enc_packed, d, dsrc, dsp, n, Mc, s));
    float* logits = nullptr;
    RET(ctc_head_logits(m, s, head, stk, d, Mc, false, &logits));
    RET(launch_masked_argmax_lprob(logits, V, Mc, V, c.pad, c.unk, -1, raw_stk, lp_stk, s));
    nl += 2;
  }
  const size_t hoff = (size_t)head * p->S * p->R;
  RET(launch_pool_gather_ids(d_raw, raw_stk, reinterpret_cast<int32_t*>(p->raw.p) + hoff, p->R, dgt, dgp, n, total, s));
  RET(launch_pool_gather_ids(reinterpret_cast<int32_t*>(d_lprob), reinterpret_cast<const int32_t*>(lp_stk),
                             reinterpret_cast<int32_t*>(p->lp.p) + hoff, p->R, dgt, dgp, n, total, s));   // float bits, moved as int32
  RET(launch_ctc_collapse_spans(d_raw, d_lprob, 0, 0, c.pad, d_tokens, d_index, d_last, d_tok_lprob, d_counts, s, dcs, n));
  nl += 3;
  p->launches += nl + (gemm_census() - g0);
  RET(pool_mark(p, s));
  p->head_rows += Mc;
  for (int i = 0; i < n; ++i) { PoolSlot& st = p->slot[h_slots[i]]; st.cfin[head] = st.nf; st.lfin[head] = st.nf; }
  return SS_OK;
}

// ---- op-level entry points of the pool's own kernels (tests/test_stream_ops_gpu.py): each launcher with the kernel's arguments as the
// pool step passes them; every pointer a DEVICE pointer ----
extern "C" int ss_op_pool_dwconv(void* stream, const float* gs, float* cache, int slot_rows, float* y, const float* wt, int K,
                                 const float* bn_mean, const float* bn_var, const float* bn_gamma, const float* bn_beta, float bn_eps,
                                 int C, const int32_t* sess, int nsess, int max_n) {
  return launch_pool_dwconv(gs, cache, slot_rows, y, wt, K, bn_mean, bn_var, bn_gamma, bn_beta, bn_eps, C, sess, nsess, max_n,
                            (hipStream_t)stream);
}
extern "C" int ss_op_pool_gather_rows(void* stream, float* out, const float* stk, float* cache, int slot_rows, int W, const int32_t* tab,
                                      const int32_t* pre, int nsess, int total) {
  return launch_pool_gather_rows(out, stk, cache, slot_rows, W, tab, pre, nsess, total, (hipStream_t)stream);
}
extern "C" int ss_op_pool_gather_ids(void* stream, int32_t* out, const int32_t* stk, int32_t* cache, int slot_rows, const int32_t* tab,
                                     const int32_t* pre, int nsess, int total) {
  return launch_pool_gather_ids(out, stk, cache, slot_rows, tab, pre, nsess, total, (hipStream_t)stream);
}
extern "C" int ss_op_pool_stack_rows(void* stream, float* out, const float* enc, int W, const int32_t* src, const int32_t* pre, int nsess,
                                     int total) {
  return launch_pool_stack_rows(out, enc, W, src, pre, nsess, total, (hipStream_t)stream);
}
