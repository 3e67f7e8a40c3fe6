// Keyword spotting on the two text CTC heads (blank = 0): did these phrases occur in this audio, and when -- many keywords at once,
// each with a free start and a free end, for a ragged pack (ss_batch_ctc_spot, ss_op_ctc_spot) and for live streams whose state
// stays on the device between calls (ss_ctc_spot_stream_*).  The rule is the header's; the step and the emission rule are
// ctc_spot.hpp's, compiled here for the device and for the host twins.  Three kernels:
//   ctc_spot_gather_kernel  a workgroup per logits row in ctc_row.hpp's thread layout: the row maximum and its NaN flag, then
//                           c = logit - max for the set's U distinct labels alone, a compact [rows][U] float matrix (column 0 the blank)
//   ctc_spot_dp_kernel      lanes are states, a workgroup owns 256 of them (the keywords the set laid there) for one utterance and
//                           walks its frames; neighbours come by wave shuffles, frame rows through LDS, hits by an atomic append
//   ctc_spot_sort_kernel    a workgroup per utterance orders its first min(n, max_hits) records by (end, keyword, start)
#include "ctc_spot.hpp"

#include <algorithm>
#include <atomic>
#include <cstring>
#include <map>
#include <new>

#include "ctc_row.hpp"
#include "model_internal.hpp"

int launch_pool_stack_rows(float* out, const float* enc, int W, const int* src, const int* pre, int nsess, int total,
                           hipStream_t s);   // stream_pool.hip

namespace ss {

// pre[i] = first row of session i among the call's rows, pre[n] = rows (ascending; an empty session repeats its neighbour's).
__global__ __launch_bounds__(256) void ctc_spot_gather_kernel(const float* __restrict__ logits, int ld, int N,
                                                              const int32_t* __restrict__ labels, int U, const int32_t* __restrict__ pre,
                                                              int n, float* __restrict__ cm, ss_ctc_spot_count* counts) {
  __shared__ float sm[4];
  __shared__ int sn[4];
  const int t = threadIdx.x;
  const int row = blockIdx.x;
  const float* r = logits + (size_t)row * ld;
  float v[1];                                                  // (the re-reading form: any N)
  const float mx = ctc_row_max<0>(r, N, v, sm, sn);
  const bool bad = ctc_row_nan(sn) || !(mx > -INFINITY);
  float* out = cm + (size_t)row * U;
  for (int j = t; j < U; j += 256) out[j] = r[labels[j]] - mx;
  if (bad && t == 0) {
    int lo = 0, hi = n - 1;                                    // the last session whose first row is <= row: the one that owns it
    while (lo < hi) {
      const int mid = (lo + hi + 1) >> 1;
      if (pre[mid] <= row) lo = mid; else hi = mid - 1;
    }
    counts[lo].status = 2;
  }
}

// grid (G, n): workgroup (g, i) runs the lanes of the set's workgroup g on session i.  A lane keeps its state's value (float64) and
// start frame in registers over the frames of the call; the lane of a keyword's last state also keeps its pending candidate.  Per
// CTC_SPOT_STAGE frames the workgroup loads, once for all its keywords, the columns it needs of those rows of the compact matrix
// into LDS.  Every lane takes part in every shuffle (the trip counts are uniform); a lane reads a neighbour's value only where that
// neighbour is a state of its own keyword, so a keyword's result does not depend on what shares its wave.
__global__ __launch_bounds__(256) void ctc_spot_dp_kernel(SpotView v, const SpotSess* __restrict__ sess, const float* __restrict__ cm,
                                                          SpotState st, int max_hits, ss_ctc_hit* hits, ss_ctc_spot_count* counts) {
  __shared__ float tile[CTC_SPOT_STAGE][CTC_SPOT_COLS];
  __shared__ int scol[CTC_SPOT_COLS];
  const int tid = threadIdx.x, g = blockIdx.x, i = blockIdx.y;
  const SpotSess se = sess[i];
  const SpotLane ln = v.lanes[(size_t)g * CTC_SPOT_LANES + tid];
  const int nc = v.ncols[g];
  for (int j = tid; j < nc; j += 256) scol[j] = v.cols[(size_t)g * CTC_SPOT_COLS + j];
  const bool fresh = se.f == 0, keep = st.a != nullptr && !se.fin;
  // the utterance's status: what the gather kernel found in this call's rows, and what the slot carries.  Every workgroup of the
  // session computes the same word; workgroup 0 records it.
  int status = counts[i].status;
  if (!fresh && st.a) status |= st.status[se.slot];
  if (g == 0 && tid == 0) {
    counts[i].status = status;
    counts[i].frames = se.upto;
    if (st.a) st.status[se.slot] = status;
  }
  if (status) return;
  const bool active = ln.kw >= 0, last = active && ln.s == ln.S - 1;
  double a = -INFINITY;
  int b = -1;
  SpotPend p{0.0, -1, -1, -1};
  double thr = 0.0;
  int L = 0;
  if (last) { thr = v.kws[ln.kw].thr; L = v.kws[ln.kw].L; }
  if (!fresh && active && st.a) {
    a = st.a[(size_t)se.slot * v.NS + ln.sidx];
    b = st.b[(size_t)se.slot * v.NS + ln.sidx];
    if (last) {
      const size_t q = (size_t)se.slot * v.K + ln.kw;
      p = SpotPend{st.pscore[q], st.pstart[q], st.pend[q], st.plast[q]};
    }
  }
  ss_ctc_hit* out = hits + (size_t)i * max_hits;
  const int nrows = se.upto - se.f;
  for (int t0 = 0; t0 < nrows; t0 += CTC_SPOT_STAGE) {
    __syncthreads();                                           // the tile's last reads (and, the first time, scol's stores)
    const int nt = min(CTC_SPOT_STAGE, nrows - t0);
    for (int idx = tid; idx < nt * nc; idx += 256) {
      const int d = idx / nc, j = idx - d * nc;
      tile[d][j] = cm[(size_t)(se.row0 + t0 + d) * v.U + scol[j]];
    }
    __syncthreads();
    for (int d = 0; d < nt; ++d) {
      const double a1 = __shfl_up(a, 1, 64), a2 = __shfl_up(a, 2, 64);
      const int b1 = __shfl_up(b, 1, 64), b2 = __shfl_up(b, 2, 64);
      if (!active) continue;
      const int t = se.f + t0 + d;
      ctc_spot_step(ln.s, ln.skip != 0, (double)tile[d][ln.col], t, a, b, a1, b1, a2, b2, &a, &b);
      if (last) {
        SpotPend h;
        if (ctc_spot_emit(p, a >= thr, a, b, t, &h)) {
          const int at = atomicAdd(&counts[i].n_hits, 1);
          if (at < max_hits) out[at] = ss_ctc_hit{ln.kw, h.start, h.end, L, h.score};
        }
      }
    }
  }
  if (!active) return;
  if (se.fin) {
    if (last && p.end >= 0) {
      const int at = atomicAdd(&counts[i].n_hits, 1);
      if (at < max_hits) out[at] = ss_ctc_hit{ln.kw, p.start, p.end, L, p.score};
    }
  } else if (keep) {
    st.a[(size_t)se.slot * v.NS + ln.sidx] = a;
    st.b[(size_t)se.slot * v.NS + ln.sidx] = b;
    if (last) {
      const size_t q = (size_t)se.slot * v.K + ln.kw;
      st.pscore[q] = p.score; st.pstart[q] = p.start; st.pend[q] = p.end; st.plast[q] = p.last_end;
    }
  }
}

// A workgroup per utterance: the overflow flag, then a rank sort of the records that were written -- a record's place is the number
// of records before it in (end, keyword, start); two hits of one keyword never share an end, so the places are distinct.
__global__ __launch_bounds__(256) void ctc_spot_sort_kernel(int max_hits, ss_ctc_hit* hits, ss_ctc_hit* copy, ss_ctc_spot_count* counts) {
  const int i = blockIdx.x, tid = threadIdx.x;
  const int n = counts[i].n_hits, m = min(n, max_hits);
  if (tid == 0) counts[i].overflow = n > max_hits ? 1 : 0;
  ss_ctc_hit* rec = hits + (size_t)i * max_hits;
  ss_ctc_hit* tmp = copy + (size_t)i * max_hits;
  for (int j = tid; j < m; j += 256) tmp[j] = rec[j];
  __syncthreads();
  for (int j = tid; j < m; j += 256) {
    const ss_ctc_hit x = tmp[j];
    int rank = 0;
    for (int k = 0; k < m; ++k) rank += ctc_spot_hit_less(tmp[k], x) ? 1 : 0;
    rec[rank] = x;
  }
}

// The one upload, made by the first device call that needs the table (ss_ctc_spot_set_create itself touches no device).  The table
// lives on the device that is current at that call and the set serves that device: a call with another device current is refused.
int spot_device_view(const ss_ctc_spot_set* cset, SpotView* out) {
  ss_ctc_spot_set* set = const_cast<ss_ctc_spot_set*>(cset);
  std::lock_guard<std::mutex> lk(set->mu);
  int cur = -1;
  SS_HIP_CHECK(hipGetDevice(&cur));
  if (set->d_mem && cur != set->device) return SS_ERR_ARG;
  if (!set->d_mem) {
    const SpotTable& t = set->host;
    const size_t nk = t.kws.size() * sizeof(SpotKw), nl = t.lanes.size() * sizeof(SpotLane), nu = t.labels.size() * 4,
                 ncl = t.cols.size() * 4, nn = t.ncols.size() * 4;
    std::vector<unsigned char> img(nk + nl + nu + ncl + nn);
    memcpy(img.data(), t.kws.data(), nk);
    memcpy(img.data() + nk, t.lanes.data(), nl);
    memcpy(img.data() + nk + nl, t.labels.data(), nu);
    memcpy(img.data() + nk + nl + nu, t.cols.data(), ncl);
    memcpy(img.data() + nk + nl + nu + ncl, t.ncols.data(), nn);
    void* d_mem = nullptr;
    SS_HIP_CHECK(hipMalloc(&d_mem, img.size()));
    const hipError_t e = hipMemcpy(d_mem, img.data(), img.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) { (void)hipFree(d_mem); SS_HIP_CHECK(e); }
    unsigned char* d = static_cast<unsigned char*>(d_mem);
    set->dev = SpotView{reinterpret_cast<const SpotKw*>(d), reinterpret_cast<const SpotLane*>(d + nk),
                        reinterpret_cast<const int32_t*>(d + nk + nl), reinterpret_cast<const int32_t*>(d + nk + nl + nu),
                        reinterpret_cast<const int32_t*>(d + nk + nl + nu + ncl), t.K, t.U, t.G, t.NS};
    set->d_mem = d_mem;
    set->device = cur;
  }
  *out = set->dev;
  return SS_OK;
}

static size_t up8(size_t x) { return (x + 7) & ~(size_t)7; }

// ss_debug_ctc_spot_phases: which of the three kernels launch_ctc_spot launches (bit 0 gather, 1 DP, 2 sort; 7 = all).  A
// measuring knob (tools/ctc_spot_bench.py times the kernels apart with it); anything but 7 gives no valid records, for EVERY
// caller of the process until it is set back: one word, read once per call.
static std::atomic<int> g_spot_phases{7};

size_t spot_work_bytes(const ss_ctc_spot_set* set, int rows, int n, int max_hits) {
  return up8((size_t)rows * set->host.U * sizeof(float)) + (size_t)n * max_hits * sizeof(ss_ctc_hit) + up8((size_t)n * sizeof(SpotSess)) +
         up8(((size_t)n + 1) * sizeof(int32_t));
}

int launch_ctc_spot(const ss_ctc_spot_set* set, const float* logits, int ld, int rows, int n, const SpotSess* h_sess, void* d_work,
                    const SpotState& state, int max_hits, ss_ctc_hit* d_hits, ss_ctc_spot_count* d_counts, hipStream_t stream) {
  if (!set || n <= 0 || !h_sess || !d_work || max_hits < 1 || !d_hits || !d_counts || (rows > 0 && (!logits || ld < set->V)))
    return SS_ERR_ARG;
  SpotView dev;
  RET(spot_device_view(set, &dev));
  unsigned char* w = static_cast<unsigned char*>(d_work);
  float* cm = reinterpret_cast<float*>(w);
  w += up8((size_t)rows * dev.U * sizeof(float));
  ss_ctc_hit* copy = reinterpret_cast<ss_ctc_hit*>(w);
  w += (size_t)n * max_hits * sizeof(ss_ctc_hit);
  SpotSess* d_sess = reinterpret_cast<SpotSess*>(w);
  w += up8((size_t)n * sizeof(SpotSess));
  int32_t* d_pre = reinterpret_cast<int32_t*>(w);
  const int phases = g_spot_phases.load(std::memory_order_relaxed);
  std::vector<int32_t> pre(n + 1);
  for (int i = 0; i < n; ++i) pre[i] = h_sess[i].row0;
  pre[n] = rows;
  SS_HIP_CHECK(hipMemcpyAsync(d_sess, h_sess, (size_t)n * sizeof(SpotSess), hipMemcpyHostToDevice, stream));
  SS_HIP_CHECK(hipMemcpyAsync(d_pre, pre.data(), pre.size() * sizeof(int32_t), hipMemcpyHostToDevice, stream));
  SS_HIP_CHECK(hipMemsetAsync(d_counts, 0, (size_t)n * sizeof(ss_ctc_spot_count), stream));
  if (rows > 0 && (phases & 1)) {
    hipLaunchKernelGGL(ctc_spot_gather_kernel, dim3(rows), dim3(256), 0, stream, logits, ld, set->V, dev.labels, dev.U, d_pre, n, cm,
                       d_counts);
    SS_LAUNCH_CHECK();
  }
  if (phases & 2) {
    hipLaunchKernelGGL(ctc_spot_dp_kernel, dim3(dev.G, n), dim3(256), 0, stream, dev, d_sess, cm, state, max_hits, d_hits, d_counts);
    SS_LAUNCH_CHECK();
  }
  if (phases & 4) {
    hipLaunchKernelGGL(ctc_spot_sort_kernel, dim3(n), dim3(256), 0, stream, max_hits, d_hits, copy, d_counts);
    SS_LAUNCH_CHECK();
  }
  return SS_OK;
}

// The refusals of the one-shot calls past their pointers; fills the sessions (every one fresh and final).
static int spot_plan(int B, const int32_t* h_T, int max_hits, std::vector<SpotSess>& sess, int* rows) {
  if (B <= 0 || B > SS_CTC_SPOT_MAX_UTTERANCES || !h_T || max_hits < 1 || max_hits > SS_CTC_SPOT_MAX_HITS) return SS_ERR_ARG;
  sess.resize(B);
  int total = 0;
  for (int b = 0; b < B; ++b) {
    if (h_T[b] < 1 || h_T[b] > SS_CTC_ALIGN_MAX_FRAMES) return SS_ERR_ARG;
    sess[b] = SpotSess{b, total, 0, h_T[b], 1, 0};
    total += h_T[b];
  }
  *rows = total;
  return SS_OK;
}

// The records of one utterance in the returned order, cut to max_hits (the twins).
static void spot_host_write(std::vector<ss_ctc_hit>& hits, int status, int frames, int max_hits, ss_ctc_hit* out, ss_ctc_spot_count* cnt) {
  std::sort(hits.begin(), hits.end(), [](const ss_ctc_hit& x, const ss_ctc_hit& y) { return ctc_spot_hit_less(x, y); });
  const int n = status ? 0 : (int)hits.size();
  for (int j = 0; j < n && j < max_hits; ++j) out[j] = hits[j];
  *cnt = ss_ctc_spot_count{n, status, n > max_hits ? 1 : 0, frames};
}

}  // namespace ss

using namespace ss;

extern "C" int ss_ctc_spot_set_create(int n_keywords, const int32_t* h_tokens, const int32_t* h_off, const float* h_tau, int V, int pad,
                                      int unk, ss_ctc_spot_set** out) {
  if (!out) return SS_ERR_ARG;
  *out = nullptr;
  SpotTable t;                                                 // (the object is made only of a set that passed every check)
  RET(spot_build(n_keywords, h_tokens, h_off, h_tau, V, pad, unk, t));
  ss_ctc_spot_set* set = new (std::nothrow) ss_ctc_spot_set();
  if (!set) return SS_ERR_ARG;
  set->host = std::move(t);
  set->V = V; set->pad = pad; set->unk = unk;
  set->d_bytes = set->host.table_bytes();
  *out = set;
  return SS_OK;
}

extern "C" void ss_ctc_spot_set_destroy(ss_ctc_spot_set* set) {
  if (!set) return;
  if (set->d_mem) (void)hipFree(set->d_mem);
  delete set;
}

extern "C" int ss_ctc_spot_set_info(const ss_ctc_spot_set* set, int32_t* n_keywords, int32_t* n_labels, int64_t* states,
                                    int32_t* workgroups, int64_t* device_bytes) {
  if (!set) return SS_ERR_ARG;
  if (n_keywords) *n_keywords = set->host.K;
  if (n_labels) *n_labels = set->host.U;
  if (states) *states = set->host.NS;
  if (workgroups) *workgroups = set->host.G;
  if (device_bytes) *device_bytes = (int64_t)set->d_bytes;
  return SS_OK;
}

extern "C" int ss_ctc_spot_host(const float* h_logits, int ld, int B, const int32_t* h_T, const ss_ctc_spot_set* set, int max_hits,
                                ss_ctc_hit* h_hits, ss_ctc_spot_count* h_counts) {
  if (!h_logits || !set || ld < set->V || !h_hits || !h_counts) return SS_ERR_ARG;
  std::vector<SpotSess> sess;
  int rows = 0;
  RET(spot_plan(B, h_T, max_hits, sess, &rows));
  for (int b = 0; b < B; ++b) {
    SpotHostState st;
    st.start(set->host.NS, set->host.K);
    std::vector<ss_ctc_hit> hits;
    spot_host_run(set->host, h_logits + (size_t)sess[b].row0 * ld, ld, set->V, 0, h_T[b], true, st, hits);
    spot_host_write(hits, st.status, h_T[b], max_hits, h_hits + (size_t)b * max_hits, h_counts + b);
  }
  return SS_OK;
}

extern "C" int ss_debug_ctc_spot_phases(int mask) {
  if (mask < 0 || mask > 7) return SS_ERR_ARG;
  g_spot_phases.store(mask, std::memory_order_relaxed);
  return SS_OK;
}

extern "C" int ss_debug_ctc_spot_trace_host(const float* h_logits, int ld, int T, const ss_ctc_spot_set* set, double* h_e, int32_t* h_start) {
  if (!h_logits || !set || ld < set->V || T < 1 || T > SS_CTC_ALIGN_MAX_FRAMES || !h_e || !h_start) return SS_ERR_ARG;
  SpotHostState st;
  st.start(set->host.NS, set->host.K);
  std::vector<ss_ctc_hit> hits;
  spot_host_run(set->host, h_logits, ld, set->V, 0, T, true, st, hits, h_e, h_start);
  return st.status ? SS_ERR_ARG : SS_OK;
}

extern "C" int ss_op_ctc_spot(void* stream, const float* d_logits, int ld, int B, const int32_t* h_T, const ss_ctc_spot_set* set,
                              int max_hits, ss_ctc_hit* d_hits, ss_ctc_spot_count* d_counts) {
  if (!d_logits || !set || ld < set->V || !d_hits || !d_counts) return SS_ERR_ARG;
  std::vector<SpotSess> sess;
  int rows = 0;
  RET(spot_plan(B, h_T, max_hits, sess, &rows));
  static thread_local std::map<hipStream_t, DevBuf> tmps;      // scratch as ss_op_ctc_align's: a buffer per stream of the calling thread
  DevBuf& tmp = tmps[(hipStream_t)stream];
  RET(tmp.ensure(spot_work_bytes(set, rows, B, max_hits)));
  return launch_ctc_spot(set, d_logits, ld, rows, B, sess.data(), tmp.p, SpotState{}, max_hits, d_hits, d_counts, (hipStream_t)stream);
}

// ss_batch_ctc_align's packing, head GEMM (the same linear, CanonScope and workspace) and scratch booking, then the three kernels.
// Every refusal comes before the first launch; the compact matrix, the sort's copy and the tables live in the encoder scratch (idle
// here: d_enc_out is the caller's).
extern "C" int ss_batch_ctc_spot(ss_model* m, void* stream, int head, int B, const float* d_enc_out, const int32_t* h_Tp,
                                 const ss_ctc_spot_set* set, int max_hits, ss_ctc_hit* d_hits, ss_ctc_spot_count* d_counts) {
  if (!m || head < 0 || head > 1 || !d_enc_out || !h_Tp || !set || !d_hits || !d_counts) return SS_ERR_ARG;
  const ss_config& c = m->cfg;
  const int V = head == 0 ? c.src_vocab : c.tgt_vocab;
  if (set->V != V || set->pad != c.pad || set->unk != c.unk) return SS_ERR_ARG;
  std::vector<SpotSess> sess;
  int rows = 0;
  RET(spot_plan(B, h_Tp, max_hits, sess, &rows));
  SkScope sk_scope(m->sc->skws);
  CanonScope canon_scope(m->pack_invariant ? CANON_SEQ : CANON_NONE);
  hipStream_t s = (hipStream_t)stream;
  RET(m->sc->mt_ws.ensure((size_t)rows * V * sizeof(float)));
  RET(m->sc->ws.ensure(spot_work_bytes(set, rows, B, max_hits)));
  float* logits = nullptr;
  RET(ctc_head_logits(m, s, head, d_enc_out, c.enc_dim, rows, true, &logits));
  return launch_ctc_spot(set, logits, V, rows, B, sess.data(), m->sc->ws.p, SpotState{}, max_hits, d_hits, d_counts, s);
}

// ---- the resumable form ----

struct ss_ctc_spot_stream {
  const ss_ctc_spot_set* set = nullptr;
  int head = -1, S = 0;
  ss_scratch* sc = nullptr;          // the set the state is booked on (ss_ctc_spot_stream_create), else null
  bool on_device = false;
  DevBuf buf;                        // the slots' state, spot_state_carve'd into dev
  SpotState dev{};
  std::vector<SpotHostState> host;   // ... or the twin's, one per slot
  std::vector<int> frames;           // frames consumed per slot
};

namespace {

int spot_stream_make(const ss_ctc_spot_set* set, int max_sessions, bool on_device, ScratchAcct* acct, ss_ctc_spot_stream** out) {
  if (!set || max_sessions <= 0 || max_sessions > SS_CTC_SPOT_MAX_UTTERANCES) return SS_ERR_ARG;
  ss_ctc_spot_stream* ks = new ss_ctc_spot_stream();
  ks->set = set; ks->S = max_sessions;
  ks->frames.assign(max_sessions, 0);
  if (on_device) {
    ks->buf.acct = acct;
    const int rc = ks->buf.ensure(spot_state_bytes(max_sessions, set->host.NS, set->host.K), true);   // exact size; refused on the cap
    if (rc != SS_OK) { delete ks; return rc; }
    ks->dev = spot_state_carve(ks->buf.p, max_sessions, set->host.NS, set->host.K);
    ks->on_device = true;
  } else {
    ks->host.resize(max_sessions);
  }
  *out = ks;
  return SS_OK;
}

// Every refusal of an advance past its pointers (ss_ctc_stream_advance's); fills the sessions and the number of stacked new rows.
int spot_stream_check(const ss_ctc_spot_stream* ks, int n, const int32_t* h_slots, const int32_t* h_T, const int32_t* h_upto,
                      const int32_t* h_final, int max_hits, std::vector<SpotSess>& sess, int* rows) {
  if (n <= 0 || n > ks->S || max_hits < 1 || max_hits > SS_CTC_SPOT_MAX_HITS) return SS_ERR_ARG;
  std::vector<char> seen(ks->S, 0);
  sess.resize(n);
  int total = 0;
  for (int i = 0; i < n; ++i) {
    const int sl = h_slots[i];
    if (sl < 0 || sl >= ks->S || seen[sl]) return SS_ERR_ARG;
    seen[sl] = 1;
    const int f = ks->frames[sl], upto = h_upto[i];
    if (upto < f || (h_T && upto > h_T[i]) || upto > SS_CTC_ALIGN_MAX_FRAMES) return SS_ERR_ARG;
    sess[i] = SpotSess{sl, total, f, upto, h_final[i] != 0 ? 1 : 0, 0};
    total += upto - f;
  }
  *rows = total;
  return SS_OK;
}

void spot_stream_commit(ss_ctc_spot_stream* ks, const std::vector<SpotSess>& sess) {
  for (const SpotSess& se : sess) ks->frames[se.slot] = se.fin ? 0 : se.upto;
}

}  // namespace

extern "C" int ss_ctc_spot_stream_create(ss_model* m, int head, int max_sessions, const ss_ctc_spot_set* set, ss_ctc_spot_stream** out) {
  if (!out) return SS_ERR_ARG;
  *out = nullptr;
  if (!m || head < 0 || head > 1 || !set || (m->cfg.enc_dim & 3) != 0 || m->cfg.enc_dim > 1024) return SS_ERR_ARG;
  const ss_config& c = m->cfg;
  if (set->V != (head == 0 ? c.src_vocab : c.tgt_vocab) || set->pad != c.pad || set->unk != c.unk) return SS_ERR_ARG;
  ss_ctc_spot_stream* ks = nullptr;
  RET(spot_stream_make(set, max_sessions, true, &m->sc->acct, &ks));
  ks->head = head;
  ks->sc = m->sc;
  ks->sc->extra.push_back(&ks->buf);
  ks->sc->refs.fetch_add(1);                // the set lives as long as an object booked in it
  *out = ks;
  return SS_OK;
}

extern "C" int ss_debug_ctc_spot_stream_create(const ss_ctc_spot_set* set, int on_device, int max_sessions, ss_ctc_spot_stream** out) {
  if (!out) return SS_ERR_ARG;
  *out = nullptr;
  return spot_stream_make(set, max_sessions, on_device != 0, nullptr, out);
}

extern "C" void ss_ctc_spot_stream_destroy(ss_ctc_spot_stream* ks) {
  if (!ks) return;
  ks->buf.release();                        // (hipFree waits for whatever still reads or writes the slots)
  if (ks->sc) {
    auto& ex = ks->sc->extra;
    ex.erase(std::remove(ex.begin(), ex.end(), &ks->buf), ex.end());
    scratch_unref(ks->sc);
  }
  delete ks;
}

extern "C" int ss_ctc_spot_stream_reset(ss_ctc_spot_stream* ks, int slot) {
  if (!ks || slot < 0 || slot >= ks->S) return SS_ERR_ARG;
  ks->frames[slot] = 0;
  return SS_OK;
}

extern "C" int ss_ctc_spot_stream_advance(ss_model* m, void* stream, ss_ctc_spot_stream* ks, int n, const int32_t* h_slots,
                                          const float* d_enc_packed, const int32_t* h_T, const int32_t* h_upto, const int32_t* h_final,
                                          int max_hits, ss_ctc_hit* d_hits, ss_ctc_spot_count* d_counts) {
  if (!m || !ks || !ks->sc || ks->sc != m->sc || !h_slots || !d_enc_packed || !h_T || !h_upto || !h_final || !d_hits || !d_counts)
    return SS_ERR_ARG;
  const ss_config& c = m->cfg;
  const int d = c.enc_dim, V = ks->set->V;
  if (V != (ks->head == 0 ? c.src_vocab : c.tgt_vocab)) return SS_ERR_ARG;
  std::vector<SpotSess> sess;
  int rows = 0;
  RET(spot_stream_check(ks, n, h_slots, h_T, h_upto, h_final, max_hits, sess, &rows));
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
  const size_t stk_bytes = ((size_t)rows * d * sizeof(float) + 7) & ~(size_t)7;
  RET(m->sc->seg_buf.ensure(ti.size() * sizeof(int)));
  RET(m->sc->mt_ws.ensure((size_t)rows * V * sizeof(float)));
  RET(m->sc->ws.ensure(stk_bytes + spot_work_bytes(ks->set, rows, n, max_hits)));
  float* logits = m->sc->mt_ws.f();         // (a call without new rows launches no head; the kernels read no row then)
  float* stk = m->sc->ws.f();
  if (rows > 0) {
    int* dti = static_cast<int*>(m->sc->seg_buf.p);
    SS_HIP_CHECK(hipMemcpyAsync(dti, ti.data(), ti.size() * sizeof(int), hipMemcpyHostToDevice, s));
    RET(launch_pool_stack_rows(stk, d_enc_packed, d, dti, dti + n, n, rows, s));
    RET(ctc_head_logits(m, s, ks->head, stk, d, rows, false, &logits));
  }
  RET(launch_ctc_spot(ks->set, logits, V, rows, n, sess.data(), static_cast<unsigned char*>(m->sc->ws.p) + stk_bytes, ks->dev, max_hits,
                      d_hits, d_counts, s));
  spot_stream_commit(ks, sess);
  return SS_OK;
}

extern "C" int ss_op_ctc_spot_stream_advance(void* stream, ss_ctc_spot_stream* ks, int n, const int32_t* h_slots, const float* d_logits,
                                             int ld, const int32_t* h_upto, const int32_t* h_final, int max_hits, ss_ctc_hit* d_hits,
                                             ss_ctc_spot_count* d_counts) {
  if (!ks || !ks->on_device || ks->sc || !h_slots || !d_logits || ld < ks->set->V || !h_upto || !h_final || !d_hits || !d_counts)
    return SS_ERR_ARG;
  std::vector<SpotSess> sess;
  int rows = 0;
  RET(spot_stream_check(ks, n, h_slots, nullptr, h_upto, h_final, max_hits, sess, &rows));
  static thread_local std::map<hipStream_t, DevBuf> tmps;
  DevBuf& tmp = tmps[(hipStream_t)stream];
  RET(tmp.ensure(spot_work_bytes(ks->set, rows, n, max_hits)));
  RET(launch_ctc_spot(ks->set, d_logits, ld, rows, n, sess.data(), tmp.p, ks->dev, max_hits, d_hits, d_counts, (hipStream_t)stream));
  spot_stream_commit(ks, sess);
  return SS_OK;
}

extern "C" int ss_ctc_spot_stream_advance_host(ss_ctc_spot_stream* ks, int n, const int32_t* h_slots, const float* h_logits, int ld,
                                               const int32_t* h_upto, const int32_t* h_final, int max_hits, ss_ctc_hit* h_hits,
                                               ss_ctc_spot_count* h_counts) {
  if (!ks || ks->on_device || ks->host.empty() || !h_slots || !h_logits || ld < ks->set->V || !h_upto || !h_final || !h_hits || !h_counts)
    return SS_ERR_ARG;
  std::vector<SpotSess> sess;
  int rows = 0;
  RET(spot_stream_check(ks, n, h_slots, nullptr, h_upto, h_final, max_hits, sess, &rows));
  const SpotTable& t = ks->set->host;
  for (int i = 0; i < n; ++i) {
    const SpotSess& se = sess[i];
    SpotHostState& st = ks->host[se.slot];
    if (se.f == 0) st.start(t.NS, t.K);
    std::vector<ss_ctc_hit> hits;
    spot_host_run(t, h_logits + (size_t)se.row0 * ld, ld, ks->set->V, se.f, se.upto, se.fin != 0, st, hits);
    spot_host_write(hits, st.status, se.upto, max_hits, h_hits + (size_t)i * max_hits, h_counts + i);
  }
  spot_stream_commit(ks, sess);
  return SS_OK;
}
