// Unit spans (include/streamspeech_hip.h, "Unit spans"): which CTC units of the unit decoder's arg-max belong to which text-decoder
// state, and where their speech lies on the clock of the emitted vocoder frames.  The unit decoder upsamples every state into `up`
// positions, so a unit (the first frame of a run of equal ids that is none of blank / pad / bos / eos: what ctc_collapse_kernel plus
// the host's dictionary walk keep) belongs to state f / up.  One kernel for a whole ragged call, one workgroup per row; the plain-C++
// twin (ss_unit_spans_host) loops over rows with the same definitions.  Integers only.
#include <algorithm>
#include <cstring>
#include <map>
#include <mutex>
#include <vector>

#include "model_internal.hpp"

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;

// One row as the kernel sees it.
struct SpanRow {
  int32_t raw_off;     // first arg-max id of the row in the packed raw array
  int32_t n;           // states
  int32_t dur_off;     // dur[dur_off + j - d0] = the frames of unit ordinal j
  int32_t d0, u0;      // first unit with a duration; first NEW unit
  int32_t K;           // the units the caller counted: no duration is read at or past it
  int32_t span_off;    // first state of the row in the packed spans
  int32_t reserved;
};
static_assert(sizeof(SpanRow) == 32, "SpanRow is 32 bytes");

// A thread per frame, chunks of 1024 frames.  Three running sums go through the chunk: the units (their ordinals decide which are
// new and which duration is theirs), the new units, and the frames of the new units (the clock).  The first two are ballots, the
// clock is a shuffle scan inside the wave; the wave totals and the carries between chunks go through LDS, as ctc_collapse_kernel
// carries its offset.  The thread on a state's LAST frame writes the state's four numbers in one 16-byte store: the sums before the
// state's first frame lie in this chunk's LDS, or -- when the state began in an earlier chunk -- in the two carried "open" values.
// States are ordered, so nothing is accumulated in memory: no atomics, every span written exactly once, zeros included.
__global__ __launch_bounds__(kThreads) void unit_spans_kernel(const int* __restrict__ raw, const SpanRow* __restrict__ rows,
                                                              const int* __restrict__ dur, int up, int blank, int pad, int bos,
                                                              int eos, int4* __restrict__ spans, int* __restrict__ K_out) {
  __shared__ int ex_n[kThreads + 1], ex_c[kThreads + 1];   // new units / frames before each frame of the chunk; [1024]: after it
  __shared__ int wt_u[kWaves], wt_n[kWaves], wt_c[kWaves];
  __shared__ int base[3];                                  // units, new units, frames before the chunk
  __shared__ int open_[2];                                 // new units, frames before the state that holds the chunk's first frame
  const SpanRow r = rows[blockIdx.x];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int* x = raw + r.raw_off;
  const int* du = dur + r.dur_off;
  int4* out = spans + r.span_off;
  const int T = r.n * up;                                  // fits an int: checked on the host
  if (t == 0) { base[0] = base[1] = base[2] = 0; open_[0] = open_[1] = 0; }
  __syncthreads();
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int c0 = 0; c0 < T; c0 += kThreads) {
    const int f = c0 + t;
    bool unit = false;
    if (f < T) {
      const int v = x[f];
      unit = v != blank && v != pad && v != bos && v != eos && (f == 0 || v != x[f - 1]);
    }
    const unsigned long long bu = __ballot(unit);
    if (lane == 0) wt_u[wave] = __popcll(bu);
    __syncthreads();
    int ord = base[0] + __popcll(bu & below);
    for (int w = 0; w < wave; ++w) ord += wt_u[w];
    const bool nw = unit && ord >= r.u0;
    const int d = (nw && ord < r.K) ? du[ord - r.d0] : 0;  // a row that holds more units than the caller counted reads no further
    const unsigned long long bn = __ballot(nw);
    int inc = d;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int y = __shfl_up(inc, o, 64);
      if (lane >= o) inc += y;
    }
    if (lane == 63) wt_c[wave] = inc;
    if (lane == 0) wt_n[wave] = __popcll(bn);
    __syncthreads();
    int en = base[1] + __popcll(bn & below), ec = base[2] + inc - d;
    for (int w = 0; w < wave; ++w) { en += wt_n[w]; ec += wt_c[w]; }
    ex_n[t] = en; ex_c[t] = ec;
    if (t == kThreads - 1) { ex_n[kThreads] = en + (nw ? 1 : 0); ex_c[kThreads] = ec + d; }
    __syncthreads();
    if (f < T && f % up == up - 1) {
      const int fs = f - up + 1;
      const int sn = fs >= c0 ? ex_n[fs - c0] : open_[0], sc = fs >= c0 ? ex_c[fs - c0] : open_[1];
      out[f / up] = make_int4(r.u0 + sn, en + (nw ? 1 : 0) - sn, sc, ec + d - sc);
    }
    __syncthreads();
    if (t == 0) {
      int su = 0;
      for (int w = 0; w < kWaves; ++w) su += wt_u[w];
      base[0] += su; base[1] = ex_n[kThreads]; base[2] = ex_c[kThreads];
      const int fs = (c0 + kThreads) / up * up;            // where the state of the next chunk's first frame begins
      if (fs >= c0) { open_[0] = ex_n[fs - c0]; open_[1] = ex_c[fs - c0]; }
    }
    __syncthreads();
  }
  if (t == 0) K_out[blockIdx.x] = base[0];
}

struct SpanPlan {
  std::vector<SpanRow> rows;
  int64_t states = 0, units = 0;
};

// Every refusal of the three entry points past their own pointers, for the whole call; fills the row table.
int plan(int B, const int32_t* h_n, const int32_t* h_K, const int32_t* h_d0, const int32_t* h_u0, int up, SpanPlan& p) {
  if (B < 1 || !h_n || !h_K || !h_d0 || !h_u0 || up < 1) return SS_ERR_ARG;
  const int64_t lim = (int64_t)0x7fffffff - kThreads;
  p.rows.resize((size_t)B);
  int64_t frames = 0;
  for (int b = 0; b < B; ++b) {
    if (h_n[b] < 1 || h_K[b] < 0 || h_d0[b] < 0 || h_d0[b] > h_u0[b] || h_u0[b] > h_K[b]) return SS_ERR_ARG;
    SpanRow& r = p.rows[(size_t)b];
    r.raw_off = (int32_t)frames; r.n = h_n[b]; r.dur_off = (int32_t)p.units; r.d0 = h_d0[b]; r.u0 = h_u0[b]; r.K = h_K[b];
    r.span_off = (int32_t)p.states; r.reserved = 0;
    frames += (int64_t)h_n[b] * up; p.states += h_n[b]; p.units += h_K[b];
    if (frames > lim || p.units > lim) return SS_ERR_ARG;
  }
  return SS_OK;
}

// The device side of a call: one grow-only buffer per (device, stream), as vad.hip and pcm.hip keep theirs.
struct TableBuf { void* p = nullptr; size_t cap = 0; };
std::mutex g_mu;
std::map<std::pair<int, void*>, TableBuf> g_tables;

int table_for(void* stream, size_t bytes, void** out) {
  int dev = 0;
  SS_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_mu);
  TableBuf& t = g_tables[{dev, stream}];
  if (t.cap < bytes) {
    if (t.p) {
      SS_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));               // an earlier call of this stream may still read it
      SS_HIP_CHECK(hipFree(t.p));
      t.p = nullptr; t.cap = 0;
    }
    const size_t cap = std::max<size_t>(8192, 2 * bytes);
    SS_HIP_CHECK(hipMalloc(&t.p, cap));
    t.cap = cap;
  }
  *out = t.p;
  return SS_OK;
}

size_t round16(size_t x) { return (x + 15) & ~(size_t)15; }

void launch(hipStream_t st, int B, const int32_t* d_raw, const SpanRow* d_rows, const int32_t* d_dur, int up, int blank, int pad,
            int bos, int eos, int32_t* d_spans, int32_t* d_K) {
  hipLaunchKernelGGL(unit_spans_kernel, dim3((unsigned)B), dim3(kThreads), 0, st, d_raw, d_rows, d_dur, up, blank, pad, bos, eos,
                     reinterpret_cast<int4*>(d_spans), d_K);
}

}  // namespace

extern "C" int ss_op_unit_spans(void* stream, int B, const int32_t* d_raw, const int32_t* h_n, const int32_t* h_K,
                                const int32_t* h_dur_first, const int32_t* h_unit0, const int32_t* d_dur, int up, int blank, int pad,
                                int bos, int eos, int32_t* d_spans, int32_t* d_K_out) {
  if (!d_raw || !d_dur || !d_spans || !d_K_out || ((uintptr_t)d_spans & 15)) return SS_ERR_ARG;
  SpanPlan p;
  RET(plan(B, h_n, h_K, h_dur_first, h_unit0, up, p));
  const size_t bytes = p.rows.size() * sizeof(SpanRow);
  void* d_tab = nullptr;
  RET(table_for(stream, bytes, &d_tab));
  hipStream_t st = (hipStream_t)stream;
  SS_HIP_CHECK(hipMemcpyAsync(d_tab, p.rows.data(), bytes, hipMemcpyHostToDevice, st));   // pageable source: staged when the call returns
  launch(st, B, d_raw, (const SpanRow*)d_tab, d_dur, up, blank, pad, bos, eos, d_spans, d_K_out);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

extern "C" int ss_batch_unit_spans(ss_model* m, void* stream, int B, const int32_t* d_raw, const int32_t* h_n, const int32_t* h_K,
                                   const int32_t* h_dur_first, const int32_t* h_unit0, const int32_t* d_dur, const int32_t* h_dur,
                                   int32_t* h_spans, int32_t* h_K_out) {
  if (!m || !d_raw || !h_spans || !h_K_out || (d_dur != nullptr) == (h_dur != nullptr)) return SS_ERR_ARG;
  const ss_config& c = m->cfg;
  SpanPlan p;
  RET(plan(B, h_n, h_K, h_dur_first, h_unit0, c.ctc_upsample, p));
  // one buffer: [row table | host durations] goes up in one copy, [spans | K] comes down in one
  const size_t tab_bytes = p.rows.size() * sizeof(SpanRow);
  const size_t dur_bytes = h_dur ? (size_t)p.units * sizeof(int32_t) : 0;
  const size_t in_bytes = round16(tab_bytes + dur_bytes);
  const size_t span_bytes = (size_t)p.states * 4 * sizeof(int32_t), out_bytes = span_bytes + (size_t)B * sizeof(int32_t);
  void* buf = nullptr;
  RET(table_for(stream, in_bytes + out_bytes, &buf));
  std::vector<unsigned char> up_host(tab_bytes + dur_bytes);
  memcpy(up_host.data(), p.rows.data(), tab_bytes);
  if (dur_bytes) memcpy(up_host.data() + tab_bytes, h_dur, dur_bytes);
  hipStream_t st = (hipStream_t)stream;
  unsigned char* d = static_cast<unsigned char*>(buf);
  SS_HIP_CHECK(hipMemcpyAsync(d, up_host.data(), up_host.size(), hipMemcpyHostToDevice, st));
  const int32_t* dur = h_dur ? reinterpret_cast<const int32_t*>(d + tab_bytes) : d_dur;
  int32_t* d_spans = reinterpret_cast<int32_t*>(d + in_bytes);
  int32_t* d_K = reinterpret_cast<int32_t*>(d + in_bytes + span_bytes);
  launch(st, B, d_raw, reinterpret_cast<const SpanRow*>(d), dur, c.ctc_upsample, c.unit_vocab - 1, c.pad, 0, c.eos, d_spans, d_K);
  SS_LAUNCH_CHECK();
  std::vector<unsigned char> down(out_bytes);
  SS_HIP_CHECK(hipMemcpyAsync(down.data(), d + in_bytes, out_bytes, hipMemcpyDeviceToHost, st));
  SS_HIP_CHECK(hipStreamSynchronize(st));
  memcpy(h_spans, down.data(), span_bytes);
  memcpy(h_K_out, down.data() + span_bytes, (size_t)B * sizeof(int32_t));
  return SS_OK;
}

extern "C" int ss_unit_spans_host(int B, const int32_t* h_raw, const int32_t* h_n, const int32_t* h_K, const int32_t* h_dur_first,
                                  const int32_t* h_unit0, const int32_t* h_dur, int up, int blank, int pad, int bos, int eos,
                                  int32_t* h_spans, int32_t* h_K_out) {
  if (!h_raw || !h_dur || !h_spans || !h_K_out) return SS_ERR_ARG;
  SpanPlan p;
  RET(plan(B, h_n, h_K, h_dur_first, h_unit0, up, p));
  for (int b = 0; b < B; ++b) {
    const SpanRow& r = p.rows[(size_t)b];
    const int32_t* x = h_raw + r.raw_off;
    const int32_t* du = h_dur + r.dur_off;
    int32_t* out = h_spans + 4 * (size_t)r.span_off;
    int ord = 0, units = 0, clock = 0;
    for (int s = 0; s < r.n; ++s) {
      const int n0 = units, c0 = clock;
      for (int f = s * up; f < (s + 1) * up; ++f) {
        const int v = x[f];
        if (v == blank || v == pad || v == bos || v == eos || (f > 0 && v == x[f - 1])) continue;
        if (ord >= r.u0) {
          ++units;
          if (ord < r.K) clock += du[ord - r.d0];
        }
        ++ord;
      }
      out[4 * s] = r.u0 + n0; out[4 * s + 1] = units - n0; out[4 * s + 2] = c0; out[4 * s + 3] = clock - c0;
    }
    h_K_out[b] = ord;
  }
  return SS_OK;
}
