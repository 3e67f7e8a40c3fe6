// Endpointing of live PCM streams (include/streamspeech_hip.h, "Endpointing"): ss_vad_scan runs the energy scan over the new frames
// of every endpointed session of a pool step in ONE launch.  A workgroup owns a segment.  Its four waves compute frame powers in
// parallel -- a wave per frame, lane-strided partial sums and a fixed shuffle tree (vad.hpp), so the order of every addition is the
// host twin's -- in batches of kBatch frames that go through LDS; after each batch one lane walks the noise floor and the state
// machine over it, which is serial by nature (a few dozen instructions per frame), so a backlog of any length needs 1 KB of LDS.
// The frames of a segment overlap (W = 2.5 H for the fbank framing) and are read twice, so a sample is loaded five times; they come
// from L1/L2 after the first, and the whole scan of a step is a few hundred KB.
#include <map>
#include <mutex>
#include <vector>

#include "vad.hpp"

namespace {

using namespace ss::vad;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kLanes;
constexpr int kBatch = 256;                      // frames per LDS batch

static_assert(sizeof(ss_vad_state) == 40, "ss_vad_state is 40 bytes");
static_assert(sizeof(ss_vad_seg) == 96, "ss_vad_seg is 96 bytes");
static_assert(sizeof(ss_vad_result) == 40, "ss_vad_result is 40 bytes");

// One segment as the kernel sees it: the caller's record and 1 / W, divided once on the host for both sides.
struct SegDev {
  ss_vad_seg sg;
  float inv_w;
  int32_t pad;
};
static_assert(sizeof(SegDev) == 104, "SegDev is 104 bytes");

__device__ __forceinline__ float wave_tree(float v) {
#pragma unroll
  for (int o = kLanes / 2; o >= 1; o >>= 1) v = v + __shfl_xor(v, o, kLanes);
  return v;
}

__global__ __launch_bounds__(kThreads) void vad_scan_kernel(const SegDev* __restrict__ segs, ss_vad_result* __restrict__ results) {
  __shared__ float pw[kBatch];
  __shared__ int stop_s;
  const SegDev sd = segs[blockIdx.x];
  const ss_vad_seg& sg = sd.sg;
  const int lane = (int)threadIdx.x & (kLanes - 1), wave = (int)threadIdx.x / kLanes;
  ss_vad_state st;
  ss_vad_result r;
  if (threadIdx.x == 0) {
    st = *sg.state;
    result_init(r, sg, st);
  }
  for (int b0 = 0; b0 < sg.n_frames; b0 += kBatch) {
    const int nb = min(kBatch, sg.n_frames - b0);
    for (int i = wave; i < nb; i += kWaves) {      // wave-uniform: all 64 lanes take part in the shuffles
      const int64_t j = sg.first_frame + b0 + i;
      const float* x = sg.hist + (j * sg.H - sg.hist_first);   // [0, n_hist - W]: checked on the host
      const float m = scaled(wave_tree(lane_sum(x, sg.W, lane)), sd.inv_w);
      const float P = scaled(wave_tree(lane_sq(x, sg.W, lane, m)), sd.inv_w);
      if (lane == 0) pw[i] = P;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      int stop = 0;
      for (int i = 0; i < nb && !stop; ++i) {
        if (sg.powers) sg.powers[b0 + i] = pw[i];
        stop = step(st, r, sg, sg.first_frame + b0 + i, pw[i]) ? 1 : 0;
      }
      stop_s = stop;
    }
    __syncthreads();
    if (stop_s) break;
  }
  if (threadIdx.x == 0) {
    *sg.state = st;
    results[blockIdx.x] = r;
  }
}

// Every refusal of ss_vad_scan / ss_vad_scan_host past the counts, in the header's order.
int scan_check(const ss_vad_seg* h_segs, int n_segs, const void* results) {
  if (!h_segs || !results) return SS_ERR_ARG;
  for (int i = 0; i < n_segs; ++i) {
    const ss_vad_seg& s = h_segs[i];
    if (!s.state || s.reserved != 0) return SS_ERR_ARG;
    if (s.H < 1 || s.W < 1 || s.H > s.W || s.W > (1 << 20)) return SS_ERR_ARG;
    if (s.min_speech < 1 || s.end_silence < 1 || s.post_roll < 0 || s.post_roll > s.end_silence || s.max_frames < 1) return SS_ERR_ARG;
    if (!(s.p_abs >= 0.0f) || !(s.p_min >= 0.0f) || !(s.snr > 0.0f) || !(s.rise > 0.0f)) return SS_ERR_ARG;
    if (s.n_frames < 0 || s.n_hist < 0 || s.first_frame < 0 || s.hist_first < 0) return SS_ERR_ARG;
    if (s.first_frame + s.n_frames > (1LL << 40)) return SS_ERR_ARG;
    if (s.n_frames > 0) {
      if (s.first_frame * s.H < s.hist_first) return SS_ERR_ARG;
      if ((s.first_frame + s.n_frames - 1) * s.H + s.W - s.hist_first > s.n_hist) return SS_ERR_ARG;
      if (!s.hist) return SS_ERR_ARG;
    }
  }
  return SS_OK;
}

// The device copy of a call's segment table: one grow-only buffer per (device, stream), as pcm.hip keeps its own.
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
      SS_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));             // an earlier call of this stream may still read it
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

}  // namespace

extern "C" int ss_vad_scan(void* stream, const ss_vad_seg* h_segs, int n_segs, ss_vad_result* d_results) {
  if (n_segs < 0) return SS_ERR_ARG;
  if (n_segs == 0) return SS_OK;
  const int rc = scan_check(h_segs, n_segs, d_results);
  if (rc != SS_OK) return rc;
  std::vector<SegDev> tab((size_t)n_segs);
  for (int i = 0; i < n_segs; ++i) {
    tab[i].sg = h_segs[i];
    tab[i].inv_w = 1.0f / (float)h_segs[i].W;
    tab[i].pad = 0;
  }
  hipStream_t st = (hipStream_t)stream;
  void* d_tab = nullptr;
  const size_t bytes = sizeof(SegDev) * (size_t)n_segs;
  const int rt = table_for(stream, bytes, &d_tab);
  if (rt != SS_OK) return rt;
  SS_HIP_CHECK(hipMemcpyAsync(d_tab, tab.data(), bytes, hipMemcpyHostToDevice, st));   // pageable source: staged when the call returns
  hipLaunchKernelGGL(vad_scan_kernel, dim3((unsigned)n_segs), dim3(kThreads), 0, st, (const SegDev*)d_tab, d_results);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

extern "C" int ss_vad_scan_host(const ss_vad_seg* h_segs, int n_segs, ss_vad_result* h_results) {
  if (n_segs < 0) return SS_ERR_ARG;
  if (n_segs == 0) return SS_OK;
  const int rc = scan_check(h_segs, n_segs, h_results);
  if (rc != SS_OK) return rc;
  for (int i = 0; i < n_segs; ++i) {
    const ss_vad_seg& sg = h_segs[i];
    const float inv_w = 1.0f / (float)sg.W;
    ss_vad_state st = *sg.state;
    ss_vad_result r;
    result_init(r, sg, st);
    for (int k = 0; k < sg.n_frames; ++k) {
      const int64_t j = sg.first_frame + k;
      const float P = frame_power_host(sg.hist + (j * sg.H - sg.hist_first), sg.W, inv_w);
      if (sg.powers) sg.powers[k] = P;
      if (step(st, r, sg, j, P)) break;
    }
    *sg.state = st;
    h_results[i] = r;
  }
  return SS_OK;
}
