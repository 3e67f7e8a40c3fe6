// Raw PCM in and out of the session pools (include/streamspeech_hip.h, "Binary PCM"): ss_pcm_scatter decodes every chunk a pool step
// received -- float32 / 16-bit / G.711 mu-law / A-law, mono or interleaved stereo, all lying in ONE staging buffer the step uploaded
// once -- into the sessions' float32 sample histories in one launch; ss_pcm_pack_s16 turns the synthesised speech of a step's writers
// into 16-bit PCM in one launch, for one download.  Both kernels are memory-bound copies with a conversion: no LDS, no atomics, 16-byte
// loads and stores where the addresses allow them, scalar heads and tails.  The conversions are the inline functions of pcm.hpp, the
// same ones the host entry points (ss_pcm_decode_host, ss_pcm_pack_s16_host) call.
// ss_pcm_emit is the way out at the caller's own rate and format: the streaming output resampler (resample_sample of fbank.hpp over a
// history that lies in the session's carry buffer and the step's new tail) and the encoders, for all such sessions of a step at once.
#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/streamspeech_hip.h"
#include "fbank.hpp"
#include "pcm.hpp"

namespace {

using namespace ss::pcm;

constexpr int kThreads = 256;
constexpr int kGroup = 8;                        // sample frames per lane: 8-16 source bytes per load, two 16-byte stores
constexpr int kTile = kThreads * kGroup;         // frames per workgroup

static_assert(sizeof(ss_pcm_seg) == 32, "ss_pcm_seg is 32 bytes");
static_assert(SS_PCM_F32LE == F32LE && SS_PCM_S16LE == S16LE && SS_PCM_ULAW == ULAW && SS_PCM_ALAW == ALAW, "one enum");

// One segment as the kernel sees it.  Groups of 8 frames are cut on the DESTINATION's 16-byte grid: `shift` = float index of dst
// modulo 4, group g covers frames [8 g - shift, 8 g - shift + 8), so a whole group stores two aligned 16-byte words.
struct SegDev {
  const uint8_t* src;
  float* dst;                // first sample of the segment's range
  int32_t frames, fmt, channels;
  int32_t tile0;             // first workgroup of the segment (an exclusive prefix sum of the segments' tile counts)
};
static_assert(sizeof(SegDev) == 32, "SegDev is 32 bytes");

// Frame j (a constant after unrolling) of a group whose 8 * bytes-per-frame source bytes lie in the words w -> the float32 bits.
template <int FMT, int CH>
__device__ __forceinline__ uint32_t frame_bits(const uint32_t* w, int j) {
  if (FMT == F32LE) {
    if (CH == 1) return w[j];
    return float_to_bits(f32_pair_to_float(bits_to_float(w[2 * j]), bits_to_float(w[2 * j + 1])));
  }
  int l, r = 0;
  if (FMT == S16LE) {
    if (CH == 1) {
      l = (int16_t)(uint16_t)(w[j >> 1] >> (16 * (j & 1)));
    } else {
      l = (int16_t)(uint16_t)(w[j] & 0xFFFFu);
      r = (int16_t)(uint16_t)(w[j] >> 16);
    }
  } else {
    const int k = CH * j;                        // byte index of the frame
    const uint8_t a = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
    const uint8_t b = (uint8_t)(w[(k + CH - 1) >> 2] >> (8 * ((k + CH - 1) & 3)));
    l = FMT == ULAW ? ulaw_to_s16(a) : alaw_to_s16(a);
    if (CH == 2) r = FMT == ULAW ? ulaw_to_s16(b) : alaw_to_s16(b);
  }
  return float_to_bits(CH == 1 ? s16_to_float(l) : s16_pair_to_float(l, r));
}

template <int FMT, int CH>
__device__ __forceinline__ void scatter_group(const SegDev& sg, int g, int shift) {
  constexpr int kBpf = (FMT == F32LE ? 4 : FMT == S16LE ? 2 : 1) * CH;      // bytes per frame
  constexpr int kBytes = kGroup * kBpf;                                     // 8 (G.711 mono), else a multiple of 16
  constexpr int kVec = kBytes >= 16 ? 16 : 8;
  const int f0 = g * kGroup - shift;                                        // first frame of the group; < 0 only in group 0
  if (f0 >= sg.frames) return;
  const uint8_t* p = sg.src + (int64_t)f0 * kBpf;
  const bool whole = f0 >= 0 && f0 + kGroup <= sg.frames;
  // sg.src is 16-byte aligned and 8 g kBpf a multiple of kVec: whether the group's bytes are aligned is the segment's property
  // (shift * kBpf), the same for every lane of the workgroup
  if (whole) {
    uint32_t w[kBytes / 4];
    if ((((uintptr_t)p) & (kVec - 1)) == 0) {
      if (kVec == 16) {
#pragma unroll
        for (int i = 0; i < kBytes / 16; ++i) {
          const uint4 v = reinterpret_cast<const uint4*>(p)[i];
          w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
        }
      } else {
        const uint2 v = *reinterpret_cast<const uint2*>(p);
        w[0] = v.x; w[1] = v.y;
      }
    } else if (FMT == F32LE) {                   // off the vector grid (the destination offset is not a multiple of 4 samples):
#pragma unroll
      for (int i = 0; i < kBytes / 4; ++i) w[i] = reinterpret_cast<const uint32_t*>(p)[i];   // sample by sample, naturally aligned
    } else if (FMT == S16LE) {
      const uint16_t* h = reinterpret_cast<const uint16_t*>(p);
#pragma unroll
      for (int i = 0; i < kBytes / 4; ++i) w[i] = (uint32_t)h[2 * i] | ((uint32_t)h[2 * i + 1] << 16);
    } else {
#pragma unroll
      for (int i = 0; i < kBytes / 4; ++i)
        w[i] = (uint32_t)p[4 * i] | ((uint32_t)p[4 * i + 1] << 8) | ((uint32_t)p[4 * i + 2] << 16) | ((uint32_t)p[4 * i + 3] << 24);
    }
    uint4 o0, o1;
    o0.x = frame_bits<FMT, CH>(w, 0); o0.y = frame_bits<FMT, CH>(w, 1); o0.z = frame_bits<FMT, CH>(w, 2); o0.w = frame_bits<FMT, CH>(w, 3);
    o1.x = frame_bits<FMT, CH>(w, 4); o1.y = frame_bits<FMT, CH>(w, 5); o1.z = frame_bits<FMT, CH>(w, 6); o1.w = frame_bits<FMT, CH>(w, 7);
    uint4* d = reinterpret_cast<uint4*>(sg.dst + f0);                       // 16-byte aligned by the choice of shift
    d[0] = o0;
    d[1] = o1;
    return;
  }
  // head or tail of the segment: only frames [0, frames) are read and written
  uint32_t* d = reinterpret_cast<uint32_t*>(sg.dst);
  for (int j = 0; j < kGroup; ++j) {
    const int f = f0 + j;
    if (f >= 0 && f < sg.frames) d[f] = decode_frame_bits(sg.src + (int64_t)f * kBpf, FMT, CH);
  }
}

__global__ __launch_bounds__(kThreads) void pcm_scatter_kernel(const SegDev* __restrict__ segs, int n_segs) {
  // the segment of this workgroup: the last one whose first tile is <= blockIdx.x (empty segments share a successor's tile0)
  int lo = 0, hi = n_segs;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (segs[mid].tile0 <= (int)blockIdx.x) lo = mid; else hi = mid;
  }
  const SegDev sg = segs[lo];
  const int shift = (int)((((uintptr_t)sg.dst) >> 2) & 3);
  const int g = ((int)blockIdx.x - sg.tile0) * kThreads + (int)threadIdx.x;
  switch (sg.fmt * 2 + sg.channels - 1) {
    case F32LE * 2: scatter_group<F32LE, 1>(sg, g, shift); break;
    case F32LE * 2 + 1: scatter_group<F32LE, 2>(sg, g, shift); break;
    case S16LE * 2: scatter_group<S16LE, 1>(sg, g, shift); break;
    case S16LE * 2 + 1: scatter_group<S16LE, 2>(sg, g, shift); break;
    case ULAW * 2: scatter_group<ULAW, 1>(sg, g, shift); break;
    case ULAW * 2 + 1: scatter_group<ULAW, 2>(sg, g, shift); break;
    case ALAW * 2: scatter_group<ALAW, 1>(sg, g, shift); break;
    default: scatter_group<ALAW, 2>(sg, g, shift); break;
  }
}

// 8 floats per lane -> 8 int16: two 16-byte loads, one 16-byte store when both pointers are 16-byte aligned; the tail (and everything,
// when they are not) goes sample by sample.
__global__ __launch_bounds__(kThreads) void pcm_pack_s16_kernel(const float* __restrict__ src, int64_t n, int16_t* __restrict__ out,
                                                                int aligned) {
  const int64_t i0 = ((int64_t)blockIdx.x * kThreads + threadIdx.x) * kGroup;
  if (i0 >= n) return;
  if (aligned && i0 + kGroup <= n) {
    const float4 a = reinterpret_cast<const float4*>(src + i0)[0];
    const float4 b = reinterpret_cast<const float4*>(src + i0)[1];
    uint4 o;
    o.x = (uint32_t)(uint16_t)pack_s16(a.x) | ((uint32_t)(uint16_t)pack_s16(a.y) << 16);
    o.y = (uint32_t)(uint16_t)pack_s16(a.z) | ((uint32_t)(uint16_t)pack_s16(a.w) << 16);
    o.z = (uint32_t)(uint16_t)pack_s16(b.x) | ((uint32_t)(uint16_t)pack_s16(b.y) << 16);
    o.w = (uint32_t)(uint16_t)pack_s16(b.z) | ((uint32_t)(uint16_t)pack_s16(b.w) << 16);
    *reinterpret_cast<uint4*>(out + i0) = o;
    return;
  }
  const int64_t i1 = std::min<int64_t>(i0 + kGroup, n);
  for (int64_t i = i0; i < i1; ++i) out[i] = pack_s16(src[i]);
}

// ---- speech out at the caller's rate and format ------------------------------------------------------------------------------------
// One segment of ss_pcm_emit as the kernels see it.  A workgroup owns `tile` consecutive outputs of one segment (a multiple of
// kTile; a lane takes groups of 8, so a whole group stores 32 / 16 / 8 aligned bytes); tile0 is the exclusive prefix sum of the
// segments' tile counts, searched as pcm_scatter_kernel searches its own.
struct EmitDev {
  float* carry;
  const float* tail;
  const float* taps;
  uint8_t* out;              // first byte of the segment's range, 16-byte aligned
  long long n_before, n_after, k0;
  long long base;            // index in y of carry[0] on entry: n_before - carry_len
  int32_t n_out, up, down, half, fmt;
  int32_t tile, tile0;
  int32_t keep;              // samples of y the carry holds after the call: min((2 half) / up, n_after)
};
static_assert(sizeof(EmitDev) == 96, "EmitDev is 96 bytes");
static_assert(sizeof(ss_pcm_emit_seg) == 88, "ss_pcm_emit_seg is 88 bytes");

constexpr int kMaxTaps = 64 * 1024 / (int)sizeof(float);   // ss_resample's own limit: the taps go through LDS
constexpr int kMaxTileMul = 8;

// Outputs per workgroup for a table of ntaps taps: staging the table costs ntaps loads, so a workgroup that stages more writes more
// (441:160 -- 8821 taps, 35 KB -- gets 10240 outputs where 3:1 -- 61 taps -- gets 2048).
inline int emit_tile(int ntaps) { return kTile * std::min(kMaxTileMul, std::max(1, (ntaps + kTile - 1) / kTile)); }

__host__ __device__ inline float emit_value(const float* carry, const float* tail, long long base, long long n_before,
                                            long long n_after, int up, int down, const float* hs, int half, long long k) {
  if (up == down) return tail[k - n_before];           // K(N) = N: sample k of z is sample k of y, and it arrived with this call
  return ss::resample_sample(SplitHistory{carry, tail, base, n_before}, n_after, up, down, hs, half, k);
}

__host__ __device__ inline void store_sample(uint8_t* out, long long j, uint32_t bits, int fmt) {
  if (fmt == F32LE) reinterpret_cast<uint32_t*>(out)[j] = bits;             // out is 16-byte aligned
  else if (fmt == S16LE) reinterpret_cast<uint16_t*>(out)[j] = (uint16_t)bits;
  else out[j] = (uint8_t)bits;
}

__global__ __launch_bounds__(kThreads) void pcm_emit_kernel(const EmitDev* __restrict__ segs, int n_segs) {
  extern __shared__ float hs[];
  int lo = 0, hi = n_segs;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (segs[mid].tile0 <= (int)blockIdx.x) lo = mid; else hi = mid;
  }
  const EmitDev sg = segs[lo];
  if (sg.up != sg.down) {                              // the whole workgroup takes the same side
    const int ntaps = 2 * sg.half + 1;
    for (int i = threadIdx.x; i < ntaps; i += kThreads) hs[i] = sg.taps[i];
    __syncthreads();
  }
  const int j_begin = ((int)blockIdx.x - sg.tile0) * sg.tile;
  const int j_end = min(sg.n_out, j_begin + sg.tile);  // n_out <= 2^30 - 1: the sums stay inside the int range
  for (int j0 = j_begin + (int)threadIdx.x * kGroup; j0 < j_end; j0 += kTile) {
    if (j0 + kGroup <= j_end) {
      uint32_t b[kGroup];
#pragma unroll
      for (int i = 0; i < kGroup; ++i)
        b[i] = encode_sample(emit_value(sg.carry, sg.tail, sg.base, sg.n_before, sg.n_after, sg.up, sg.down, hs, sg.half,
                                        sg.k0 + j0 + i), sg.fmt);
      if (sg.fmt == F32LE) {
        uint4* d = reinterpret_cast<uint4*>(sg.out + (size_t)j0 * 4);
        d[0] = make_uint4(b[0], b[1], b[2], b[3]);
        d[1] = make_uint4(b[4], b[5], b[6], b[7]);
      } else if (sg.fmt == S16LE) {
        *reinterpret_cast<uint4*>(sg.out + (size_t)j0 * 2) =
            make_uint4(b[0] | (b[1] << 16), b[2] | (b[3] << 16), b[4] | (b[5] << 16), b[6] | (b[7] << 16));
      } else {
        *reinterpret_cast<uint2*>(sg.out + (size_t)j0) = make_uint2(b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24),
                                                                    b[4] | (b[5] << 8) | (b[6] << 16) | (b[7] << 24));
      }
    } else {                                           // the segment's tail: sample by sample
      for (int j = j0; j < j_end; ++j)
        store_sample(sg.out, j, encode_sample(emit_value(sg.carry, sg.tail, sg.base, sg.n_before, sg.n_after, sg.up, sg.down, hs,
                                                         sg.half, sg.k0 + j), sg.fmt), sg.fmt);
    }
  }
}

// The carry buffers after the emit grid has read them: workgroup = one segment.  The new carry (the last `keep` samples of y) may
// take samples from the old one at other positions, so it goes through LDS: all reads, a barrier, all writes.
__global__ __launch_bounds__(kThreads) void pcm_emit_carry_kernel(const EmitDev* __restrict__ segs) {
  extern __shared__ float cs[];
  const EmitDev sg = segs[blockIdx.x];
  if (sg.keep == 0 || sg.n_after == sg.n_before) return;                   // nothing kept, or nothing new: the carry stays
  const SplitHistory y{sg.carry, sg.tail, sg.base, sg.n_before};
  const long long first = sg.n_after - sg.keep;                            // >= base
  for (int i = threadIdx.x; i < sg.keep; i += kThreads) cs[i] = y[first + i];
  __syncthreads();
  for (int i = threadIdx.x; i < sg.keep; i += kThreads) sg.carry[i] = cs[i];
}

// Every refusal of ss_pcm_emit / ss_pcm_emit_host, in the header's order.
int emit_check(const ss_pcm_emit_seg* h_segs, int n_segs, const void* out, int64_t out_bytes) {
  if (n_segs < 0 || (n_segs > 0 && !h_segs)) return SS_ERR_ARG;
  for (int i = 0; i < n_segs; ++i) {
    const ss_pcm_emit_seg& s = h_segs[i];
    if (s.fmt < 0 || s.fmt >= N_FMT) return SS_ERR_ARG;
    if (s.up < 1 || s.down < 1) return SS_ERR_ARG;
    if (s.up != s.down && (s.half < 1 || 2LL * s.half + 1 > kMaxTaps)) return SS_ERR_ARG;
    if (s.n_before < 0 || s.n_new < 0 || s.n_before + s.n_new > 0x7fffffffLL) return SS_ERR_ARG;
    const long long hist = emit_history(s.up, s.down, s.half);
    if (s.carry_len != std::min<long long>(hist, s.n_before)) return SS_ERR_ARG;
    const long long n_after = s.n_before + s.n_new;
    if (s.k0 < emit_count(s.n_before, s.up, s.down, s.half, 0) || s.k1 < s.k0) return SS_ERR_ARG;
    if (s.k1 > emit_count(n_after, s.up, s.down, s.half, s.finished != 0) || s.k1 - s.k0 > 0x3fffffffLL) return SS_ERR_ARG;
    if (s.out_offset < 0 || (s.out_offset & 15) != 0) return SS_ERR_ARG;
    const bool work = s.k1 > s.k0;
    if (work && !out) return SS_ERR_ARG;
    if (s.n_new > 0 && !s.tail) return SS_ERR_ARG;
    if (work && s.up != s.down && !s.taps) return SS_ERR_ARG;
    if (!s.carry && (s.carry_len > 0 || std::min<long long>(hist, n_after) > 0)) return SS_ERR_ARG;
  }
  if (out_bytes < 0) return SS_ERR_ARG;
  for (int i = 0; i < n_segs; ++i) {
    const ss_pcm_emit_seg& s = h_segs[i];
    const int64_t bytes = (s.k1 - s.k0) * sample_bytes(s.fmt);
    if (s.out_offset > out_bytes || bytes > out_bytes - s.out_offset) return SS_ERR_CAPACITY;
  }
  return SS_OK;
}

// The device copy of a call's segment table: one grow-only buffer per (device, stream), so calls on one stream reuse it in stream
// order and calls on different streams never share one; ss_pcm_scatter's table is slot 0 of a stream, ss_pcm_emit's slot 1.  Buffers
// live until the process ends.
struct TableBuf { void* p = nullptr; size_t cap = 0; };
std::mutex g_mu;
std::map<std::pair<std::pair<int, void*>, int>, TableBuf> g_tables;

int table_for(void* stream, size_t bytes, void** out, int slot = 0) {
  int dev = 0;
  SS_HIP_CHECK(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_mu);
  TableBuf& t = g_tables[{{dev, stream}, slot}];
  if (t.cap < bytes) {
    if (t.p) {
      SS_HIP_CHECK(hipStreamSynchronize((hipStream_t)stream));             // an earlier call of this stream may still read it
      SS_HIP_CHECK(hipFree(t.p));
      t.p = nullptr; t.cap = 0;
    }
    const size_t cap = std::max<size_t>(4096, 2 * bytes);
    SS_HIP_CHECK(hipMalloc(&t.p, cap));
    t.cap = cap;
  }
  *out = t.p;
  return SS_OK;
}

}  // namespace

extern "C" int ss_pcm_scatter(void* stream, const void* d_stage, int64_t stage_bytes, const ss_pcm_seg* h_segs, int n_segs,
                              float* const* h_dst, const int64_t* h_dst_cap, int n_dst) {
  // every refusal before any HIP call, in the header's order: arguments of all segments first, then capacities
  if (n_segs < 0) return SS_ERR_ARG;
  if (n_segs == 0) return SS_OK;
  if (!h_segs) return SS_ERR_ARG;
  for (int i = 0; i < n_segs; ++i) {
    const ss_pcm_seg& s = h_segs[i];
    if (s.fmt < 0 || s.fmt >= N_FMT) return SS_ERR_ARG;
    if (s.channels != 1 && s.channels != 2) return SS_ERR_ARG;
    if (s.frames < 0) return SS_ERR_ARG;
    if (s.src_offset < 0 || (s.src_offset & 15) != 0) return SS_ERR_ARG;
    if (s.dst < 0 || s.dst >= n_dst) return SS_ERR_ARG;
    if (s.dst_offset < 0) return SS_ERR_ARG;
  }
  if (!h_dst || !h_dst_cap || stage_bytes < 0) return SS_ERR_ARG;
  int64_t tiles = 0;
  for (int i = 0; i < n_segs; ++i) {
    const ss_pcm_seg& s = h_segs[i];
    const int64_t bytes = (int64_t)s.frames * sample_bytes(s.fmt) * s.channels;
    if (s.src_offset > stage_bytes || bytes > stage_bytes - s.src_offset) return SS_ERR_CAPACITY;
    if (s.dst_offset > h_dst_cap[s.dst] || (int64_t)s.frames > h_dst_cap[s.dst] - s.dst_offset) return SS_ERR_CAPACITY;
  }
  std::vector<SegDev> tab((size_t)n_segs);
  for (int i = 0; i < n_segs; ++i) {
    const ss_pcm_seg& s = h_segs[i];
    if (s.frames > 0 && (!d_stage || !h_dst[s.dst])) return SS_ERR_ARG;
    SegDev& d = tab[i];
    d.src = (const uint8_t*)d_stage + s.src_offset;
    d.dst = h_dst[s.dst] ? h_dst[s.dst] + s.dst_offset : nullptr;
    d.frames = s.frames; d.fmt = s.fmt; d.channels = s.channels;
    d.tile0 = (int32_t)tiles;
    const int shift = (int)((((uintptr_t)d.dst) >> 2) & 3);
    if (s.frames > 0) tiles += ((int64_t)s.frames + shift + kTile - 1) / kTile;
    if (tiles > 0x7fffffff) return SS_ERR_ARG;
  }
  if (tiles == 0) return SS_OK;
  if ((((uintptr_t)d_stage) & 15) != 0) return SS_ERR_ARG;                  // the staging buffer itself: an allocation, 256-byte aligned
  hipStream_t st = (hipStream_t)stream;
  void* d_tab = nullptr;
  const size_t bytes = sizeof(SegDev) * (size_t)n_segs;
  const int rc = table_for(stream, bytes, &d_tab);
  if (rc != SS_OK) return rc;
  // pageable source: the runtime has staged it when the call returns, so `tab` may go out of scope
  SS_HIP_CHECK(hipMemcpyAsync(d_tab, tab.data(), bytes, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(pcm_scatter_kernel, dim3((unsigned)tiles), dim3(kThreads), 0, st, (const SegDev*)d_tab, n_segs);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

extern "C" int ss_pcm_pack_s16(void* stream, const float* d_src, int64_t n, int16_t* d_out) {
  if (n < 0) return SS_ERR_ARG;
  if (n == 0) return SS_OK;
  if (!d_src || !d_out) return SS_ERR_ARG;
  const int64_t blocks = (n + kTile - 1) / kTile;
  if (blocks > 0x7fffffff) return SS_ERR_ARG;
  const int aligned = ((((uintptr_t)d_src) | ((uintptr_t)d_out)) & 15) == 0;
  hipLaunchKernelGGL(pcm_pack_s16_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, (hipStream_t)stream, d_src, n, d_out, aligned);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

extern "C" int ss_pcm_decode_host(const void* h_src, int fmt, int channels, int64_t frames, float* h_dst) {
  if (fmt < 0 || fmt >= N_FMT || (channels != 1 && channels != 2) || frames < 0) return SS_ERR_ARG;
  if (frames == 0) return SS_OK;
  if (!h_src || !h_dst) return SS_ERR_ARG;
  const uint8_t* p = (const uint8_t*)h_src;
  const int bpf = sample_bytes(fmt) * channels;
  for (int64_t f = 0; f < frames; ++f) {
    const uint32_t b = decode_frame_bits(p + f * bpf, fmt, channels);
    memcpy(h_dst + f, &b, 4);
  }
  return SS_OK;
}

extern "C" int ss_pcm_pack_s16_host(const float* h_src, int64_t n, int16_t* h_out) {
  if (n < 0) return SS_ERR_ARG;
  if (n == 0) return SS_OK;
  if (!h_src || !h_out) return SS_ERR_ARG;
  for (int64_t i = 0; i < n; ++i) h_out[i] = pack_s16(h_src[i]);
  return SS_OK;
}

extern "C" int64_t ss_pcm_emit_count(int64_t n, int up, int down, int half, int finished) {
  if (n < 0 || up < 1 || down < 1 || half < 0) return -1;
  return emit_count(n, up, down, half, finished != 0);
}

extern "C" int ss_pcm_emit(void* stream, const ss_pcm_emit_seg* h_segs, int n_segs, void* d_out, int64_t out_bytes) {
  const int rc = emit_check(h_segs, n_segs, d_out, out_bytes);
  if (rc != SS_OK) return rc;
  if (n_segs == 0) return SS_OK;
  if ((((uintptr_t)d_out) & 15) != 0) return SS_ERR_ARG;                   // the output buffer itself: an allocation
  std::vector<EmitDev> tab((size_t)n_segs);
  int64_t tiles = 0;
  int max_taps = 0, max_keep = 0;
  for (int i = 0; i < n_segs; ++i) {
    const ss_pcm_emit_seg& s = h_segs[i];
    EmitDev& d = tab[i];
    d.carry = s.carry; d.tail = s.tail; d.taps = s.taps;
    d.out = (uint8_t*)d_out + s.out_offset;
    d.n_before = s.n_before; d.n_after = s.n_before + s.n_new; d.k0 = s.k0;
    d.base = s.n_before - s.carry_len;
    d.n_out = (int32_t)(s.k1 - s.k0); d.up = s.up; d.down = s.down; d.half = s.half; d.fmt = s.fmt;
    const int ntaps = s.up == s.down ? 0 : 2 * s.half + 1;
    d.tile = emit_tile(ntaps);
    d.tile0 = (int32_t)tiles;
    d.keep = (int32_t)std::min<long long>(emit_history(s.up, s.down, s.half), d.n_after);
    if (d.n_out > 0) {
      tiles += ((int64_t)d.n_out + d.tile - 1) / d.tile;
      max_taps = std::max(max_taps, ntaps);
    }
    if (s.n_new > 0) max_keep = std::max(max_keep, d.keep);
    if (tiles > 0x7fffffff) return SS_ERR_ARG;
  }
  if (tiles == 0 && max_keep == 0) return SS_OK;
  hipStream_t st = (hipStream_t)stream;
  void* d_tab = nullptr;
  const size_t bytes = sizeof(EmitDev) * (size_t)n_segs;
  const int rt = table_for(stream, bytes, &d_tab, 1);
  if (rt != SS_OK) return rt;
  SS_HIP_CHECK(hipMemcpyAsync(d_tab, tab.data(), bytes, hipMemcpyHostToDevice, st));   // pageable source: staged when the call returns
  if (tiles > 0) {
    hipLaunchKernelGGL(pcm_emit_kernel, dim3((unsigned)tiles), dim3(kThreads), (size_t)max_taps * sizeof(float), st,
                       (const EmitDev*)d_tab, n_segs);
    SS_LAUNCH_CHECK();
  }
  if (max_keep > 0) {
    hipLaunchKernelGGL(pcm_emit_carry_kernel, dim3((unsigned)n_segs), dim3(kThreads), (size_t)max_keep * sizeof(float), st,
                       (const EmitDev*)d_tab);
    SS_LAUNCH_CHECK();
  }
  return SS_OK;
}

extern "C" int ss_pcm_emit_host(const ss_pcm_emit_seg* h_segs, int n_segs, void* h_out, int64_t out_bytes) {
  const int rc = emit_check(h_segs, n_segs, h_out, out_bytes);
  if (rc != SS_OK) return rc;
  if (n_segs > 0 && (((uintptr_t)h_out) & 3) != 0) return SS_ERR_ARG;      // f32le / s16le samples are stored as words
  std::vector<float> kept;
  for (int i = 0; i < n_segs; ++i) {
    const ss_pcm_emit_seg& s = h_segs[i];
    const long long n_after = s.n_before + s.n_new, base = s.n_before - s.carry_len;
    uint8_t* out = (uint8_t*)h_out + s.out_offset;
    for (long long k = s.k0; k < s.k1; ++k)
      store_sample(out, k - s.k0, encode_sample(emit_value(s.carry, s.tail, base, s.n_before, n_after, s.up, s.down, s.taps, s.half,
                                                           k), s.fmt), s.fmt);
    const long long keep = std::min<long long>(emit_history(s.up, s.down, s.half), n_after);
    if (keep == 0 || s.n_new == 0) continue;
    const SplitHistory y{s.carry, s.tail, base, s.n_before};
    kept.resize((size_t)keep);
    for (long long j = 0; j < keep; ++j) kept[(size_t)j] = y[n_after - keep + j];
    memcpy(s.carry, kept.data(), sizeof(float) * (size_t)keep);
  }
  return SS_OK;
}

extern "C" int ss_pcm_encode_host(const float* h_src, int64_t n, int fmt, void* h_out) {
  if (n < 0 || fmt < 0 || fmt >= N_FMT) return SS_ERR_ARG;
  if (n == 0) return SS_OK;
  if (!h_src || !h_out) return SS_ERR_ARG;
  uint8_t* o = (uint8_t*)h_out;
  const int sb = sample_bytes(fmt);
  for (int64_t i = 0; i < n; ++i) {
    const uint32_t b = encode_sample(h_src[i], fmt);
    memcpy(o + i * sb, &b, (size_t)sb);                                    // little-endian host, as everywhere in this file
  }
  return SS_OK;
}
