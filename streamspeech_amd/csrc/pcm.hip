// Raw PCM in and out of the session pools (include/streamspeech_hip.h, "Binary PCM"): ss_pcm_scatter decodes every chunk a pool step
// received -- float32 / 16-bit / G.711 mu-law / A-law, mono or interleaved stereo, all lying in ONE staging buffer the step uploaded
// once -- into the sessions' float32 sample histories in one launch; ss_pcm_pack_s16 turns the synthesised speech of a step's writers
// into 16-bit PCM in one launch, for one download.  Both kernels are memory-bound copies with a conversion: no LDS, no atomics, 16-byte
// loads and stores where the addresses allow them, scalar heads and tails.  The conversions are the inline functions of pcm.hpp, the
// same ones the host entry points (ss_pcm_decode_host, ss_pcm_pack_s16_host) call.
#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/streamspeech_hip.h"
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

// The device copy of a call's segment table: one grow-only buffer per (device, stream), so calls on one stream reuse it in stream
// order and calls on different streams never share one.  Buffers live until the process ends.
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
