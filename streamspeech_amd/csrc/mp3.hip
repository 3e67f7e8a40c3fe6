// MP3 ingest, device stage: the numeric part of Layer III decoding over a ragged batch of files (records and q[576] from
// mp3_host.hip), two kernels per batch, no host round trip between them.
//
//  (a) mp3_imdct_kernel, one workgroup per granule (both channels, which MS stereo couples): requantisation
//      sign(q) |q|^(4/3) 2^(e/4) with e an integer (global gain, subblock gain, scalefactors, pretab), short-block reorder into
//      index 3 f + window, MS stereo, alias reduction (long subbands only), IMDCT (one 36-point or three 12-point transforms as
//      the defining cosine sums over LDS tables) and the block-type window.  Writes the 36 windowed samples of every subband.
//  (b) mp3_synth_kernel, one workgroup per granule (channels in turn; with `mono` their mean is written): overlap-add with the
//      previous granule's block, frequency inversion, matrixing V[t][i] = sum_k N[i][k] S[t][k] of the granule's 18 time slots
//      and the 15 before them as a [48 x 32] x [32 x 64] product on FP32 MFMA (v_mfma_f32_16x16x4f32: exact FP32 products, the
//      same rounding class as the FMA loop it replaces, and the 2 x 64 x 32 flops of each slot become 8 matrix instructions per
//      16 x 16 tile instead of a DCT factorisation whose error the float64 restatement would have to bound), then the 16-tap
//      windowed sum with D[512].  The slots before the granule are recomputed from (a)'s output instead of carried, so no
//      granule waits for another: nothing is serial across granules, and a file decodes to the same bits alone or in a batch.
// A file's first granule sees zero overlap and zero V history.
//
// Streams (ss_mp3_stream_synthesize): the same kernel (a) for the new granules of every stream of a step, then a twin of (b) whose
// granules g-1 and g-2 may lie in the stream's carried state -- the blocks of its last two granules, which is everything a granule
// reads besides its own block: g-1 for the overlap-add and the 15 slots in front, g-2 for the overlap-add of those slots -- and a
// third launch that moves the carried blocks on.  Both (b) kernels are one device function over two block sources, so a sample
// goes through the same operations in the same order and a stream decodes to the bits of the whole file in any chunking.
#include <math.h>
#include <string.h>

#include <vector>

#include "../../include/streamspeech_hip.h"
#include "common.hpp"
#define MP3T_DEVICE
#include "mp3_tables.hpp"

namespace {

constexpr int kThreads = 256;

struct FileDev { int64_t rec_offset, out_offset; int32_t granules, channels, skip, n_out; };
static_assert(sizeof(FileDev) == sizeof(ss_mp3_file), "file table layout");
static_assert(sizeof(ss_mp3_granule) == 80, "record layout");

__device__ inline int find_file(const int64_t* gpre, int n_files, int64_t g) {
  int lo = 0, hi = n_files;                          // gpre[lo] <= g < gpre[hi]
  while (hi - lo > 1) {
    int mid = (lo + hi) >> 1;
    if (gpre[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

__device__ inline float pow2_quarter(int e4) {       // 2^(e4 / 4), exact up to the rounding of 2^(k/4)
  const float frac[4] = {1.0f, 1.18920711500272106672f, 1.41421356237309504880f, 1.68179283050742908606f};
  return ldexpf(frac[e4 & 3], e4 >> 2);
}

__global__ void __launch_bounds__(kThreads) mp3_imdct_kernel(const int16_t* __restrict__ q, const ss_mp3_granule* __restrict__ rec,
                                                              const FileDev* __restrict__ files, const int64_t* __restrict__ gpre,
                                                              int n_files, float* __restrict__ blk) {
  __shared__ float xr[2][576];
  __shared__ float c144[144];                        // cos(pi n / 72), copied from constant memory (mp3_tables.hpp)
  __shared__ float win[4][36];                       // block-type windows (type 2: the 12-point window in [0, 12))
  const int tid = threadIdx.x;
  const int64_t g = blockIdx.x;
  const int f = find_file(gpre, n_files, g);
  const FileDev fd = files[f];
  const int nch = fd.channels;
  const int64_t r0 = fd.rec_offset + (g - gpre[f]) * nch;

  for (int n = tid; n < 144; n += kThreads) c144[n] = mp3t::kCos144[n];
  for (int n = tid; n < 4 * 36; n += kThreads) win[n / 36][n % 36] = mp3t::kImdctWin[n / 36][n % 36];

  // -- requantisation, written in reordered position (short lines: 3 f + window)
  for (int c = 0; c < nch; ++c) {
    const ss_mp3_granule& R = rec[r0 + c];
    const int sr = R.sr_index < 9 ? R.sr_index : 8;
    const int bt = R.block_type & 3, nz = R.nz < 576 ? (R.nz > 0 ? R.nz : 0) : 576;
    const int gg = R.global_gain - 210, mult = R.scalefac_scale ? 4 : 2;
    const int long_end = bt != 2 ? 576 : (R.mixed ? 36 : 0);
    const int16_t* qq = q + (r0 + c) * 576;
    for (int l = tid; l < 576; l += kThreads) {
      const int v = l < nz ? qq[l] : 0;
      int dst = l, e4;
      if (l < long_end) {
        int b = 0;
        while (b < 21 && mp3t::kSfbLong[sr][b + 1] <= l) ++b;
        e4 = gg - mult * (R.sf_l[b] + (R.preflag ? mp3t::kPretab[b] : 0));
      } else {
        int b = 0;
        while (b < 12 && 3 * mp3t::kSfbShort[sr][b + 1] <= l) ++b;
        const int start = mp3t::kSfbShort[sr][b], width = mp3t::kSfbShort[sr][b + 1] - start;
        const int off = l - 3 * start, w = off / width, i = off - w * width;
        dst = 3 * (start + i) + w;
        e4 = gg - 8 * R.subblock_gain[w] - mult * R.sf_s[b][w];
      }
      const float a = (float)(v < 0 ? -v : v);
      const float m = a * cbrtf(a) * pow2_quarter(e4);
      xr[c][dst] = v < 0 ? -m : m;
    }
  }
  __syncthreads();
  // -- MS stereo
  if (nch == 2 && rec[r0].ms) {
    const float s = 0.70710678118654752440f;
    for (int l = tid; l < 576; l += kThreads) {
      const float m = xr[0][l], d = xr[1][l];
      xr[0][l] = (m + d) * s;
      xr[1][l] = (m - d) * s;
    }
    __syncthreads();
  }
  // -- alias reduction: butterflies across the 31 subband boundaries (mixed blocks: the first only; short blocks: none)
  for (int c = 0; c < nch; ++c) {
    const ss_mp3_granule& R = rec[r0 + c];
    const int bt = R.block_type & 3;
    const int nb = bt != 2 ? 31 : (R.mixed ? 1 : 0);
    if (tid < nb * 8) {
      const int sb = tid / 8 + 1, i = tid % 8;
      const float cs = mp3t::kAliasCs[i], ca = mp3t::kAliasCa[i];
      const float bu = xr[c][18 * sb - 1 - i], bd = xr[c][18 * sb + i];
      xr[c][18 * sb - 1 - i] = bu * cs - bd * ca;
      xr[c][18 * sb + i] = bd * cs + bu * ca;
    }
  }
  __syncthreads();
  // -- IMDCT + window: thread per (subband, output sample)
  for (int c = 0; c < nch; ++c) {
    const ss_mp3_granule& R = rec[r0 + c];
    const int bt = R.block_type & 3;
    float* out = blk + (r0 + c) * 1152;
    for (int n = tid; n < 1152; n += kThreads) {
      const int sb = n / 36, i = n % 36;
      const float* X = &xr[c][18 * sb];
      float y = 0.0f;
      if (bt != 2 || (R.mixed && sb < 2)) {
        const int bte = bt == 2 ? 0 : bt;
        for (int k = 0; k < 18; ++k) y = fmaf(X[k], c144[((2 * i + 19) * (2 * k + 1)) % 144], y);
        y *= win[bte][i];
      } else {
        for (int w = 0; w < 3; ++w) {
          const int j = i - 6 - 6 * w;
          if (j < 0 || j >= 12) continue;
          float s = 0.0f;
          for (int k = 0; k < 6; ++k) s = fmaf(X[3 * k + w], c144[(3 * (2 * j + 7) * (2 * k + 1)) % 144], s);
          y = fmaf(s, win[2][j], y);
        }
      }
      out[n] = y;
    }
  }
}

typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int kSlots = 33;                           // 15 slots of the previous granule + 18 of this one
constexpr int kYld = 33;                             // LDS row stride of the subband samples (bank-conflict padding)

// Where a granule's IMDCT blocks come from.  back = 0: the granule itself, 1 / 2: the granules before it.
struct FileBlocks {                                  // a whole file: every granule's block is in blk; the file starts from nothing
  const float* blk;
  int64_t rec_offset, gi;
  int nch;
  __device__ bool has(int back) const { return gi - back >= 0; }
  __device__ const float* row(int back, int c) const { return blk + (rec_offset + (gi - back) * nch + c) * 1152; }
};

struct StreamBlocks {                                // a stream: the new granules in blk, the two before them in the carried state
  const float* blk;
  const float* state;                                // [2][nch][1152], older first
  int64_t rec_offset, gi;                            // gi: index among the new granules
  int nch, history;                                  // history: granules decoded before the new ones, saturated at 2
  __device__ bool has(int back) const { return gi - back >= -(int64_t)history; }
  __device__ const float* row(int back, int c) const {
    const int64_t h = gi - back;
    return h >= 0 ? blk + (rec_offset + h * nch + c) * 1152 : state + ((2 + h) * nch + c) * 1152;
  }
};

// One granule's synthesis, the body of both synthesis kernels: sample n of the granule goes to out[c * ch_stride + o0 + n] when
// 0 <= o0 + n < n_out (with mono: the channel mean, to out[o0 + n]).  The arithmetic of a sample depends on the blocks alone.
template <class Blocks>
__device__ __forceinline__ void mp3_synth_granule(const Blocks& src, int nch, int mono, float* __restrict__ out, int64_t ch_stride,
                                                  int64_t o0, int64_t n_out) {
  __shared__ float Y[48 * kYld];                     // subband samples [slot][subband], rows >= 33 zero
  __shared__ float B[32 * 64];                       // N^T: B[k][i] = cos((16 + i)(2k + 1) pi / 64)
  __shared__ float V[kSlots * 64];
  __shared__ float D[512];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

  for (int n = tid; n < 32 * 64; n += kThreads) {
    const int k = n / 64, i = n % 64;
    B[n] = mp3t::kCos128[((16 + i) * (2 * k + 1)) % 128];
  }
  for (int n = tid; n < 512; n += kThreads) {
    const int base = n <= 256 ? mp3t::kWinBase[n] : mp3t::kWinBase[512 - n];
    D[n] = (float)base * (1.0f / 65536.0f) * (((n >> 6) & 1) ? -1.0f : 1.0f);
  }
  for (int n = tid; n < (48 - kSlots) * kYld; n += kThreads) Y[kSlots * kYld + n] = 0.0f;

  float acc[3] = {0.0f, 0.0f, 0.0f};                 // this thread's outputs n = tid + 256 e of the granule (576 = 2.25 x 256)
  for (int c = 0; c < nch; ++c) {
    __syncthreads();                                 // Y / V of the previous channel are consumed
    // -- overlap-add + frequency inversion of slots -15..17
    for (int n = tid; n < kSlots * 32; n += kThreads) {
      const int t = n / 32, sb = n % 32;
      const int back = t < 15 ? 1 : 0;               // granule the slot belongs to: the previous one, or this
      const int s = t < 15 ? t + 3 : t - 15;         // slot within it
      float y = 0.0f;
      if (src.has(back)) {
        y = src.row(back, c)[sb * 36 + s];
        if (src.has(back + 1)) y += src.row(back + 1, c)[sb * 36 + 18 + s];
        if ((sb & 1) && (s & 1)) y = -y;
      }
      Y[t * kYld + sb] = y;
    }
    __syncthreads();
    // -- matrixing on MFMA: wave w owns output columns [16 w, 16 w + 16), all three 16-slot row tiles
    {
      v4f d[3];
      for (int rt = 0; rt < 3; ++rt) d[rt] = v4f{0.0f, 0.0f, 0.0f, 0.0f};
      const int r = lane & 15, kq = lane >> 4;
#pragma unroll
      for (int s = 0; s < 8; ++s) {
        const float b = B[(4 * s + kq) * 64 + wave * 16 + r];
#pragma unroll
        for (int rt = 0; rt < 3; ++rt) {
          const float a = Y[(rt * 16 + r) * kYld + 4 * s + kq];
          d[rt] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, d[rt], 0, 0, 0);
        }
      }
#pragma unroll
      for (int rt = 0; rt < 3; ++rt)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const int t = rt * 16 + 4 * kq + e;
          if (t < kSlots) V[t * 64 + wave * 16 + r] = d[rt][e];
        }
    }
    __syncthreads();
    // -- windowed sum: sample j of slot t = sum_i D[64 i + j] V_{t-2i}[j] + D[64 i + 32 + j] V_{t-2i-1}[32 + j]
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const int n = tid + e * kThreads;
      if (n < 576) {
        const int t = n / 32 + 15, j = n % 32;
        float s = 0.0f;
        for (int i = 0; i < 8; ++i) {
          s = fmaf(D[64 * i + j], V[(t - 2 * i) * 64 + j], s);
          s = fmaf(D[64 * i + 32 + j], V[(t - 2 * i - 1) * 64 + 32 + j], s);
        }
        if (mono) acc[e] += s;
        else {
          const int64_t o = o0 + n;
          if (o >= 0 && o < n_out) out[(int64_t)c * ch_stride + o] = s;
        }
      }
    }
  }
  if (mono) {
    const float inv = 1.0f / (float)nch;
#pragma unroll
    for (int e = 0; e < 3; ++e) {
      const int n = tid + e * kThreads;
      const int64_t o = o0 + n;
      if (n < 576 && o >= 0 && o < n_out) out[o] = acc[e] * inv;
    }
  }
}

__global__ void __launch_bounds__(kThreads) mp3_synth_kernel(const float* __restrict__ blk, const FileDev* __restrict__ files,
                                                             const int64_t* __restrict__ gpre, int n_files, int mono,
                                                             float* __restrict__ out) {
  const int64_t g = blockIdx.x;
  const int f = find_file(gpre, n_files, g);
  const FileDev fd = files[f];
  const int64_t gi = g - gpre[f];                    // granule index within the file
  const FileBlocks src{blk, fd.rec_offset, gi, fd.channels};
  mp3_synth_granule(src, fd.channels, mono, out + fd.out_offset, (int64_t)fd.n_out, gi * 576 - fd.skip, (int64_t)fd.n_out);
}

// ---- streams: the same two stages against two granules of carried blocks per stream -----------------------------------------------
struct SegDev { float* dst; float* state; int64_t rec_offset, ch_stride; int32_t granules, channels, skip, history; };
static_assert(sizeof(SegDev) == 48, "segment table layout");

__global__ void __launch_bounds__(kThreads) mp3_stream_synth_kernel(const float* __restrict__ blk, const SegDev* __restrict__ segs,
                                                                    const int64_t* __restrict__ gpre, int n_segs, int mono) {
  const int64_t g = blockIdx.x;
  const int f = find_file(gpre, n_segs, g);
  const SegDev sd = segs[f];
  const int64_t gi = g - gpre[f];                    // index among the segment's new granules
  const StreamBlocks src{blk, sd.state, sd.rec_offset, gi, sd.channels, sd.history};
  mp3_synth_granule(src, sd.channels, mono, sd.dst, sd.ch_stride, gi * 576 - sd.skip, (int64_t)sd.granules * 576 - sd.skip);
}

// After the synthesis: each stream's state becomes the blocks of its last two granules.  One workgroup column per segment; an
// element is read and written by one thread only, so the move {old last -> older, new -> last} of a single new granule is in place.
__global__ void __launch_bounds__(kThreads) mp3_stream_carry_kernel(const float* __restrict__ blk, const SegDev* __restrict__ segs) {
  const SegDev sd = segs[blockIdx.y];
  const int n = sd.channels * 1152;                  // floats of one granule's blocks (both channels)
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (sd.granules <= 0 || i >= n) return;
  const float* last = blk + (sd.rec_offset + (int64_t)(sd.granules - 1) * sd.channels) * 1152;
  sd.state[i] = sd.granules >= 2 ? last[i - n] : sd.state[n + i];
  sd.state[n + i] = last[i];
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

extern "C" int ss_mp3_synthesize(void* stream, const int16_t* d_q, const ss_mp3_granule* d_rec, int64_t n_rec,
                                 const ss_mp3_file* h_files, int n_files, int mono, float* d_out, int64_t out_floats,
                                 void* d_work, size_t* work_bytes) {
  if (!work_bytes || n_files < 0 || n_rec < 0 || (n_files > 0 && !h_files)) return SS_ERR_ARG;
  int64_t G = 0;
  std::vector<int64_t> gpre(n_files + 1);
  for (int i = 0; i < n_files; ++i) {
    const ss_mp3_file& F = h_files[i];
    const int64_t nsamp = (int64_t)F.granules * 576;
    if (F.channels < 1 || F.channels > 2 || F.granules < 0 || F.skip < 0 || F.n_out < 0 || F.rec_offset < 0 || F.out_offset < 0)
      return SS_ERR_ARG;
    if (F.rec_offset + (int64_t)F.granules * F.channels > n_rec) return SS_ERR_ARG;
    if ((int64_t)F.skip + F.n_out > nsamp) return SS_ERR_ARG;
    if (F.out_offset + (int64_t)F.n_out * (mono ? 1 : F.channels) > out_floats) return SS_ERR_CAPACITY;
    gpre[i] = G;
    G += F.granules;
  }
  gpre[n_files] = G;
  const size_t files_bytes = align256(sizeof(ss_mp3_file) * (size_t)(n_files > 0 ? n_files : 1));
  const size_t gpre_bytes = align256(sizeof(int64_t) * (size_t)(n_files + 1));
  const size_t need = files_bytes + gpre_bytes + (size_t)n_rec * 1152 * sizeof(float);
  if (!d_work) { *work_bytes = need; return SS_OK; }
  if (*work_bytes < need) return SS_ERR_CAPACITY;
  if (G == 0) return SS_OK;
  if (!d_q || !d_rec || !d_out) return SS_ERR_ARG;
  if (G > 0x7fffffff) return SS_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  std::vector<uint8_t> stage(files_bytes + gpre_bytes, 0);
  memcpy(stage.data(), h_files, sizeof(ss_mp3_file) * (size_t)n_files);
  memcpy(stage.data() + files_bytes, gpre.data(), sizeof(int64_t) * (size_t)(n_files + 1));
  uint8_t* w = (uint8_t*)d_work;
  // pageable source: the runtime has staged it when the call returns, so `stage` may go out of scope
  SS_HIP_CHECK(hipMemcpyAsync(w, stage.data(), stage.size(), hipMemcpyHostToDevice, st));
  const FileDev* files = (const FileDev*)w;
  const int64_t* dg = (const int64_t*)(w + files_bytes);
  float* blk = (float*)(w + files_bytes + gpre_bytes);
  hipLaunchKernelGGL(mp3_imdct_kernel, dim3((unsigned)G), dim3(kThreads), 0, st, d_q, d_rec, files, dg, n_files, blk);
  SS_LAUNCH_CHECK();
  hipLaunchKernelGGL(mp3_synth_kernel, dim3((unsigned)G), dim3(kThreads), 0, st, blk, files, dg, n_files, mono ? 1 : 0, d_out);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

extern "C" int ss_mp3_stream_synthesize(void* stream, const int16_t* d_q, const ss_mp3_granule* d_rec, int64_t n_rec,
                                        const ss_mp3_stream_seg* h_segs, int n_segs, float* const* h_state, float* const* h_dst,
                                        const int64_t* h_dst_cap, int n_dst, int mono, void* d_work, size_t* work_bytes) {
  if (!work_bytes || n_segs < 0 || n_rec < 0 || n_dst < 0 || (n_segs > 0 && (!h_segs || !h_state || !h_dst || !h_dst_cap)))
    return SS_ERR_ARG;
  // every refusal before any HIP call: arguments first, capacities second
  int64_t G = 0;
  std::vector<int64_t> gpre(n_segs + 1);
  for (int i = 0; i < n_segs; ++i) {
    const ss_mp3_stream_seg& S = h_segs[i];
    if (S.channels < 1 || S.channels > 2 || S.granules < 0 || S.history < 0 || S.history > 2 || S.rec_offset < 0 || S.dst_offset < 0 ||
        S.ch_stride < 0 || S.dst < 0 || S.dst >= n_dst || S.skip < 0 || (int64_t)S.skip > (int64_t)S.granules * 576)
      return SS_ERR_ARG;
    if (S.rec_offset + (int64_t)S.granules * S.channels > n_rec) return SS_ERR_ARG;
    if (S.granules > 0 && !h_state[i]) return SS_ERR_ARG;
    if ((int64_t)S.granules * 576 > S.skip && !h_dst[S.dst]) return SS_ERR_ARG;               // something is written
    if (!mono && S.channels == 2 && S.ch_stride < (int64_t)S.granules * 576 - S.skip) return SS_ERR_ARG;   // the planes would overlap
    gpre[i] = G;
    G += S.granules;
  }
  gpre[n_segs] = G;
  if (G > 0x7fffffff) return SS_ERR_ARG;
  for (int i = 0; i < n_segs; ++i) {
    const ss_mp3_stream_seg& S = h_segs[i];
    const int64_t n_out = (int64_t)S.granules * 576 - S.skip;
    const int64_t planes = mono ? 0 : S.channels - 1;
    if (n_out > 0 && S.dst_offset + planes * S.ch_stride + n_out > h_dst_cap[S.dst]) return SS_ERR_CAPACITY;
  }
  const size_t nt = (size_t)(n_segs > 0 ? n_segs : 1);
  const size_t files_bytes = align256(sizeof(FileDev) * nt), segs_bytes = align256(sizeof(SegDev) * nt);
  const size_t gpre_bytes = align256(sizeof(int64_t) * (size_t)(n_segs + 1));
  const size_t need = files_bytes + segs_bytes + gpre_bytes + (size_t)n_rec * 1152 * sizeof(float);
  if (!d_work) { *work_bytes = need; return SS_OK; }
  if (*work_bytes < need) return SS_ERR_CAPACITY;
  if (G == 0) return SS_OK;
  if (!d_q || !d_rec) return SS_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  std::vector<uint8_t> stage(files_bytes + segs_bytes + gpre_bytes, 0);
  FileDev* hf = (FileDev*)stage.data();
  SegDev* hs = (SegDev*)(stage.data() + files_bytes);
  for (int i = 0; i < n_segs; ++i) {
    const ss_mp3_stream_seg& S = h_segs[i];
    hf[i] = FileDev{S.rec_offset, 0, S.granules, S.channels, 0, 0};                          // what the IMDCT kernel reads of a file
    hs[i] = SegDev{h_dst[S.dst] ? h_dst[S.dst] + S.dst_offset : nullptr, h_state[i], S.rec_offset, S.ch_stride, S.granules,
                   S.channels, S.skip, S.history};
  }
  memcpy(stage.data() + files_bytes + segs_bytes, gpre.data(), sizeof(int64_t) * (size_t)(n_segs + 1));
  uint8_t* w = (uint8_t*)d_work;
  // pageable source: the runtime has staged it when the call returns, so `stage` may go out of scope
  SS_HIP_CHECK(hipMemcpyAsync(w, stage.data(), stage.size(), hipMemcpyHostToDevice, st));
  const FileDev* files = (const FileDev*)w;
  const SegDev* segs = (const SegDev*)(w + files_bytes);
  const int64_t* dg = (const int64_t*)(w + files_bytes + segs_bytes);
  float* blk = (float*)(w + files_bytes + segs_bytes + gpre_bytes);
  hipLaunchKernelGGL(mp3_imdct_kernel, dim3((unsigned)G), dim3(kThreads), 0, st, d_q, d_rec, files, dg, n_segs, blk);
  SS_LAUNCH_CHECK();
  hipLaunchKernelGGL(mp3_stream_synth_kernel, dim3((unsigned)G), dim3(kThreads), 0, st, blk, segs, dg, n_segs, mono ? 1 : 0);
  SS_LAUNCH_CHECK();
  hipLaunchKernelGGL(mp3_stream_carry_kernel, dim3((2 * 1152 + kThreads - 1) / kThreads, (unsigned)n_segs), dim3(kThreads), 0, st, blk,
                     segs);
  SS_LAUNCH_CHECK();
  return SS_OK;
}
