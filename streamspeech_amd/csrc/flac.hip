// FLAC ingest, device stage (gfx950): the predictor, the wasted-bits shift, the inter-channel decorrelation and the float
// conversion of a ragged batch of files in ONE launch -- one workgroup per frame, one wave per subframe of it.
//
// The recurrence s[i] = r[i] + ((sum_j coef[j] * s[i-1-j]) >> shift) is serial inside a subframe (the shift makes it non-linear),
// so a wave spreads the TAPS over its lanes: lane j < 32 keeps the sample s[p] with p = j (mod 32) -- a ring that is never
// indexed by a runtime value, because lane j simply overwrites its place when i = j (mod 32) -- and, for each of the 32 phases
// of i, the coefficient that belongs to its place in that phase (32 registers, selected by the unrolled loop's compile-time
// phase).  One step is a multiply, a 4-step DPP butterfly inside each row of 16 lanes, two v_readlane that add the two rows on
// the scalar unit, the shift and the add -- no LDS, no scratch.  Fixed predictors are LPC with the binomial taps the host stage
// wrote into the record, constant and verbatim subframes are order 0.  64 residuals are loaded per lane-coalesced read and 64
// restored samples written per lane-coalesced store into the workspace; after a workgroup barrier every thread of the frame reads
// all channels of a sample from there, undoes the stereo decorrelation and writes float(s) * 2^-(bps-1).
// The accumulator is 32 bits where libFLAC's rule proves that exact (flac.hpp needs_wide), 64 bits otherwise.
#include <hip/hip_runtime.h>
#include <string.h>

#include <vector>

#include "../../include/streamspeech_hip.h"
#include "common.hpp"
#include "flac.hpp"

namespace {

struct FileDev { int64_t rec_offset, out_offset; int32_t frames, channels, bps, n_out; };
static_assert(sizeof(FileDev) == sizeof(ss_flac_file), "file table layout");

__device__ inline int find_file(const int64_t* gpre, int n_files, int64_t g) {
  int lo = 0, hi = n_files;                          // gpre[lo] <= g < gpre[hi]
  while (hi - lo > 1) {
    int mid = (lo + hi) >> 1;
    if (gpre[mid] <= g) lo = mid; else hi = mid;
  }
  return lo;
}

// x + (x of the lane the DPP control names): quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror in turn leave
// the sum of a row's 16 lanes in every lane of the row (integer adds: the order does not matter)
template <int CTRL>
__device__ inline uint32_t dpp(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, 0xf, 0xf, false);
}

__device__ inline uint32_t row_sum(uint32_t x) {
  x += dpp<0xB1>(x);
  x += dpp<0x4E>(x);
  x += dpp<0x141>(x);
  x += dpp<0x140>(x);
  return x;
}

__device__ inline uint64_t row_sum(uint64_t x) {
#define SS_FLAC_STEP(CTRL) x += ((uint64_t)dpp<CTRL>((uint32_t)(x >> 32)) << 32) | dpp<CTRL>((uint32_t)x)
  SS_FLAC_STEP(0xB1);
  SS_FLAC_STEP(0x4E);
  SS_FLAC_STEP(0x141);
  SS_FLAC_STEP(0x140);
#undef SS_FLAC_STEP
  return x;
}

__device__ inline int32_t rows01(uint32_t x) {       // lanes 0-31 hold the taps: row 0 + row 1, uniform
  return (int32_t)((uint32_t)__builtin_amdgcn_readlane((int)x, 0) + (uint32_t)__builtin_amdgcn_readlane((int)x, 16));
}

__device__ inline int64_t rows01(uint64_t x) {
  const uint32_t lo0 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, 0), hi0 = (uint32_t)__builtin_amdgcn_readlane((int)(x >> 32), 0);
  const uint32_t lo1 = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)x, 16), hi1 = (uint32_t)__builtin_amdgcn_readlane((int)(x >> 32), 16);
  return (int64_t)((((uint64_t)hi0 << 32) | lo0) + (((uint64_t)hi1 << 32) | lo1));
}

// One subframe by one wave: d_res[res_offset ..) -> work[res_offset ..), wasted-bits shift applied.
template <typename U, typename S>                    // (uint32_t, int32_t) or (uint64_t, int64_t): the accumulator
__device__ inline void restore_subframe(const int32_t* __restrict__ res, int32_t* __restrict__ dst, const ss_flac_subframe& r,
                                        int lane) {
  const int n = r.block_size, order = r.order, shift = r.shift, wasted = r.wasted;
  const bool constant = r.type == SS_FLAC_CONSTANT;
  // c[ph]: the coefficient of this lane's place while i = ph (mod 32): the place holds s[i-1-j] with j = (ph - 1 - lane) mod 32
  int32_t c[32];
#pragma unroll
  for (int ph = 0; ph < 32; ++ph) {
    const int j = (ph - 1 - lane) & 31;
    c[ph] = (lane < 32 && j < order) ? (int32_t)r.coef[j] : 0;
  }
  int32_t hist = 0;
  for (int base = 0; base < n; base += 64) {
    const int at = constant ? 0 : base + lane;
    const int32_t rv = (constant || at < n) ? res[at] : 0;
    int32_t outv = 0;
#pragma unroll
    for (int k = 0; k < 64; ++k) {
      const int ph = k & 31;
      const U prod = (U)(S)c[ph] * (U)(S)hist;
      const S tot = rows01(row_sum(prod));
      const int32_t rk = __builtin_amdgcn_readlane(rv, k);
      const int32_t v = (base + k < order) ? rk : flac::add_wrap(rk, (int32_t)(tot >> shift));
      if (lane == ph) hist = v;
      if (lane == k) outv = v;
    }
    if (base + lane < n) dst[base + lane] = flac::shl_wrap(outv, wasted);
  }
}

// grid = frames of the batch, block = 64 * (most channels of a file of the batch)
__global__ __launch_bounds__(512) void flac_restore_kernel(const int32_t* __restrict__ res, const ss_flac_subframe* __restrict__ rec,
                                                           int64_t n_res, const FileDev* __restrict__ files,
                                                           const int64_t* __restrict__ gpre, int n_files, int mono,
                                                           int32_t* __restrict__ work, float* __restrict__ out) {
  __shared__ ss_flac_subframe srec[8];
  __shared__ int bad;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t g = blockIdx.x;
  const int f = find_file(gpre, n_files, g);
  const FileDev fd = files[f];
  const int nch = fd.channels;
  const ss_flac_subframe* R = rec + fd.rec_offset + (g - gpre[f]) * nch;
  if (tid == 0) bad = 0;
  for (int i = tid; i < nch * (int)(sizeof(ss_flac_subframe) / 4); i += blockDim.x)
    ((int32_t*)srec)[i] = ((const int32_t*)R)[i];
  __syncthreads();
  if (tid < nch) {
    const ss_flac_subframe& r = srec[tid];
    if (!flac::record_ok(r, n_res, fd.n_out) || r.block_size != srec[0].block_size || r.sample_start != srec[0].sample_start)
      bad = 1;
  }
  __syncthreads();
  if (bad) return;                                   // the whole workgroup: such a frame writes nothing
  if (wave < nch) {
    const ss_flac_subframe& r = srec[wave];
    if (flac::needs_wide(r)) restore_subframe<uint64_t, int64_t>(res + r.res_offset, work + r.res_offset, r, lane);
    else restore_subframe<uint32_t, int32_t>(res + r.res_offset, work + r.res_offset, r, lane);
  }
  __syncthreads();                                   // the frame's subframes are in `work`, written by this workgroup
  const int n = srec[0].block_size, assignment = srec[0].assignment;
  const int64_t t0 = srec[0].sample_start;
  const float scale = flac::scale_of(fd.bps), inv = 1.0f / (float)nch;
  float* o = out + fd.out_offset + t0;
  for (int i = tid; i < n; i += blockDim.x) {
    int32_t s[8];
#pragma unroll
    for (int c = 0; c < 8; ++c) s[c] = c < nch ? work[srec[c].res_offset + i] : 0;
    if (nch == 2) flac::undo_stereo(assignment, s[0], s[1], s[0], s[1]);
    if (mono) {
      float acc = (float)s[0] * scale;
#pragma unroll
      for (int c = 1; c < 8; ++c) if (c < nch) acc += (float)s[c] * scale;
      o[i] = nch > 1 ? acc * inv : acc;
    } else {
#pragma unroll
      for (int c = 0; c < 8; ++c) if (c < nch) o[(int64_t)c * fd.n_out + i] = (float)s[c] * scale;
    }
  }
}

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

}  // namespace

extern "C" int ss_flac_restore(void* stream, const int32_t* d_res, const ss_flac_subframe* d_rec, int64_t n_rec, int64_t n_res,
                               const ss_flac_file* h_files, int n_files, int mono, float* d_out, int64_t out_floats,
                               void* d_work, size_t* work_bytes) {
  if (!work_bytes || n_files < 0 || n_rec < 0 || n_res < 0 || out_floats < 0 || (n_files > 0 && !h_files)) return SS_ERR_ARG;
  int64_t G = 0;
  int max_ch = 1;
  std::vector<int64_t> gpre(n_files + 1);
  for (int i = 0; i < n_files; ++i) {
    const ss_flac_file& F = h_files[i];
    if (F.channels < 1 || F.channels > 8 || F.bps < 4 || F.bps > 24 || F.frames < 0 || F.n_out < 0 || F.rec_offset < 0 ||
        F.out_offset < 0)
      return SS_ERR_ARG;
    if (F.rec_offset + (int64_t)F.frames * F.channels > n_rec) return SS_ERR_ARG;
    gpre[i] = G;
    G += F.frames;
    if (F.channels > max_ch) max_ch = F.channels;
  }
  for (int i = 0; i < n_files; ++i) {
    const ss_flac_file& F = h_files[i];
    if (F.out_offset + (int64_t)F.n_out * (mono ? 1 : F.channels) > out_floats) return SS_ERR_CAPACITY;
  }
  gpre[n_files] = G;
  const size_t files_bytes = align256(sizeof(ss_flac_file) * (size_t)(n_files > 0 ? n_files : 1));
  const size_t gpre_bytes = align256(sizeof(int64_t) * (size_t)(n_files + 1));
  const size_t need = files_bytes + gpre_bytes + (size_t)n_res * sizeof(int32_t);
  if (!d_work) { *work_bytes = need; return SS_OK; }
  if (*work_bytes < need) return SS_ERR_CAPACITY;
  if (G == 0) return SS_OK;
  if (!d_res || !d_rec || !d_out) return SS_ERR_ARG;
  if (G > 0x7fffffff) return SS_ERR_ARG;
  hipStream_t st = (hipStream_t)stream;
  std::vector<uint8_t> stage(files_bytes + gpre_bytes, 0);
  memcpy(stage.data(), h_files, sizeof(ss_flac_file) * (size_t)n_files);
  memcpy(stage.data() + files_bytes, gpre.data(), sizeof(int64_t) * (size_t)(n_files + 1));
  uint8_t* w = (uint8_t*)d_work;
  // pageable source: the runtime has staged it when the call returns, so `stage` may go out of scope
  SS_HIP_CHECK(hipMemcpyAsync(w, stage.data(), stage.size(), hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(flac_restore_kernel, dim3((unsigned)G), dim3(64 * max_ch), 0, st, d_res, d_rec, n_res, (const FileDev*)w,
                     (const int64_t*)(w + files_bytes), n_files, mono ? 1 : 0, (int32_t*)(w + files_bytes + gpre_bytes), d_out);
  SS_LAUNCH_CHECK();
  return SS_OK;
}
