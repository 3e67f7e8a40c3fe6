// Fused Kaldi-compatible fbank + global CMVN.
//
// Replaces OnlineFeatureExtractor -> torchaudio.compliance.kaldi.fbank -> (x-mean)/std
// (reference agent/speech_to_speech.streamspeech.agent.py:66-98, fairseq/data/audio/audio_utils.py:236-249)
// with ONE kernel: workgroup = one 25 ms frame, everything between the coalesced PCM read and the
// 80-float feature row write stays in LDS: DC removal, pre-emphasis 0.97, Povey window, 512-point
// radix-2 FFT, power spectrum, 80 triangular mel bins, log floor, CMVN.
#include "fbank.hpp"

namespace ss {

constexpr int WIN = 400, SHIFT = 160, NFFT = 512, NBIN = 257, NMEL = 80;

// One fbank row from the frame's 400 samples, two per thread: v0 = sample t, v1 = sample t + 256 (ignored from t = 144 on), both
// unscaled.  Shared by fbank_cmvn_kernel (samples loaded) and fbank_cmvn_sr_kernel (samples formed by the resampling prologue), so
// the row is ONE piece of code: the scale multiplies where it always did (hipcc contracts x0 + x1 into an fma with it), and both
// kernels get the same contraction of every expression below -- the row's bits depend on the two sample values only.
// `tabs` (fbank.hpp) holds what is the same for every frame: with tabs.twiddle the twiddles are read from the table
// fbank_twiddle_kernel filled with the expression below (the same bits), with tabs.mel_range mel row t walks its bins [lo, hi) only --
// the bins outside are exact zeros of melw, fmaf(0, x, e) == e for the finite power spectrum and e starts at +0, so the ascending
// walk over the range is the dense walk's chain with its no-ops left out (the same bits).  A null pointer keeps the in-kernel form.
__device__ __forceinline__ void fbank_row(const float v0, const float v1, const float pcm_scale,
                                          const float* __restrict__ window,   // [400]
                                          const float* __restrict__ melw,     // [80][257]
                                          const FbankTables tabs,
                                          const float* __restrict__ cmvn_mean, const float* __restrict__ cmvn_std,
                                          float* __restrict__ feat_row) {
  __shared__ float re[NFFT], im[NFFT];
  __shared__ float tw_c[NFFT / 2], tw_s[NFFT / 2];
  __shared__ float red[4];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  // frame mean
  const float x0 = v0 * pcm_scale;
  const float x1 = (t + 256 < WIN) ? v1 * pcm_scale : 0.f;
  float s = wave_sum(x0 + x1);
  if (lane == 0) red[wave] = s;
  // twiddles e^{-2 pi i k / 512}
  if (tabs.twiddle) {
    tw_c[t] = tabs.twiddle[t]; tw_s[t] = tabs.twiddle[NFFT / 2 + t];
  } else {
    float sn, cs;
    sincospif(-2.0f * (float)t / (float)NFFT, &sn, &cs);
    tw_c[t] = cs; tw_s[t] = sn;
  }
  __syncthreads();
  const float mean = (red[0] + red[1] + red[2] + red[3]) / (float)WIN;
  re[t] = x0 - mean;
  re[t + 256] = (t + 256 < WIN) ? (x1 - mean) : 0.f;
  __syncthreads();
  // pre-emphasis (replicate-pad on the left) + window, written in bit-reversed order for the DIT FFT
  float y0, y1 = 0.f;
  {
    const float prev0 = re[t > 0 ? t - 1 : 0];
    y0 = (re[t] - 0.97f * prev0) * window[t];
    if (t + 256 < WIN) y1 = (re[t + 256] - 0.97f * re[t + 255]) * window[t + 256];
  }
  __syncthreads();
  re[__brev((unsigned)t) >> 23] = y0;
  re[__brev((unsigned)(t + 256)) >> 23] = y1;
  im[t] = 0.f; im[t + 256] = 0.f;
  __syncthreads();
  // 9 radix-2 stages, one butterfly per thread
#pragma unroll
  for (int stg = 0; stg < 9; ++stg) {
    const int half = 1 << stg;
    const int grp = t >> stg, pos = t & (half - 1);
    const int i0 = (grp << (stg + 1)) + pos, i1 = i0 + half;
    const int tk = pos << (8 - stg);
    const float c = tw_c[tk], sn = tw_s[tk];
    const float br = re[i1] * c - im[i1] * sn;
    const float bi = re[i1] * sn + im[i1] * c;
    const float ar = re[i0], ai = im[i0];
    __syncthreads();
    re[i0] = ar + br; im[i0] = ai + bi;
    re[i1] = ar - br; im[i1] = ai - bi;
    __syncthreads();
  }
  // power spectrum into re[0..256]
  const float p0 = re[t] * re[t] + im[t] * im[t];
  const float p256 = (t == 0) ? (re[256] * re[256] + im[256] * im[256]) : 0.f;
  __syncthreads();
  re[t] = p0;
  if (t == 0) re[256] = p256;
  __syncthreads();
  if (t < NMEL) {
    const float* w = melw + t * NBIN;
    int lo = 0, hi = NBIN;
    if (tabs.mel_range) {                       // clamped: the table is device memory, the walk never leaves the row
      lo = max(tabs.mel_range[2 * t], 0); hi = min(tabs.mel_range[2 * t + 1], NBIN);
    }
    float e = 0.f;
    for (int i = lo; i < hi; ++i) e = fmaf(w[i], re[i], e);
    const float lg = logf(fmaxf(e, 1.1920928955078125e-07f));
    feat_row[t] = (lg - cmvn_mean[t]) / cmvn_std[t];
  }
}

__global__ __launch_bounds__(256) void fbank_cmvn_kernel(const float* __restrict__ pcm, float pcm_scale,
                                                         const float* __restrict__ window,   // [400]
                                                         const float* __restrict__ melw,     // [80][257]
                                                         const FbankTables tabs,
                                                         const float* __restrict__ cmvn_mean,
                                                         const float* __restrict__ cmvn_std, float* feat,
                                                         const int* __restrict__ segs,
                                                         const float* const* __restrict__ pcm_ptrs,
                                                         float* const* __restrict__ feat_ptrs) {
  const int t = threadIdx.x;
  const int frame = blockIdx.x;
  if (segs) {   // ragged batch {pcm_start, n_frames, frame_start}; whole workgroup exits together
    const int* sg = segs + 3 * blockIdx.y;
    if (frame >= sg[1]) return;
    if (pcm_ptrs) { pcm = pcm_ptrs[blockIdx.y]; feat = feat_ptrs[blockIdx.y]; }   // per-segment buffers (launch_fbank_cmvn_ptrs)
    pcm += sg[0]; feat += (size_t)sg[2] * NMEL;
  }
  const float* src = pcm + (size_t)frame * SHIFT;
  // load (coalesced)
  fbank_row(src[t], (t + 256 < WIN) ? src[t + 256] : 0.f, pcm_scale, window, melw, tabs, cmvn_mean, cmvn_std, feat + (size_t)frame * NMEL);
}

// The twiddle table of FbankTables: fbank_row's own expression, once (cos [256] then sin [256]).
__global__ __launch_bounds__(256) void fbank_twiddle_kernel(float* __restrict__ tw) {
  const int t = threadIdx.x;
  float sn, cs;
  sincospif(-2.0f * (float)t / (float)NFFT, &sn, &cs);
  tw[t] = cs; tw[NFFT / 2 + t] = sn;
}

int launch_fbank_twiddles(float* tw, hipStream_t stream) {
  if (!tw) return SS_ERR_ARG;
  hipLaunchKernelGGL(fbank_twiddle_kernel, dim3(1), dim3(NFFT / 2), 0, stream, tw);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

int fbank_mel_ranges(const float* melw, int rows, int cols, int* lo_hi) {
  if (!melw || !lo_hi || rows < 0 || cols < 0) return SS_ERR_ARG;
  for (int r = 0; r < rows; ++r) {
    const float* w = melw + (size_t)r * cols;
    int lo = 0, hi = 0;                               // an all-zero row: the empty range [0, 0)
    for (int i = 0; i < cols; ++i)
      if (w[i] != 0.f) { if (hi == 0) lo = i; hi = i + 1; }   // (a NaN weight counts as non-zero: it stays in the walk)
    lo_hi[2 * r] = lo; lo_hi[2 * r + 1] = hi;
  }
  return SS_OK;
}

int launch_fbank_cmvn(const float* pcm, int n_samples, float pcm_scale, const float* window,
                      const float* melw, const FbankTables& tabs, const float* cmvn_mean, const float* cmvn_std, float* feat,
                      int* n_frames, hipStream_t stream) {
  const int T = n_samples < WIN ? 0 : 1 + (n_samples - WIN) / SHIFT;
  if (n_frames) *n_frames = T;
  if (T == 0) return SS_OK;
  hipLaunchKernelGGL(fbank_cmvn_kernel, dim3(T), dim3(256), 0, stream, pcm, pcm_scale, window, melw,
                     tabs, cmvn_mean, cmvn_std, feat, (const int*)nullptr, (const float* const*)nullptr, (float* const*)nullptr);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

int launch_fbank_cmvn_batch(const float* pcm, float pcm_scale, const float* window, const float* melw,
                            const FbankTables& tabs, const float* cmvn_mean, const float* cmvn_std, float* feat, const int* segs, int nseg,
                            int max_frames, hipStream_t stream) {
  if (nseg <= 0 || max_frames <= 0) return SS_OK;
  hipLaunchKernelGGL(fbank_cmvn_kernel, dim3(max_frames, nseg), dim3(256), 0, stream, pcm, pcm_scale, window, melw,
                     tabs, cmvn_mean, cmvn_std, feat, segs, (const float* const*)nullptr, (float* const*)nullptr);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// Global CMVN alone, for fbank rows that were computed elsewhere (the recipe's precomputed features): the last line of fbank_row,
// one thread per value over the packed rows.
__global__ __launch_bounds__(256) void cmvn_rows_kernel(const float* in, const float* __restrict__ cmvn_mean,
                                                        const float* __restrict__ cmvn_std, float* out, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int t = (int)(i % NMEL);
  const float lg = in[i];
  out[i] = (lg - cmvn_mean[t]) / cmvn_std[t];
}

int launch_cmvn_rows(const float* in, long long rows, const float* cmvn_mean, const float* cmvn_std, float* out, hipStream_t stream) {
  if (rows <= 0) return SS_OK;
  const long long n = rows * NMEL, blocks = (n + 255) / 256;
  if (blocks > 0x7fffffffLL) return SS_ERR_ARG;
  hipLaunchKernelGGL(cmvn_rows_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, in, cmvn_mean, cmvn_std, out, n);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

int launch_fbank_cmvn_ptrs(const float* const* pcm_ptrs, float* const* feat_ptrs, float pcm_scale, const float* window,
                           const float* melw, const FbankTables& tabs, const float* cmvn_mean, const float* cmvn_std,
                           const int* segs, int nseg, int max_frames, hipStream_t stream) {
  if (nseg <= 0 || max_frames <= 0) return SS_OK;
  hipLaunchKernelGGL(fbank_cmvn_kernel, dim3(max_frames, nseg), dim3(256), 0, stream, (const float*)nullptr, pcm_scale, window, melw,
                     tabs, cmvn_mean, cmvn_std, (float*)nullptr, segs, pcm_ptrs, feat_ptrs);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// ---------------------------------------------------------------------------------------------
// Rational polyphase resampler (48 kHz -> 16 kHz in the agent).  Replaces the sox `rate` effect
// the reference applies to the whole sample history at every chunk
// (fairseq/data/audio/audio_utils.py:53-62 <- convert_waveform <- agent :66-98) with a zero-phase
// windowed-sinc FIR: y[k] = sum_m x[m] * h[half + k*down - m*up].  The taps (host-designed, gain
// `up`) are ~60/output sample for 3:1: a thread per output sample, taps through LDS when they fit.
// HBM-bound by construction: 4*(n_in + n_out) bytes.
// ---------------------------------------------------------------------------------------------
// (resample_sample, the ONE copy of the sum, lives in fbank.hpp: this kernel, the resampling prologue of fbank_cmvn_sr_kernel and
// the streaming output resampler of pcm.hip, device and host, compile it.)
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ x, long long n_in, int up, int down,
                                                       const float* __restrict__ h, int half, float* __restrict__ y,
                                                       long long n_out) {
  extern __shared__ float hs[];
  const int ntaps = 2 * half + 1;
  for (int i = threadIdx.x; i < ntaps; i += 256) hs[i] = h[i];
  __syncthreads();
  const long long k = (long long)blockIdx.x * 256 + threadIdx.x;
  if (k >= n_out) return;
  y[k] = resample_sample(x, n_in, up, down, hs, half, k);
}

int launch_resample(const float* x, long long n_in, int up, int down, const float* taps, int half_len, float* y,
                    long long n_out, hipStream_t stream) {
  if (n_in <= 0 || n_out <= 0) return SS_OK;
  if (up <= 0 || down <= 0 || half_len < 0) return SS_ERR_ARG;
  const size_t lds = (size_t)(2 * half_len + 1) * sizeof(float);
  if (lds > 64 * 1024) return SS_ERR_ARG;             // 16 K taps: ratios up to ~800:1 in lowest terms
  hipLaunchKernelGGL(resample_kernel, dim3((unsigned)((n_out + 255) / 256)), dim3(256), lds, stream, x, n_in, up, down,
                     taps, half_len, y, n_out);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

// ---------------------------------------------------------------------------------------------
// fbank rows of streaming sessions at ANY source rate, from the source-rate history directly: workgroup = one row of one session
// (the grid and ragged exit of launch_fbank_cmvn_ptrs).  Each thread forms its one or two 16-kHz samples 160 f + t (+ 256) of the
// row with resample_sample -- the resampler's own sum, so they are the samples ss_resample would have written -- keeps them in
// registers and the row goes through fbank_row: the bits of fbank_cmvn(resample(x[:n_in])) without the 16-kHz history in between.
// The session's taps sit in LDS beside fbank_row's arrays (a table per segment: the sessions of a launch may differ in ratio).
// A segment with up == down is already at 16 kHz: its samples are loaded, as fbank_cmvn_kernel loads them.
// ---------------------------------------------------------------------------------------------
constexpr size_t FBANK_ROW_LDS = (2 * NFFT + 2 * (NFFT / 2) + 4) * sizeof(float);   // fbank_row's static arrays
constexpr size_t WG_LDS = 64 * 1024;                                                // what a workgroup gets without asking for more
constexpr int FBANK_SR_MAX_HALF = (int)(((WG_LDS - FBANK_ROW_LDS) / sizeof(float) - 1) / 2);   // 2 half + 1 taps beside the row's arrays

__global__ __launch_bounds__(256) void fbank_cmvn_sr_kernel(const FbankSrSeg* __restrict__ segs, float pcm_scale,
                                                            const float* __restrict__ window, const float* __restrict__ melw,
                                                            const FbankTables tabs, const float* __restrict__ cmvn_mean,
                                                            const float* __restrict__ cmvn_std) {
  extern __shared__ float hs[];
  const FbankSrSeg sg = segs[blockIdx.y];
  if ((int)blockIdx.x >= sg.n_rows) return;           // ragged batch: the whole workgroup exits together
  const int t = threadIdx.x;
  const long long k0 = (long long)(sg.first + (int)blockIdx.x) * SHIFT + t;
  float v0, v1 = 0.f;
  if (sg.up == sg.down) {
    v0 = sg.pcm[k0];
    if (t + 256 < WIN) v1 = sg.pcm[k0 + 256];
  } else {
    const int ntaps = 2 * sg.half + 1;
    for (int i = t; i < ntaps; i += 256) hs[i] = sg.taps[i];
    __syncthreads();
    v0 = resample_sample(sg.pcm, sg.n_in, sg.up, sg.down, hs, sg.half, k0);
    if (t + 256 < WIN) v1 = resample_sample(sg.pcm, sg.n_in, sg.up, sg.down, hs, sg.half, k0 + 256);
  }
  fbank_row(v0, v1, pcm_scale, window, melw, tabs, cmvn_mean, cmvn_std, sg.feat + (size_t)blockIdx.x * NMEL);
}

int fbank_sr_rows(long long n_in, int up, int down, int half_len, int* n_rows, int* n_final) {
  if (n_in < 0 || up < 1 || down < 1 || half_len < 0) return SS_ERR_ARG;
  if (half_len > FBANK_SR_MAX_HALF) return SS_ERR_ARG;                                             // the taps do not fit the workgroup's LDS
  if (n_in > (long long)0x7fffffff || n_in * up > (long long)0x7fffffff * down) return SS_ERR_ARG;   // 16-kHz sample indices are ints
  const long long n16 = (n_in * up + down - 1) / down;
  const long long rows = n16 < WIN ? 0 : 1 + (n16 - WIN) / SHIFT;
  // sample K is settled iff its window's last input (K down + half) / up exists: K down + half < n_in up
  const long long top = n_in * up - 1 - half_len;
  long long fin = 0;
  if (top >= 0) {
    const long long kmax = top / down;                // the last settled sample
    if (kmax >= WIN - 1) fin = 1 + (kmax - (WIN - 1)) / SHIFT;
  }
  if (fin > rows) fin = rows;
  if (n_rows) *n_rows = (int)rows;
  if (n_final) *n_final = (int)fin;
  return SS_OK;
}

int launch_fbank_cmvn_sr(const FbankSrSeg* segs, int nseg, int max_rows, int max_taps, float pcm_scale, const float* window,
                         const float* melw, const FbankTables& tabs, const float* cmvn_mean, const float* cmvn_std,
                         hipStream_t stream) {
  if (nseg <= 0 || max_rows <= 0) return SS_OK;
  if (max_taps < 0 || max_taps > 2 * FBANK_SR_MAX_HALF + 1) return SS_ERR_ARG;
  const size_t lds = (size_t)max_taps * sizeof(float);
  hipLaunchKernelGGL(fbank_cmvn_sr_kernel, dim3(max_rows, nseg), dim3(256), lds, stream, segs, pcm_scale, window, melw, tabs,
                     cmvn_mean, cmvn_std);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

}  // namespace ss
