// Fused fbank + CMVN front-end kernel (see fbank.hip).
#pragma once
#include <math.h>

#include "common.hpp"

namespace ss {

// What fbank_row reads that is the same for every frame, made once per model (ss_model_create) and kept on the device next to melw:
// the first and one-past-the-last non-zero bin of every mel row, and the FFT's 256 twiddles.  Either pointer may be null: that part
// of the row then runs as it did before the tables existed (the dense 257-bin walk, sincospif in the kernel) -- the same bits.
struct FbankTables {
  const int* mel_range = nullptr;     // [80][2] {lo, hi}: mel row t is zero outside bins [lo, hi)
  const float* twiddle = nullptr;     // cos [256] then sin [256] of -2 pi k / 512, from fbank_row's own sincospif expression
};

// Host only, no GPU needed: lo_hi[2 r] / lo_hi[2 r + 1] = the first non-zero index of row r of melw [rows][cols] and one past the
// last (an all-zero row: 0, 0 -- an empty range).
int fbank_mel_ranges(const float* melw, int rows, int cols, int* lo_hi);
// tw [512] on the device <- the twiddle table of FbankTables (one small launch).
int launch_fbank_twiddles(float* tw, hipStream_t stream);

// pcm: mono 16 kHz float samples on the device; each sample is multiplied by pcm_scale (2^15 for
// [-1,1] input, reference fairseq/examples/speech_to_text/data_utils.py:85).  window [400] and
// melw [80][257] are host-built constants living in the weight blob.  Writes feat [T,80] and
// returns T = 1 + (n-400)/160 (snip_edges) through n_frames (host int).
int launch_fbank_cmvn(const float* pcm, int n_samples, float pcm_scale, const float* window,
                      const float* melw, const FbankTables& tabs, const float* cmvn_mean, const float* cmvn_std, float* feat,
                      int* n_frames, hipStream_t stream);

// Ragged batch: segs[3*s] = {pcm_start, n_frames, frame_start} into the packed PCM / feature arrays.
int launch_fbank_cmvn_batch(const float* pcm, float pcm_scale, const float* window, const float* melw,
                            const FbankTables& tabs, const float* cmvn_mean, const float* cmvn_std, float* feat, const int* segs, int nseg,
                            int max_frames, hipStream_t stream);

// Ragged batch over separate buffers: segment s reads pcm_ptrs[s] and writes feat_ptrs[s] (device arrays of device pointers);
// segs[3*s] = {pcm_start, n_frames, frame_start} are offsets into those buffers.  Same kernel, same bits per frame.
int launch_fbank_cmvn_ptrs(const float* const* pcm_ptrs, float* const* feat_ptrs, float pcm_scale, const float* window,
                           const float* melw, const FbankTables& tabs, const float* cmvn_mean, const float* cmvn_std,
                           const int* segs, int nseg, int max_frames, hipStream_t stream);

// out[r][c] = (in[r][c] - cmvn_mean[c]) / cmvn_std[c] over `rows` packed rows of 80: fbank_row's last line on rows computed elsewhere.
int launch_cmvn_rows(const float* in, long long rows, const float* cmvn_mean, const float* cmvn_std, float* out, hipStream_t stream);

// y[k] = sum_m x[m] * taps[half_len + k*down - m*up] for k < n_out (zero-phase polyphase FIR; `up`/`down`
// in lowest terms, taps [2*half_len+1] on the device with gain `up`).
int launch_resample(const float* x, long long n_in, int up, int down, const float* taps, int half_len, float* y,
                    long long n_out, hipStream_t stream);

// Output sample k of the resampler from the input history x[0 .. n_in) and the taps hs (LDS on the device): the input window clamped
// at both ends of the history (zero padding), taps in ascending m, one fmaf each.  The ONE copy of this sum: resample_kernel, the
// resampling prologue of fbank_cmvn_sr_kernel and the streaming output resampler (pcm.hip: ss_pcm_emit and its host twin) give the
// same bits for the same (x, n_in, k) -- fmaf is correctly rounded on both sides.  X is anything that answers x[m] with a float for
// m in [0, n_in): a pointer, or a history that lies in two pieces (pcm.hpp).
template <class X>
__host__ __device__ __forceinline__ float resample_sample(X x, long long n_in, int up, int down, const float* hs, int half,
                                                          long long k) {
  const long long c = k * down;
  long long m_lo = c - half;                          // ceil((c - half) / up), clamped at 0
  m_lo = m_lo <= 0 ? 0 : (m_lo + up - 1) / up;
  long long m_hi = (c + half) / up;
  if (m_hi > n_in - 1) m_hi = n_in - 1;
  float acc = 0.f;
  for (long long m = m_lo; m <= m_hi; ++m) acc = fmaf(x[m], hs[half + (int)(c - m * up)], acc);
  return acc;
}

// One session of launch_fbank_cmvn_sr (a device table of these): rows first .. first + n_rows - 1 of the fbank of the source-rate
// history pcm[0 .. n_in) resampled by up / down (lowest terms; taps [2 * half + 1] on the device, unused when up == down), to feat
// (n_rows rows of 80).
struct FbankSrSeg {
  const float* pcm;
  const float* taps;
  float* feat;
  int n_in, up, down, half, first, n_rows;
};

// Host only: the fbank rows n_in source samples resample to -- n16 = ceil(n_in * up / down), 1 + (n16 - 400) / 160 -- and how many
// of them are FINAL: the largest F whose last sample 160 (F - 1) + 399 has its whole FIR window inside the history,
// ((160 (F - 1) + 399) * down + half_len) / up <= n_in - 1 (the kernel's m_hi before its clamp).  Later rows still see the zero
// padding and change when more audio arrives.  SS_ERR_ARG: up or down below 1, a negative half_len or n_in, taps that do not fit
// the workgroup's LDS beside the row's arrays, a history past the int range of 16-kHz sample indices.
int fbank_sr_rows(long long n_in, int up, int down, int half_len, int* n_rows, int* n_final);

// Ragged batch of sessions at their own rates (fbank.hip, fbank_cmvn_sr_kernel): segs [nseg] on the device, max_rows the largest
// n_rows, max_taps the largest 2 * half + 1 of the segments that resample (0: none does).  Every segment must have passed
// fbank_sr_rows and ask for rows below its n_rows: the kernel reads pcm[0 .. n_in) and nothing else.
int launch_fbank_cmvn_sr(const FbankSrSeg* segs, int nseg, int max_rows, int max_taps, float pcm_scale, const float* window,
                         const float* melw, const FbankTables& tabs, const float* cmvn_mean, const float* cmvn_std,
                         hipStream_t stream);

}  // namespace ss
