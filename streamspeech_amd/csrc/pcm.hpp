// Raw PCM in and out (pcm.hip): ONE inline function per conversion, called by the kernels and by the host entry points alike, so the
// CPU suite pins the arithmetic and the GPU suite pins kernel == host.  Every conversion is exact (an integer times a power of two,
// or a bit copy) except the two that round once: the f32 stereo mean's sum and the pack's product.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "common.hpp"

namespace ss {
namespace pcm {

enum : int { F32LE = 0, S16LE = 1, ULAW = 2, ALAW = 3, N_FMT = 4 };

// bytes of one sample of one channel
__host__ __device__ inline int sample_bytes(int fmt) { return fmt == F32LE ? 4 : fmt == S16LE ? 2 : 1; }

// G.711 mu-law code -> the 16-bit linear value (ITU-T G.711 expansion, 14-bit magnitude left-aligned as every decoder returns it)
__host__ __device__ inline int ulaw_to_s16(uint8_t c) {
  const int u = ~c & 0xFF;
  const int t = (((u & 15) << 3) + 0x84) << ((u & 0x70) >> 4);
  return (u & 0x80) ? 0x84 - t : t - 0x84;
}

// G.711 A-law code -> the 16-bit linear value
__host__ __device__ inline int alaw_to_s16(uint8_t c) {
  const int a = c ^ 0x55;
  const int s = (a & 0x70) >> 4;
  int t = (a & 15) << 4;
  t = s == 0 ? t + 8 : (t + 0x108) << (s - 1);
  return (a & 0x80) ? t : -t;
}

// an integer sample of |s| <= 2^15 -> [-1, 1): exact
__host__ __device__ inline float s16_to_float(int s) { return (float)s * (1.0f / 32768.0f); }
// the channel mean of two such samples: the sum has 17 bits, exact
__host__ __device__ inline float s16_pair_to_float(int l, int r) { return ((float)l + (float)r) * (1.0f / 65536.0f); }
// the channel mean of two floats: one rounding, in the sum
__host__ __device__ inline float f32_pair_to_float(float l, float r) { return (l + r) * 0.5f; }

__host__ __device__ inline float bits_to_float(uint32_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __uint_as_float(b);
#else
  float f;
  memcpy(&f, &b, 4);
  return f;
#endif
}
__host__ __device__ inline uint32_t float_to_bits(float f) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __float_as_uint(f);
#else
  uint32_t b;
  memcpy(&b, &f, 4);
  return b;
#endif
}

// One frame at byte pointer p (little-endian, channels interleaved) -> the BITS of the mono float32 sample.  Bits, because a mono f32le
// sample is copied, not computed with: NaN payloads, -0.0 and denormals arrive as they were sent.
__host__ __device__ inline uint32_t decode_frame_bits(const uint8_t* p, int fmt, int channels) {
  if (fmt == F32LE) {
    const uint32_t l = (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
    if (channels == 1) return l;
    const uint32_t r = (uint32_t)p[4] | ((uint32_t)p[5] << 8) | ((uint32_t)p[6] << 16) | ((uint32_t)p[7] << 24);
    return float_to_bits(f32_pair_to_float(bits_to_float(l), bits_to_float(r)));
  }
  int l, r = 0;
  if (fmt == S16LE) {
    l = (int16_t)(uint16_t)(p[0] | (p[1] << 8));
    if (channels == 2) r = (int16_t)(uint16_t)(p[2] | (p[3] << 8));
  } else if (fmt == ULAW) {
    l = ulaw_to_s16(p[0]);
    if (channels == 2) r = ulaw_to_s16(p[1]);
  } else {
    l = alaw_to_s16(p[0]);
    if (channels == 2) r = alaw_to_s16(p[1]);
  }
  return float_to_bits(channels == 1 ? s16_to_float(l) : s16_pair_to_float(l, r));
}

// float -> 16-bit PCM as frontend.write_wav rounds it: clip to [-1, 1], times 32767, round half to even; NaN -> 0
__host__ __device__ inline int16_t pack_s16(float x) {
  if (x != x) return 0;
  return (int16_t)(int)rintf(fminf(fmaxf(x, -1.0f), 1.0f) * 32767.0f);
}

// 16-bit linear value -> G.711 mu-law code (ITU-T G.711 compression of the 14-bit value s >> 2: magnitude clipped at 8159, biased
// by 33, segment = position of its leading one, four mantissa bits below it; all bits inverted).  Not "the nearest level": at the
// segment edges the standard's truncation picks the level below.  ulaw_from_s16(ulaw_to_s16(c)) == c except for 0x7F (negative
// zero), which encodes as 0xFF.
__host__ __device__ inline uint8_t ulaw_from_s16(int s) {
  int v = s >> 2;
  const int mask = v < 0 ? 0x7F : 0xFF;
  if (v < 0) v = -v;
  if (v > 8159) v = 8159;
  v += 33;                                            // 33 .. 8192: bit 5 at least is set
  int seg = 0;
  while ((v >> (seg + 6)) != 0) ++seg;                // 0 .. 8 (8 only for 8192, the clipped top)
  if (seg >= 8) return (uint8_t)(0x7F ^ mask);
  return (uint8_t)(((seg << 4) | ((v >> (seg + 1)) & 15)) ^ mask);
}

// 16-bit linear value -> G.711 A-law code (compression of the 13-bit value s >> 3; a negative value v is coded as -v - 1; even bits
// inverted).  alaw_from_s16(alaw_to_s16(c)) == c for every code.
__host__ __device__ inline uint8_t alaw_from_s16(int s) {
  int v = s >> 3;
  const int mask = v >= 0 ? 0xD5 : 0x55;
  if (v < 0) v = -v - 1;                              // 0 .. 4095
  int seg = 0;
  while ((v >> (seg + 5)) != 0) ++seg;                // 0 .. 7
  const int q = seg < 2 ? (v >> 1) & 15 : (v >> seg) & 15;
  return (uint8_t)(((seg << 4) | q) ^ mask);
}

// One float sample -> its sample_bytes(fmt) little-endian bytes in the low end of the result: f32le the float's bits (no clipping,
// NaN payloads as they are), s16le pack_s16, G.711 the compression of pack_s16's value.
__host__ __device__ inline uint32_t encode_sample(float x, int fmt) {
  if (fmt == F32LE) return float_to_bits(x);
  const int s = pack_s16(x);
  if (fmt == S16LE) return (uint32_t)(uint16_t)s;
  return fmt == ULAW ? ulaw_from_s16(s) : alaw_from_s16(s);
}

// A 16-kHz output history that lies in two pieces: samples [base, n_before) in the session's carry buffer, [n_before, ...) in the
// new tail.  resample_sample (fbank.hpp) reads it as x[m].
struct SplitHistory {
  const float* carry;
  const float* tail;
  long long base, n_before;
  __host__ __device__ inline float operator[](long long m) const { return m < n_before ? carry[m - base] : tail[m - n_before]; }
};

// Output samples of the streaming resampler that are settled after n input samples (ss_pcm_emit_count): all ceil(n up / down) once
// the utterance is finished, else those whose FIR window (k down + half) / up <= n - 1 lies inside the history.
__host__ __device__ inline long long emit_count(long long n, int up, int down, int half, int finished) {
  if (up == down) return n;
  if (finished) return (n * up + down - 1) / down;
  const long long top = n * up - 1 - half;
  return top < 0 ? 0 : top / down + 1;
}
// samples of history the next call may still read: (2 half) / up (0 when nothing is resampled)
__host__ __device__ inline long long emit_history(int up, int down, int half) { return up == down ? 0 : (2LL * half) / up; }

}  // namespace pcm
}  // namespace ss
