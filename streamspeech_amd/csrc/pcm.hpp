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

}  // namespace pcm
}  // namespace ss
