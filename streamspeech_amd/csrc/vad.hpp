// Endpointing of live PCM streams (vad.hip; include/streamspeech_hip.h, "Endpointing"): the arithmetic of the energy scan, ONE inline
// function per step, called by the kernel and by the host twin alike, so the CPU suite pins the arithmetic and the GPU suite pins
// kernel == host bit for bit.  For that to hold there is no libm call here but fmaf (no logarithm: every threshold is a linear power
// ratio the caller converted from dB once), the summation order is fixed (lane-strided partial sums, then one reduction tree), and
// contraction is off, so the only fused multiply-adds are the ones spelled fmaf.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/streamspeech_hip.h"
#include "common.hpp"

namespace ss {
namespace vad {

constexpr int kLanes = 64;                        // partial sums of a frame: the lanes of one wave

// Lane `lane`'s share of a frame's first pass: x[lane] + x[lane + 64] + ... in ascending order.
__host__ __device__ inline float lane_sum(const float* x, int W, int lane) {
#pragma clang fp contract(off)
  float acc = 0.0f;
  for (int i = lane; i < W; i += kLanes) acc += x[i];
  return acc;
}

// Lane `lane`'s share of the second pass: the squares of the deviations from the mean m, one fmaf each, in the same order.
__host__ __device__ inline float lane_sq(const float* x, int W, int lane, float m) {
#pragma clang fp contract(off)
  float acc = 0.0f;
  for (int i = lane; i < W; i += kLanes) {
    const float d = x[i] - m;
    acc = fmaf(d, d, acc);
  }
  return acc;
}

// sum * (1 / W): the mean of the first pass, the power of the second.  inv_w is 1.0f / (float)W, computed once on the host.
__host__ __device__ inline float scaled(float sum, float inv_w) {
#pragma clang fp contract(off)
  return sum * inv_w;
}

// The reduction tree of the 64 partial sums as the wave runs it (v += shfl_xor(v, o), o = 32 .. 1: every lane ends with lane 0's sum,
// float addition being commutative).
inline float tree_host(float* p) {
  for (int o = kLanes / 2; o >= 1; o >>= 1)
    for (int l = 0; l < o; ++l) p[l] = p[l] + p[l + o];
  return p[0];
}

// P of one frame on the host: the kernel's two passes, lane by lane.
inline float frame_power_host(const float* x, int W, float inv_w) {
  float p[kLanes];
  for (int l = 0; l < kLanes; ++l) p[l] = lane_sum(x, W, l);
  const float m = scaled(tree_host(p), inv_w);
  for (int l = 0; l < kLanes; ++l) p[l] = lane_sq(x, W, l, m);
  return scaled(tree_host(p), inv_w);
}

__host__ __device__ inline void result_init(ss_vad_result& r, const ss_vad_seg& sg, const ss_vad_state& st) {
  r.consumed = sg.first_frame;
  r.start_frame = -1;
  r.cut_sample = -1;
  r.last_speech = st.last_speech;
  r.events = 0;
  r.mode = st.mode;
}

// Frame j with power P through the noise floor, the decision and the state machine.  -> true when the scan stops behind this frame.
__host__ __device__ inline bool step(ss_vad_state& st, ss_vad_result& r, const ss_vad_seg& sg, int64_t j, float P) {
#pragma clang fp contract(off)
  bool speech = false;
  if (j == 0) {
    st.floor = sg.p_min > P ? sg.p_min : P;
  } else {
    const float rel = st.floor * sg.snr;
    const float thr = sg.p_abs > rel ? sg.p_abs : rel;
    speech = P > thr;
    const float up = speech ? st.floor : st.floor * sg.rise;
    const float lo = P < up ? P : up;
    st.floor = sg.p_min > lo ? sg.p_min : lo;
  }
  bool stop = false;
  if (st.mode == SS_VAD_IDLE) {
    if (speech) {
      if (st.run == 0) st.onset = j;
      ++st.run;
      if (st.run >= sg.min_speech) {
        r.events |= SS_VAD_START;
        r.start_frame = st.onset;
        st.mode = SS_VAD_SPEECH;
        st.utt_first_frame = st.onset;
        st.last_speech = j;
        st.run = 0;
      }
    } else {
      st.run = 0;
    }
  } else if (speech) {
    st.last_speech = j;
    st.run = 0;
  } else {
    ++st.run;
  }
  if (st.mode == SS_VAD_SPEECH) {
    if (st.run >= sg.end_silence) {
      r.events |= SS_VAD_END;
      r.cut_sample = (st.last_speech + 1 + sg.post_roll) * (int64_t)sg.H + (sg.W - sg.H);
      st.mode = SS_VAD_IDLE;
      st.run = 0;
      stop = true;
    } else if (j + 1 - st.utt_first_frame >= sg.max_frames) {
      r.events |= SS_VAD_FORCED;
      r.cut_sample = (j + 1) * (int64_t)sg.H + (sg.W - sg.H);
      st.utt_first_frame = j + 1;
      st.last_speech = j;
      st.run = 0;
      stop = true;
    }
  }
  r.consumed = j + 1;
  r.last_speech = st.last_speech;
  r.mode = st.mode;
  return stop;
}

}  // namespace vad
}  // namespace ss
