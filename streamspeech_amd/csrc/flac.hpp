// FLAC ingest: what the host twin (flac_host.hip: ss_flac_restore_host) and the device stage (flac.hip) share -- the record checks,
// the accumulator-width rule and the per-sample arithmetic after the predictor.  All integer arithmetic wraps (unsigned adds and
// multiplies), so a corrupt stream gives the same bits on both sides instead of undefined behaviour.
#pragma once
#include <stdint.h>

#include "../../include/streamspeech_hip.h"

#if defined(__HIPCC__)
#define SS_FLAC_HD __host__ __device__ inline
#else
#define SS_FLAC_HD inline
#endif

namespace flac {

static_assert(sizeof(ss_flac_subframe) == 96, "record layout");
static_assert(sizeof(ss_flac_file) == 32, "file table layout");
static_assert(sizeof(ss_flac_info) == 64, "info layout");

constexpr int kMaxOrder = 32;

// a record the restore stage may follow without leaving its buffers: d_res / work [n_res], the file's n_out samples per channel
SS_FLAC_HD bool record_ok(const ss_flac_subframe& r, int64_t n_res, int32_t n_out) {
  return r.block_size >= 1 && r.res_offset >= 0 && r.res_offset <= n_res - r.block_size && r.sample_start >= 0 &&
         r.sample_start <= (int64_t)n_out - r.block_size && r.order <= kMaxOrder && (int32_t)r.order <= r.block_size &&
         r.wasted < 32 && r.shift < 32 && r.type <= SS_FLAC_LPC && r.assignment <= SS_FLAC_MID_SIDE;
}

SS_FLAC_HD int ceil_log2(int v) {
  int b = 0;
  while ((1 << b) < v) ++b;
  return b;
}

// libFLAC's rule: the sum of `order` products of a (bps - wasted)-bit sample and a precision-bit coefficient fits 32 bits
SS_FLAC_HD bool needs_wide(const ss_flac_subframe& r) {
  if (r.order == 0) return false;
  return (int)r.bps - (int)r.wasted + (int)r.precision + ceil_log2(r.order) > 32;
}

SS_FLAC_HD int32_t add_wrap(int32_t a, int32_t b) { return (int32_t)((uint32_t)a + (uint32_t)b); }
SS_FLAC_HD int32_t sub_wrap(int32_t a, int32_t b) { return (int32_t)((uint32_t)a - (uint32_t)b); }
SS_FLAC_HD int32_t shl_wrap(int32_t a, int s) { return (int32_t)((uint32_t)a << s); }

// the two channels of a stereo frame from its two restored subframes (after the wasted-bits shift)
SS_FLAC_HD void undo_stereo(int assignment, int32_t a, int32_t b, int32_t& l, int32_t& r) {
  switch (assignment) {
    case SS_FLAC_LEFT_SIDE: l = a; r = sub_wrap(a, b); break;
    case SS_FLAC_RIGHT_SIDE: l = add_wrap(a, b); r = b; break;
    case SS_FLAC_MID_SIDE: {
      const int32_t m = (int32_t)(((uint32_t)a << 1) | ((uint32_t)b & 1u));     // the bit the mid channel's halving dropped
      l = add_wrap(m, b) >> 1;
      r = sub_wrap(m, b) >> 1;
      break;
    }
    default: l = a; r = b; break;
  }
}

SS_FLAC_HD float scale_of(int bps) {                 // 2^-(bps-1), exact
  union { uint32_t u; float f; } v;
  v.u = (uint32_t)(127 - (bps - 1)) << 23;
  return v.f;
}

}  // namespace flac
