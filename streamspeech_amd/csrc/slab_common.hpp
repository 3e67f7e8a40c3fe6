// Device code shared by the persistent "slab" conv kernels of the vocoder (conv_slab.hip: conv_slab / conv_pair, resblock.hip,
// conv_c16.hip, conv_c32.hip, conv_c64.hip, conv_c64w.hip): the segment walk and the GemmArgs epilogue.  Each kernel's staging and
// contraction is its own; only the code around them lives here.  Everything is force-inlined into the kernels.
#pragma once
#include "gemm.hpp"

namespace ss {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// Segment walk of a packed batch: blocks of `bm` output rows, numbered utterance by utterance (a block never straddles two
// utterances, so validity is uniform per block) and visited in ascending order by each workgroup.  The constructor builds the
// block prefix table s_blk[s] = first block of segment s, s_blk[nseg] = total, in LDS (nseg + 1 ints) on thread 0; the CALLER
// issues the barrier before nblocks() / locate() (resblock.hip shares it with its own LDS set-up).  Unsegmented (p.nseg == 0):
// one segment of p.M rows.
template <class P>
struct SlabWalk {
  const P& p;
  int* const s_blk;
  const int bm;
  int seg = 0, seg_lo = 0, seg_hi = 0, m0 = 0;   // block located last: its segment, the segment's rows [seg_lo, seg_hi), first row

  __device__ __forceinline__ SlabWalk(const P& p_, int* s_blk_, int bm_) : p(p_), s_blk(s_blk_), bm(bm_) {
    const int nseg = p.nseg > 0 ? p.nseg : 1;
    if (threadIdx.x == 0) {
      int acc = 0;
      for (int s = 0; s < nseg; ++s) {
        s_blk[s] = acc;
        const int len = p.nseg > 0 ? p.segs[4 * s + 1] : p.M;
        acc += (len + bm - 1) / bm;
      }
      s_blk[nseg] = acc;
    }
  }
  __device__ __forceinline__ int nblocks() const { return s_blk[p.nseg > 0 ? p.nseg : 1]; }
  // unseg_len: the rows of the unsegmented launch's one segment (p.in_len for the GemmArgs kernels, p.M for resblock)
  __device__ __forceinline__ void locate(int blk, int unseg_len) {
    while (blk >= s_blk[seg + 1]) ++seg;
    seg_lo = p.nseg > 0 ? p.segs[4 * seg] : 0;
    seg_hi = seg_lo + (p.nseg > 0 ? p.segs[4 * seg + 1] : unseg_len);
    m0 = seg_lo + (blk - s_blk[seg]) * bm;      // first output row (packed coordinates)
  }
};

// The tail of every slab epilogue on one float4 (4 consecutive channels of one row): the MRF accumulate R2, then the mean div.
// rr2() yields this row's R2 operand and is called only when p.R2 is set: the preloading kernels hand over the value they loaded
// before the math, the others load it here, where they always did.
template <class P, class R2Op>
__device__ __forceinline__ f32x4 slab_epi_tail(const P& p, f32x4 v, R2Op rr2) {
  if (p.R2) {
    const f32x4 r2 = rr2();
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = r2[e] + v[e];
  }
  if (p.div > 0.f) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] / p.div;
  }
  return v;
}

// GemmArgs epilogue of the conv_c16 / c32 / c64 / Winograd kernels: bias, epilogue leaky-ReLU (their only activation), alpha,
// residual R, then the tail.  bb is zero without a bias; rr / rr2 are preloaded by the caller before the math (read only when
// p.R / p.R2 is set).
__device__ __forceinline__ f32x4 slab_epi_apply(const GemmArgs& p, f32x4 v, const f32x4& bb, const f32x4& rr, const f32x4& rr2) {
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] += bb[e];
  if (p.act == ACT_LRELU) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * p.act_slope;
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] *= p.alpha;
  if (p.R) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] += rr[e];
  }
  return slab_epi_tail(p, v, [&] { return rr2; });
}

// The same epilogue over ALL the N float4 a lane holds (conv_c64 and the Winograd kernels), one operation at a time with every
// condition outside the loops: all the residuals R of the lane are requested in one batch before any is used, R2 (one conv in six) in
// a second batch into the same registers, and the caller stores only afterwards -- one dependent round trip to memory per operand
// and block, and no wait that covers a store (vmcnt counts stores too).  A lane still reads R / R2 of an element before it writes the
// element (the vocoder passes R == C and R2 == C).  Every element sees the operations of slab_epi_apply in the same order; alpha and
// R are ONE fma, which is what hipcc contracts slab_epi_apply's `v *= alpha; v += rr` to in these kernels (written out here so that
// the bits do not hang on the contraction surviving the restructuring).
// v[n]: accumulators in, results out; bias of v[n]: bb[n % NBB].  addr(q, n): element offset of float4 n in operand q (0: R, 1: R2).
template <int N, int NBB, class Addr>
__device__ __forceinline__ void slab_epi_batch(const GemmArgs& p, f32x4 (&v)[N], const f32x4 (&bb)[NBB], Addr addr) {
  f32x4 rr[N];
  if (p.R) {
#pragma unroll
    for (int n = 0; n < N; ++n) rr[n] = *reinterpret_cast<const f32x4*>(p.R + addr(0, n));
  }
#pragma unroll
  for (int n = 0; n < N; ++n) v[n] += bb[n % NBB];
  if (p.act == ACT_LRELU) {
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[n][e] = v[n][e] > 0.f ? v[n][e] : v[n][e] * p.act_slope;
  }
  if (p.R) {
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[n][e] = __builtin_fmaf(v[n][e], p.alpha, rr[n][e]);
  } else {
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] *= p.alpha;
  }
  if (p.R2) {
#pragma unroll
    for (int n = 0; n < N; ++n) rr[n] = *reinterpret_cast<const f32x4*>(p.R2 + addr(1, n));
#pragma unroll
    for (int n = 0; n < N; ++n) v[n] = rr[n] + v[n];
  }
  if (p.div > 0.f) {
#pragma unroll
    for (int n = 0; n < N; ++n)
#pragma unroll
      for (int e = 0; e < 4; ++e) v[n][e] = v[n][e] / p.div;
  }
}

// Store of row m, columns n .. n + 3: C, and with TWIN the optional pre-activated twin C2 = leaky_relu(C, c2_slope) for a consumer
// that cannot activate while staging.
template <bool TWIN = true, class P>
__device__ __forceinline__ void slab_epi_store(const P& p, int m, int n, f32x4 v) {
  *reinterpret_cast<f32x4*>(p.C + (size_t)m * p.ldc + n) = v;
  if (TWIN && p.C2) {
    f32x4 w2;
#pragma unroll
    for (int e = 0; e < 4; ++e) w2[e] = v[e] > 0.f ? v[e] : v[e] * p.c2_slope;
    *reinterpret_cast<f32x4*>(p.C2 + (size_t)m * p.ldc2 + n) = w2;
  }
}

}  // namespace ss
