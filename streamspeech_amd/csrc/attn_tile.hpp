// Device-only pieces of the attention kernels (attention.hip): the blocks that the paired kernels share, each written once.
// Everything is __forceinline__ -- a kernel built from these compiles to what its hand-inlined text compiled to.
//
// Fragment algebra of the MFMA pieces (v_mfma_f32_16x16x4_f32; C/D layout: col = lane&15, row = 4*(lane>>4) + reg; lane = (r, g)):
//   S^T = K . Q^T : A = K rows (lane (r,g) reads K[key r][16kk+4g .. +3] with one ds_read_b128 --
//     MFMA e then contracts d = {16kk+4g'+e}, a permutation of d shared with the Q operand),
//     B = Q rows held in registers.  The tile comes out as lane (r = query, g) holding the scores of
//     keys 4g..4g+3: a query's row lives in the 4 lanes {r, r+16, r+32, r+48} -> row max / sum are
//     2 shuffles, no LDS.
//   O^T = V^T . P^T : B = P^T is EXACTLY what the lane already holds (MFMA e takes keys {4g'+e}),
//     A = V^T[d = r][keys 4g..4g+3] is one ds_read_b128 from the transposed V tile.  The output
//     comes out as lane (r = query, g) holding d = 16dt+4g..+3 -> float4 stores.
#pragma once
#include "attention.hpp"

namespace ss {

constexpr int KT = 64;              // keys per tile
constexpr int DH = 64;              // head dim
constexpr int MQ = 64;              // queries per workgroup of the 64-query MFMA kernels
constexpr int LDT = 68;             // padded LDS row (floats): 17 sixteen-byte slots -> conflict-free b128 fragments
constexpr int LDG = 36;             // per-wave G patch row stride
constexpr int Q16_LDO = 68;         // padded row of the cross-wave output sum of the 16-query kernels

using f32x4 = __attribute__((ext_vector_type(4))) float;

// Ragged batch: rebases the workgroup (blockIdx.z = segment, blockIdx.x = tile of rows_per_wg query rows) onto its utterance.
// false: the segment has no query row for this workgroup.
__device__ __forceinline__ bool seg_rebase(AttnArgs& p, int rows_per_wg, bool relpos) {
  const int* sg = p.segs + 4 * blockIdx.z;
  p.Tq = sg[1]; p.Tk = sg[3];
  if (p.seg_tail) p.k_mask_tail = p.seg_tail[blockIdx.z];
  if ((int)blockIdx.x * rows_per_wg >= p.Tq) return false;
  p.Q += (size_t)sg[0] * p.ldq; p.O += (size_t)sg[0] * p.ldo;
  p.K += (size_t)sg[2] * p.ldk; p.V += (size_t)sg[2] * p.ldv;
  if (relpos) p.P += (size_t)(p.p_tmax - p.Tk) * p.ldp;
  return true;
}

// first key hidden from absolute query position pos by the chunk mask (Tk: none)
__device__ __forceinline__ int chunk_bound(int Tk, int chunk, int pos) { return chunk > 0 ? min(Tk, (pos / chunk + 1) * chunk) : Tk; }

// K rows j0 .. j0+63 of head column hoff into Ks [key][d], V rows into Vt [d][key]; rows past Tk are zero
__device__ __forceinline__ void stage_kv_tile(float* Ks, float* Vt, const float* K, const float* V, int ldk, int ldv, int Tk, int j0,
                                              int hoff, int t) {
  for (int f = t; f < KT * (DH / 4); f += 256) {
    const int row = f >> 4, c4 = (f & 15) * 4;      // 16 threads per key row (256 contiguous bytes)
    const int j = j0 + row;
    f32x4 kv = {0.f, 0.f, 0.f, 0.f}, vv = kv;
    if (j < Tk) {
      kv = *reinterpret_cast<const f32x4*>(K + (size_t)j * ldk + hoff + c4);
      vv = *reinterpret_cast<const f32x4*>(V + (size_t)j * ldv + hoff + c4);
    }
    *reinterpret_cast<f32x4*>(Ks + row * LDT + c4) = kv;
#pragma unroll
    for (int c = 0; c < 4; ++c) Vt[(c4 + c) * LDT + row] = vv[c];
  }
}

// Online softmax of one 64-key tile on the S^T fragments, s[kt][e] = score(query r, key j0 + 16kt + 4g + e): mask (keys from lim on),
// scale, running max / sum over the query's 4 lanes; s becomes the tile's probabilities.  Returns the factor of the old running sums.
__device__ __forceinline__ float softmax_tile(f32x4 (&s)[4], int j0, int lim, float scale, int g, float& m_run, float& l_run) {
  float mt = -INFINITY;
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = j0 + kt * 16 + 4 * g + e;
      s[kt][e] = (j < lim) ? s[kt][e] * scale : -INFINITY;
      mt = fmaxf(mt, s[kt][e]);
    }
  mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
  mt = fmaxf(mt, __shfl_xor(mt, 32, 64));
  const float mn = fmaxf(m_run, mt);
  float corr = 1.f, ls = 0.f;
  if (mn > -INFINITY) {
    corr = (m_run > -INFINITY) ? expf(m_run - mn) : 0.f;
#pragma unroll
    for (int kt = 0; kt < 4; ++kt)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float pe = (s[kt][e] > -INFINITY) ? expf(s[kt][e] - mn) : 0.f;
        s[kt][e] = pe;
        ls += pe;
      }
  } else {
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  ls += __shfl_xor(ls, 16, 64);
  ls += __shfl_xor(ls, 32, 64);
  l_run = l_run * corr + ls;
  m_run = mn;
  return corr;
}

// O^T = O^T corr + V^T . P^T -- the tile's product in a FRESH accumulator (a 64-key chain), then one add into the running sum:
// accumulating straight into o made one chain over all Tk keys, whose rounding grew with the utterance length (round 6:
// unit logits of an 11-s utterance sat 1.6x farther from float64 than the oracle's, of a 1.5-s one 0.8x)
__device__ __forceinline__ void pv_tile(f32x4 (&o)[4], const f32x4 (&s)[4], const float* Vt, int r, int g, float corr) {
  f32x4 ot[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) ot[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kt = 0; kt < 4; ++kt)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      const f32x4 vf = *reinterpret_cast<const f32x4*>(Vt + (dt * 16 + r) * LDT + kt * 16 + 4 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e) ot[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vf[e], s[kt][e], ot[dt], 0, 0, 0);
    }
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
#pragma unroll
    for (int e = 0; e < 4; ++e) o[dt][e] = o[dt][e] * corr + ot[dt][e];
}

// query row iq of O, head column hoff: o / l_run, lane (r, g) storing d = 16dt + 4g .. +3
__device__ __forceinline__ void store_rows(float* O, int ldo, int iq, int hoff, int g, const f32x4 (&o)[4], float l_run) {
  const float inv = 1.0f / l_run;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    f32x4 v = o[dt];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] *= inv;
    *reinterpret_cast<f32x4*>(O + (size_t)iq * ldo + hoff + 16 * dt + 4 * g) = v;
  }
}

// The two Q operands of the rel-pos score: quf[kk] = (q + u)[16kk + 4g .. +3], qvf = (q + v) likewise, of query row iq (zero q if !q_ok)
__device__ __forceinline__ void load_qu_qv(f32x4 (&quf)[4], f32x4 (&qvf)[4], const float* Q, int ldq, int iq, bool q_ok,
                                           const float* bias_u, const float* bias_v, int hoff, int g) {
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const int c = hoff + 16 * kk + 4 * g;
    f32x4 q = {0.f, 0.f, 0.f, 0.f};
    if (q_ok) q = *reinterpret_cast<const f32x4*>(Q + (size_t)iq * ldq + c);
    const f32x4 bu = *reinterpret_cast<const f32x4*>(bias_u + c);
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias_v + c);
#pragma unroll
    for (int e = 0; e < 4; ++e) { quf[kk][e] = q[e] + bu[e]; qvf[kk][e] = q[e] + bv[e]; }
  }
}

// The skewed read of the BD term through a wave's LDS patch Gs.  G[query r][window offset x]: x = 4g+e in ga, 16+4g+e in gb, the
// window starting at the table row of (last query of the 16, first key of the 16); BD for key 4g+e of query r is x = 15 - r + 4g + e
// (the rel_shift of the reference, never materialised beyond 16 x 32).  Wave-private: no barrier.
__device__ __forceinline__ f32x4 bd_skew(float* Gs, int r, int g, f32x4 ga, f32x4 gb) {
  *reinterpret_cast<f32x4*>(Gs + r * LDG + 4 * g) = ga;
  *reinterpret_cast<f32x4*>(Gs + r * LDG + 16 + 4 * g) = gb;
  const float* gr = Gs + r * LDG + 15 - r + 4 * g;
  return f32x4{gr[0], gr[1], gr[2], gr[3]};
}

// One (16-query, 64-key) rel-pos tile of a workgroup whose four waves are the four 16-KEY sub-tiles; keys jt .. jt+63, qlast = the
// absolute position of the tile's last query row, krow(j) / vrow(j) = row j of K / V (head 0).  Every operand fragment (K rows, the
// 31 table rows the sub-tile can touch, V columns) goes straight into registers in ONE round trip next to the caller's q + u / q + v,
// a wave issues 48 + 16 MFMAs, and the waves meet twice in LDS (softmax statistics in ms / ls, then the 16 x 64 output sum in osum:
// two barriers; a caller that loops puts one more between tiles).  Thread (query q = t>>4, columns d4 = 4 (t&15) .. +3) gets the
// tile's output sum normalised to the tile's own max: (acc, m_t, l_t).
template <class KRow, class VRow>
__device__ __forceinline__ void q16_tile(const f32x4 (&quf)[4], const f32x4 (&qvf)[4], KRow krow, VRow vrow, const float* P, int ldp,
                                         int Tk, int jt, int qlast, int lim, float scale, int hoff, float* Gs_all, float (*ms)[16],
                                         float (*ls)[16], float (*osum)[16][Q16_LDO], f32x4& acc, float& m_t, float& l_t) {
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int jb = jt + 16 * wave;                        // this wave's 16 keys
  f32x4 kf[4], pa[4], pb[4];
  float vv[4][4];
  const int pbase = jb - qlast + Tk - 1;                // table row of window row 0: key jb against the tile's last query
  const int pra = pbase + r, prb = pbase + 16 + r;
  const bool pa_ok = pra >= 0 && pra < 2 * Tk - 1, pb_ok = r < 15 && prb >= 0 && prb < 2 * Tk - 1;
  const bool k_ok = jb + r < Tk;
  const float* kr = krow(jb + r);
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    const int c = hoff + 16 * kk + 4 * g;
    kf[kk] = pa[kk] = pb[kk] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (k_ok) kf[kk] = *reinterpret_cast<const f32x4*>(kr + c);
    if (pa_ok) pa[kk] = *reinterpret_cast<const f32x4*>(P + (size_t)pra * ldp + c);
    if (pb_ok) pb[kk] = *reinterpret_cast<const f32x4*>(P + (size_t)prb * ldp + c);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int key = jb + 4 * g + e;
    const float* vr = vrow(key) + hoff + r;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) vv[dt][e] = key < Tk ? vr[dt * 16] : 0.f;
  }
  // ---- scores: AC = K (q + u)^T, BD through the skew patch ----
  f32x4 s = {0.f, 0.f, 0.f, 0.f}, ga = s, gb = s;
#pragma unroll
  for (int kk = 0; kk < 4; ++kk)
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      s = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[kk][e], quf[kk][e], s, 0, 0, 0);
      ga = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[kk][e], qvf[kk][e], ga, 0, 0, 0);
      gb = __builtin_amdgcn_mfma_f32_16x16x4f32(pb[kk][e], qvf[kk][e], gb, 0, 0, 0);
    }
  const f32x4 bd = bd_skew(Gs_all + wave * 16 * LDG, r, g, ga, gb);
  float mw = -INFINITY;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int j = jb + 4 * g + e;
    s[e] = (j < lim) ? (s[e] + bd[e]) * scale : -INFINITY;
    mw = fmaxf(mw, s[e]);
  }
  mw = fmaxf(mw, __shfl_xor(mw, 16, 64));
  mw = fmaxf(mw, __shfl_xor(mw, 32, 64));
  float pe[4], lw = 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) { pe[e] = (s[e] > -INFINITY) ? expf(s[e] - mw) : 0.f; lw += pe[e]; }
  lw += __shfl_xor(lw, 16, 64);
  lw += __shfl_xor(lw, 32, 64);
  if (g == 0) { ms[wave][r] = mw; ls[wave][r] = lw; }
  __syncthreads();
  {
    const float mt = fmaxf(fmaxf(ms[0][r], ms[1][r]), fmaxf(ms[2][r], ms[3][r]));
    const float fw = (mw > -INFINITY) ? expf(mw - mt) : 0.f;
#pragma unroll
    for (int e = 0; e < 4; ++e) pe[e] *= fw;
  }
  // ---- P V: D[query][d] += P[query][key] V[key][d] -- lane (r, g) ends up with queries 4 g + e', head column 16 dt + r ----
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) {
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int e = 0; e < 4; ++e) o = __builtin_amdgcn_mfma_f32_16x16x4f32(pe[e], vv[dt][e], o, 0, 0, 0);
#pragma unroll
    for (int e = 0; e < 4; ++e) osum[wave][4 * g + e][dt * 16 + r] = o[e];
  }
  __syncthreads();
  // ---- thread (query q, columns d4 .. d4 + 3): the four waves' sums in wave order, the tile's (m, l) ----
  const int q = t >> 4, d4 = (t & 15) * 4;
  acc = *reinterpret_cast<const f32x4*>(&osum[0][q][d4]);
#pragma unroll
  for (int w2 = 1; w2 < 4; ++w2) {
    const f32x4 o2 = *reinterpret_cast<const f32x4*>(&osum[w2][q][d4]);
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] += o2[e];
  }
  m_t = fmaxf(fmaxf(ms[0][q], ms[1][q]), fmaxf(ms[2][q], ms[3][q]));
  l_t = 0.f;
#pragma unroll
  for (int w2 = 0; w2 < 4; ++w2) l_t += (ms[w2][q] > -INFINITY) ? ls[w2][q] * expf(ms[w2][q] - m_t) : 0.f;
}

// Hand-off of a key split, after this workgroup parked its partial with sc1 (agent-scope) stores: wait for them, barrier, bump the
// (query tile, head) counter with a relaxed agent-scope atomic.  True in every thread of the workgroup whose bump completes s_eff
// arrivals -- it merges (sc1 loads: the per-XCD L2s are not coherent) and ends with split_reset.  Nobody waits for anybody.
__device__ __forceinline__ bool split_arrive(unsigned* cnt, int s_eff, int* s_last) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) *s_last = (__hip_atomic_fetch_add(cnt, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == (unsigned)(s_eff - 1)) ? 1 : 0;
  __syncthreads();
  return *s_last != 0;
}
// the counter back at zero: ready for the next launch of this context
__device__ __forceinline__ void split_reset(unsigned* cnt) {
  if (threadIdx.x == 0) __hip_atomic_store(cnt, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

}  // namespace ss
