// Head-averaged attention probabilities with row arg-max and row statistics (see attn_probs.hpp).
//
// Workgroup = (16 answered query rows, segment), 4 wave64.  Scores are the S^T = K . Q^T tiles of attention_mfma_kernel on
// v_mfma_f32_16x16x4_f32: A = 16 key rows (lane (r, g) reads K[key r][16 kk + 4 g .. + 3]), B = the query rows held in registers,
// and lane (r = query, g) ends up with the scores of keys 4 g .. 4 g + 3 of the 16-key tile -- a query's row lives in the four lanes
// {r, r + 16, r + 32, r + 48}.  Every score is one k-ordered fmaf chain over its own 64 products, so it does not depend on which
// tile row or which launch it is computed in, and the two passes below get the same bits for it.
//   Pass 1: wave w owns heads w and w + 4 and walks ALL keys in 16-key tiles, ascending; the running (max, sum) of a (row, head)
//           is cut once per tile.  The results go to LDS as (max, 1 / sum).
//   Pass 2: wave w owns the 16-key tiles w, w + 4, ... and recomputes their scores for every head, ascending; the heads' normalised
//           probabilities are summed in registers in head order, the tile of P is written, and the row's arg-max and centre of mass
//           are folded per lane, then over the row's four lanes and the four waves (fixed order).
// Nothing of size [rows][k_len][H] leaves the chip: recomputing 2 x 64 MACs per (row, key, head) is cheaper than parking them.
#include "attn_probs.hpp"

#include <climits>

namespace ss {

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;
constexpr int AP_QB = 16;     // query rows per workgroup
constexpr int AP_KT = 16;     // keys per MFMA tile
constexpr int AP_DH = 64;     // head dim

// scores of one (16-key tile, head): s[e] = q_{row r} . k_{j0 + 4 g + e} (unscaled)
__device__ __forceinline__ f32x4 score_tile(const float* krow, bool k_ok, const f32x4 (&q)[4], int g) {
  f32x4 s = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    f32x4 kf = {0.f, 0.f, 0.f, 0.f};
    if (k_ok) kf = *reinterpret_cast<const f32x4*>(krow + 16 * kk + 4 * g);
#pragma unroll
    for (int e = 0; e < 4; ++e) s = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[e], q[kk][e], s, 0, 0, 0);
  }
  return s;
}

// (value, index) arg-max merge: the larger value, the lower index of a tie
__device__ __forceinline__ void peak_merge(float& v, int& i, float v2, int i2) {
  if (v2 > v || (v2 == v && i2 < i)) { v = v2; i = i2; }
}

}  // namespace

__global__ __launch_bounds__(256) void attention_probs_kernel(AttnProbsArgs p) {
  const int z = blockIdx.y;
  const int* sg = p.segs + 4 * z;
  const int q_len = sg[1], k_len = sg[3];
  const int qf = p.q_first[z];
  const int i0 = qf + (int)blockIdx.x * AP_QB;
  if (k_len <= 0 || qf < 0 || i0 >= q_len) return;             // block-uniform
  const float* Q = p.Q + (size_t)sg[0] * p.ldq;
  const float* K = p.K + (size_t)sg[2] * p.ldk;
  __shared__ float Ms[ATTN_PROBS_MAX_H][AP_QB], Is[ATTN_PROBS_MAX_H][AP_QB];     // soft-max maximum and 1 / sum of (head, row)
  __shared__ float pk_v[4][AP_QB], pk_c[4][AP_QB];
  __shared__ int pk_i[4][AP_QB];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int r = lane & 15, g = lane >> 4;
  const int iq = i0 + r;
  const bool q_ok = iq < q_len;
  const float* qrow = Q + (size_t)(q_ok ? iq : i0) * p.ldq;

  // ---- pass 1: soft-max statistics of heads wave, wave + 4 ----
  {
    f32x4 qa[2][4];
    float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f};
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int h = wave + 4 * hh;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        qa[hh][kk] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (q_ok && h < p.H) qa[hh][kk] = *reinterpret_cast<const f32x4*>(qrow + h * AP_DH + 16 * kk + 4 * g);
      }
    }
    for (int j0 = 0; j0 < k_len; j0 += AP_KT) {
      const bool k_ok = j0 + r < k_len;
      const float* krow = K + (size_t)(k_ok ? j0 + r : 0) * p.ldk;
#pragma unroll
      for (int hh = 0; hh < 2; ++hh) {
        const int h = wave + 4 * hh;
        if (h >= p.H) continue;                                   // wave-uniform
        f32x4 s = score_tile(krow + h * AP_DH, k_ok, qa[hh], g);
        float mt = -INFINITY;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s[e] = (j0 + 4 * g + e < k_len) ? __fmul_rn(s[e], p.scale) : -INFINITY;
          mt = fmaxf(mt, s[e]);
        }
        mt = fmaxf(mt, __shfl_xor(mt, 16, 64));
        mt = fmaxf(mt, __shfl_xor(mt, 32, 64));                   // finite: key j0 exists
        const float mn = fmaxf(m[hh], mt);
        float ls = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e) ls += expf(__fsub_rn(s[e], mn));            // expf(-inf) = 0 for the keys past k_len
        ls += __shfl_xor(ls, 16, 64);
        ls += __shfl_xor(ls, 32, 64);
        l[hh] = __fadd_rn(__fmul_rn(l[hh], expf(__fsub_rn(m[hh], mn))), ls);     // first tile: 0 * expf(-inf) = 0
        m[hh] = mn;
      }
    }
#pragma unroll
    for (int hh = 0; hh < 2; ++hh) {
      const int h = wave + 4 * hh;
      if (h < p.H && g == 0) { Ms[h][r] = m[hh]; Is[h][r] = 1.0f / l[hh]; }
    }
  }
  __syncthreads();

  // ---- pass 2: P, arg-max, centre of mass over the 16-key tiles wave, wave + 4, ... ----
  f32x4 qh[ATTN_PROBS_MAX_H][4];
  float mr[ATTN_PROBS_MAX_H], ir[ATTN_PROBS_MAX_H];
#pragma unroll
  for (int h = 0; h < ATTN_PROBS_MAX_H; ++h) {
    mr[h] = 0.f; ir[h] = 0.f;
    if (h < p.H) { mr[h] = Ms[h][r]; ir[h] = Is[h][r]; }
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      qh[h][kk] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (q_ok && h < p.H) qh[h][kk] = *reinterpret_cast<const f32x4*>(qrow + h * AP_DH + 16 * kk + 4 * g);
    }
  }
  const float inv_h = 1.0f / (float)p.H;
  float* prow = (p.P && q_ok) ? p.P + p.p_off[z] + (long long)(iq - qf) * k_len : nullptr;
  float best_v = -1.f, cen = 0.f;
  int best_i = INT_MAX;
  for (int j0 = AP_KT * wave; j0 < k_len; j0 += 4 * AP_KT) {
    const bool k_ok = j0 + r < k_len;
    const float* krow = K + (size_t)(k_ok ? j0 + r : 0) * p.ldk;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int h = 0; h < ATTN_PROBS_MAX_H; ++h) {
      if (h >= p.H) continue;                                     // uniform
      const f32x4 s = score_tile(krow + h * AP_DH, k_ok, qh[h], g);
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float pe = __fmul_rn(expf(__fsub_rn(__fmul_rn(s[e], p.scale), mr[h])), ir[h]);
        acc[e] = __fadd_rn(acc[e], pe);
      }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int j = j0 + 4 * g + e;
      if (j < k_len) {
        const float pv = __fmul_rn(acc[e], inv_h);
        if (prow) prow[j] = pv;
        if (pv > best_v) { best_v = pv; best_i = j; }              // ascending j per lane: the first maximum stays
        cen = __fadd_rn(cen, __fmul_rn((float)j, pv));
      }
    }
  }
  // the row's four lanes (symmetric exchanges: every lane of the row ends with the same bits), then the four waves in order
#pragma unroll
  for (int d = 16; d <= 32; d <<= 1) {
    const float v2 = __shfl_xor(best_v, d, 64);
    const int i2 = __shfl_xor(best_i, d, 64);
    peak_merge(best_v, best_i, v2, i2);
    cen = __fadd_rn(cen, __shfl_xor(cen, d, 64));
  }
  if (g == 0) { pk_v[wave][r] = best_v; pk_i[wave][r] = best_i; pk_c[wave][r] = cen; }
  __syncthreads();
  if (t < AP_QB && i0 + t < q_len) {
    float v = pk_v[0][t], c = pk_c[0][t];
    int i = pk_i[0][t];
#pragma unroll
    for (int w = 1; w < 4; ++w) {
      peak_merge(v, i, pk_v[w][t], pk_i[w][t]);
      c = __fadd_rn(c, pk_c[w][t]);
    }
    const int o = p.row_off[z] + (i0 + t - qf);
    p.peak[o] = i;
    p.stat[2 * (size_t)o] = v;
    p.stat[2 * (size_t)o + 1] = c;
  }
}

int launch_attention_probs(const AttnProbsArgs& a, hipStream_t stream) {
  if (a.nseg < 0 || a.max_rows < 0) return SS_ERR_ARG;
  if (a.nseg == 0 || a.max_rows == 0) return SS_OK;
  if (!a.Q || !a.K || !a.segs || !a.q_first || !a.row_off || !a.peak || !a.stat || (a.P && !a.p_off)) return SS_ERR_ARG;
  if (a.H < 1 || a.H > ATTN_PROBS_MAX_H || ((a.ldq | a.ldk) & 3) || a.ldq < a.H * AP_DH || a.ldk < a.H * AP_DH) return SS_ERR_ARG;
  if (a.nseg > 65535) return SS_ERR_ARG;                          // (the grid's y extent)
  hipLaunchKernelGGL(attention_probs_kernel, dim3(cdiv(a.max_rows, AP_QB), a.nseg, 1), dim3(256), 0, stream, a);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

}  // namespace ss
