// Attention kernels (see attention.hpp for the arguments and launch_attention below for who takes a call).  All use the online
// (running max / running sum) softmax over 64-key tiles, so the [T,T] and [T,2T-1] score matrices the reference materialises
// (espnet_multihead_attention.py:186-196) never exist.  The seven kernels and the pieces of attn_tile.hpp each is built from:
//   attention_kernel<RELPOS>            VALU, 16 queries per workgroup, plain and rel-pos       seg_rebase
//   attention_decode_kernel<ANC>        <= 8 queries, one wave per key tile, no LDS tiles       (own prologue: the ancestry branch)
//   attention_mfma_kernel               plain, 64 queries x 64-key tiles in LDS                 seg_rebase, stage_kv_tile, softmax_tile,
//                                                                                               pv_tile, store_rows
//   attention_relpos_mfma_kernel<SPLIT> rel-pos, the same tiles + table window and skew patch   the five above + load_qu_qv, bd_skew,
//                                                                                               chunk_bound; SPLIT: split_arrive / _reset
//   attention_relpos_q16_kernel         rel-pos, <= 48 queries, one workgroup per key tile      load_qu_qv, chunk_bound, q16_tile,
//                                                                                               split_arrive / _reset
//   attention_pool_kernel               the same tile for many sessions, key tiles in a loop    load_qu_qv, chunk_bound, q16_tile
// What the paired kernels do NOT share stays in them: the park / merge layouts of the two key splits and the merge orders (the last
// arrival's two passes against the pool's running merge).
#include "attn_tile.hpp"

#include <algorithm>
#include <cstdlib>

namespace ss {

void attention_debug_no_mfma(int v) { dispatch_edit([v](Dispatch& d) { d.attn_no_mfma = v; }); }   // test hook: route plain attention to the VALU kernel
void attention_debug_q16(int v) { dispatch_edit([v](Dispatch& d) { d.attn_q16 = v; }); }          // test hook: 0 = the few-queries form off
void attention_debug_split(int v) { dispatch_edit([v](Dispatch& d) { d.attn_split = v; }); }   // test hook; SS_ATTN_NO_SPLIT=1: never split

constexpr int QB = 16;     // query rows per workgroup of the VALU kernel
constexpr int LDKS = DH + 1;

__device__ __forceinline__ float rdlane(float v, int l) {
  return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l));
}

// -------------------------------------------------------------------------------------------------
// VALU form, wavefront softmax.  Workgroup = 4 wave64 = 16 query rows of one head; wave w owns rows 4w..4w+3.  Keys are walked
// in tiles of 64 (lane = key).  K / V (and, for the rel-pos form, the 79 positional rows the
// 16x64 (query,key) pairs of the tile can touch) are staged in LDS; the query rows live in
// registers (lane d holds q[.,d]) and are broadcast with v_readlane, as are the probabilities
// for P.V (lane = output dim); max and sum are wave-wide shuffles.
// -------------------------------------------------------------------------------------------------
template <bool RELPOS>
__global__ __launch_bounds__(256) void attention_kernel(AttnArgs p) {
  if (p.nseg > 0 && !seg_rebase(p, QB, RELPOS)) return;
  __shared__ float Ks[KT * LDKS];
  __shared__ float Vs[KT * DH];
  __shared__ float Ps[RELPOS ? (KT + QB - 1) * LDKS : 1];

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int h = blockIdx.y;
  const int i0 = blockIdx.x * QB;
  const int hoff = h * DH;
  const int qoff = p.Tk - p.Tq;
  const int q0 = p.q0;               // absolute position of query row 0 (chunk mask / relative offsets)

  // query rows of this wave in registers: lane d holds element d
  float qu[4], qv[4];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int i = i0 + wave * 4 + rr;
    float q = (i < p.Tq) ? p.Q[(size_t)i * p.ldq + hoff + lane] : 0.f;
    if (RELPOS) {
      qu[rr] = q + p.bias_u[hoff + lane];
      qv[rr] = q + p.bias_v[hoff + lane];
    } else {
      qu[rr] = q;
      qv[rr] = 0.f;
    }
  }

  float m_run[4], l_run[4], acc[4];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) { m_run[rr] = -INFINITY; l_run[rr] = 0.f; acc[rr] = 0.f; }

  // last key any row of this block may see (block-uniform loop bound)
  int kmax = p.Tk - p.k_mask_tail;
  const int ilast = min(i0 + QB, p.Tq) - 1;
  if (p.causal) kmax = min(kmax, ilast + qoff + 1);
  if (p.chunk > 0) kmax = min(kmax, ((ilast + q0) / p.chunk + 1) * p.chunk);

  for (int j0 = 0; j0 < kmax; j0 += KT) {
    __syncthreads();  // previous tile fully consumed
    // stage K, V tiles: 64 rows x 16 float4
    for (int f = t; f < KT * (DH / 4); f += 256) {
      const int row = f >> 4, c4 = (f & 15) * 4;
      const int j = j0 + row;
      float4 kv = make_float4(0.f, 0.f, 0.f, 0.f), vv = kv;
      if (j < p.Tk) {
        kv = *reinterpret_cast<const float4*>(p.K + (size_t)j * p.ldk + hoff + c4);
        vv = *reinterpret_cast<const float4*>(p.V + (size_t)j * p.ldv + hoff + c4);
      }
      float* kd = Ks + row * LDKS + c4;
      kd[0] = kv.x; kd[1] = kv.y; kd[2] = kv.z; kd[3] = kv.w;
      *reinterpret_cast<float4*>(Vs + row * DH + c4) = vv;
    }
    if (RELPOS) {
      // local row lr <-> table row pbase + lr, pbase = j0 - (i0 + QB - 1) + Tk - 1
      const int pbase = j0 - (i0 + q0 + QB - 1) + p.Tk - 1;
      for (int f = t; f < (KT + QB - 1) * (DH / 4); f += 256) {
        const int row = f >> 4, c4 = (f & 15) * 4;
        const int pr = pbase + row;
        float4 pv = make_float4(0.f, 0.f, 0.f, 0.f);
        if (pr >= 0 && pr < 2 * p.Tk - 1)
          pv = *reinterpret_cast<const float4*>(p.P + (size_t)pr * p.ldp + hoff + c4);
        float* pd = Ps + row * LDKS + c4;
        pd[0] = pv.x; pd[1] = pv.y; pd[2] = pv.z; pd[3] = pv.w;
      }
    }
    __syncthreads();

    // scores: lane = key
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    const float* krow = Ks + lane * LDKS;
#pragma unroll 16
    for (int d = 0; d < DH; ++d) {
      const float kd = krow[d];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) s[rr] = fmaf(rdlane(qu[rr], d), kd, s[rr]);
    }
    if (RELPOS) {
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        // table row for (i, j): j - i + Tk - 1  ->  local row lane + (QB-1) - (wave*4+rr)
        const float* prow = Ps + (lane + (QB - 1) - (wave * 4 + rr)) * LDKS;
        float b = 0.f;
#pragma unroll 16
        for (int d = 0; d < DH; ++d) b = fmaf(rdlane(qv[rr], d), prow[d], b);
        s[rr] += b;
      }
    }

    const int j = j0 + lane;
    float pr[4];
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
      const int i = i0 + wave * 4 + rr;
      bool vis = (j < p.Tk - p.k_mask_tail) && (i < p.Tq);
      if (p.causal) vis = vis && (j <= i + qoff);
      if (p.chunk > 0) vis = vis && (j < ((i + q0) / p.chunk + 1) * p.chunk);
      const float sv = vis ? s[rr] * p.scale : -INFINITY;
      const float mt = wave_max(sv);
      const float mn = fmaxf(m_run[rr], mt);
      float pe = 0.f, corr = 1.f;
      if (mn > -INFINITY) {
        pe = vis ? expf(sv - mn) : 0.f;
        corr = (m_run[rr] > -INFINITY) ? expf(m_run[rr] - mn) : 0.f;
      }
      l_run[rr] = l_run[rr] * corr + wave_sum(pe);
      acc[rr] *= corr;
      m_run[rr] = mn;
      pr[rr] = pe;
    }
    // P.V : lane = output dim
#pragma unroll 16
    for (int jj = 0; jj < KT; ++jj) {
      const float vd = Vs[jj * DH + lane];
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) acc[rr] = fmaf(rdlane(pr[rr], jj), vd, acc[rr]);
    }
  }

#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int i = i0 + wave * 4 + rr;
    if (i < p.Tq) p.O[(size_t)i * p.ldo + hoff + lane] = acc[rr] / l_run[rr];
  }
}


// -------------------------------------------------------------------------------------------------
// Decode form (Tq <= 8, e.g. one new MT token against the KV cache): one wave64 per (query, head),
// no LDS, no barriers.  Scores: lane = key, the 64-d query is wave-uniform (scalar loads), each lane
// streams its key row (256 contiguous bytes).  P.V: lane = output dim, probabilities broadcast with
// v_readlane, V rows read coalesced.  Same online softmax as the tiled kernel.
// -------------------------------------------------------------------------------------------------
template <bool ANC>
__global__ __launch_bounds__(256) void attention_decode_kernel(AttnArgs p) {
  // 4 waves per (query, head): wave w takes key tiles w, w+4, ...; partial (max, sum, acc) merged in LDS
  const int* anc = nullptr;
  int k0 = 0;                        // ANC: position of the segment's first key in its slot rows (k_start)
  if (p.nseg > 0) {
    const int* sg = p.segs + 4 * blockIdx.z;
    p.Tq = sg[1]; p.Tk = sg[3];
    if (p.seg_tail) p.k_mask_tail = p.seg_tail[blockIdx.z];
    if ((int)blockIdx.x >= p.Tq) return;
    p.Q += (size_t)sg[0] * p.ldq; p.O += (size_t)sg[0] * p.ldo;
    if (ANC) {
      k0 = sg[2];
      anc = p.anc + (size_t)blockIdx.z * p.anc_ld + k0;
    } else {
      p.K += (size_t)sg[2] * p.ldk; p.V += (size_t)sg[2] * p.ldv;
    }
  }
  // row of key / value j: position j of the slot that holds it (ANC), else row j of the segment
  auto krow = [&](int j) -> size_t {
    if (!ANC) return (size_t)j;
    const int a = min((unsigned)anc[j], (unsigned)(p.anc_slots - 1));
    return (size_t)a * p.anc_ld + k0 + j;
  };
  __shared__ float part_m[4], part_l[4], part_acc[4][DH];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x, h = blockIdx.y;
  const int hoff = h * DH;
  const int qoff = p.Tk - p.Tq;
  const float* q = p.Q + (size_t)i * p.ldq + hoff;
  int kmax = p.Tk - p.k_mask_tail;
  if (p.causal) kmax = min(kmax, i + qoff + 1);
  if (p.chunk > 0) kmax = min(kmax, (i / p.chunk + 1) * p.chunk);
  float m_run = -INFINITY, l_run = 0.f, acc = 0.f;
  for (int j0 = wave * 64; j0 < kmax; j0 += 256) {
    const int j = j0 + lane;
    const bool vis = j < kmax;
    // The tile's V rows are requested BEFORE its scores are formed (their addresses do not depend on the scores), so the
    // kernel pays one memory latency per tile instead of two -- it is launched ~8 times per MT decode step, each a link
    // of a dependent chain.  Rows past the last visible key are clamped to it: their probability is exactly 0, and
    // fmaf(0, v, acc) == acc, so the sum is the one the 16-row groups of the earlier form produced.
    float vv[64];
#pragma unroll
    for (int u = 0; u < 64; ++u) vv[u] = p.V[krow(min(j0 + u, kmax - 1)) * p.ldv + hoff + lane];
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (vis) {
      const float4* kr = reinterpret_cast<const float4*>(p.K + krow(j) * p.ldk + hoff);
#pragma unroll
      for (int d4 = 0; d4 < DH / 4; ++d4) {
        const float4 kv = kr[d4];
        s0 = fmaf(q[4 * d4 + 0], kv.x, s0); s1 = fmaf(q[4 * d4 + 1], kv.y, s1);
        s2 = fmaf(q[4 * d4 + 2], kv.z, s2); s3 = fmaf(q[4 * d4 + 3], kv.w, s3);
      }
    }
    const float sv = vis ? ((s0 + s1) + (s2 + s3)) * p.scale : -INFINITY;
    const float mn = fmaxf(m_run, wave_max(sv));
    const float pe = vis ? expf(sv - mn) : 0.f;
    const float corr = (m_run > -INFINITY) ? expf(m_run - mn) : 0.f;
    l_run = l_run * corr + wave_sum(pe);
    acc *= corr;
    m_run = mn;
#pragma unroll
    for (int u = 0; u < 64; ++u) acc = fmaf(rdlane(pe, u), vv[u], acc);
  }
  if (lane == 0) { part_m[wave] = m_run; part_l[wave] = l_run; }
  part_acc[wave][lane] = acc;
  __syncthreads();
  if (wave == 0) {
    float mt = fmaxf(fmaxf(part_m[0], part_m[1]), fmaxf(part_m[2], part_m[3]));
    float l = 0.f, o = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float f = (part_m[w] > -INFINITY) ? expf(part_m[w] - mt) : 0.f;
      l += part_l[w] * f;
      o += part_acc[w][lane] * f;
    }
    p.O[(size_t)i * p.ldo + hoff + lane] = o / l;
  }
}

// -------------------------------------------------------------------------------------------------
// MFMA form (plain attention, Tq > 8): QK^T and PV on v_mfma_f32_16x16x4_f32, online softmax on the
// accumulator fragments.  Workgroup = 64 queries x 1 head (4 waves x 16 queries), 64-key tiles of K
// and V^T in LDS shared by the 4 waves; the fragment algebra is written down in attn_tile.hpp.
// Same arithmetic as the reference fairseq MHA (ctc_unity/modules/multihead_attention.py:544-760):
// fp32 scores, -inf masks (causal / key padding), softmax, PV; only the summation order differs.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attention_mfma_kernel(AttnArgs p) {
  if (p.nseg > 0 && !seg_rebase(p, MQ, false)) return;
  __shared__ __attribute__((aligned(16))) float Ks[KT * LDT];     // [key][d]
  __shared__ __attribute__((aligned(16))) float Vt[DH * LDT];     // [d][key]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int r = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, hoff = h * DH;
  const int i0 = blockIdx.x * MQ;
  const int qoff = p.Tk - p.Tq;
  const int iq = i0 + wave * 16 + r;                 // this lane's query row
  const bool q_ok = iq < p.Tq;

  f32x4 qf[4];                                        // Q[iq][16kk + 4g .. +3]
#pragma unroll
  for (int kk = 0; kk < 4; ++kk) {
    qf[kk] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (q_ok) qf[kk] = *reinterpret_cast<const f32x4*>(p.Q + (size_t)iq * p.ldq + hoff + 16 * kk + 4 * g);
  }
  f32x4 o[4];                                         // O^T fragments: d = 16dt + 4g + e for query r
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;

  int kmax = p.Tk - p.k_mask_tail;                    // block-uniform loop bound
  const int ilast = min(i0 + MQ, p.Tq) - 1;
  if (p.causal) kmax = min(kmax, ilast + qoff + 1);
  if (p.chunk > 0) kmax = min(kmax, (ilast / p.chunk + 1) * p.chunk);
  int lim = p.Tk - p.k_mask_tail;                     // this lane's own visibility bound
  if (p.causal) lim = min(lim, iq + qoff + 1);
  if (p.chunk > 0) lim = min(lim, (iq / p.chunk + 1) * p.chunk);
  if (!q_ok) lim = 0;

  for (int j0 = 0; j0 < kmax; j0 += KT) {
    __syncthreads();                                  // previous tile fully consumed
    stage_kv_tile(Ks, Vt, p.K, p.V, p.ldk, p.ldv, p.Tk, j0, hoff, t);
    __syncthreads();

    // S^T tiles: s[kt][e] = score(query iq, key j0 + 16kt + 4g + e)
    f32x4 s[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const f32x4 kf = *reinterpret_cast<const f32x4*>(Ks + (kt * 16 + r) * LDT + 16 * kk + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) s[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[e], qf[kk][e], s[kt], 0, 0, 0);
      }
    }
    const float corr = softmax_tile(s, j0, lim, p.scale, g, m_run, l_run);
    pv_tile(o, s, Vt, r, g, corr);
  }
  if (q_ok) store_rows(p.O, p.ldo, iq, hoff, g, o, l_run);
}

// -------------------------------------------------------------------------------------------------
// MFMA form of the Conformer's relative-position attention (espnet_multihead_attention.py:154-209):
//   score[i,j] = ((q_i+u).k_j + (q_i+v).p[j-i+T-1]) / 8, chunk mask, softmax, PV.
// AC = K.(Q+u)^T and PV are the tiles of attention_mfma_kernel.  BD is Toeplitz in (i, j): for a wave's
// 16 queries and a 16-key sub-tile only 31 table rows can occur, so G^T = Pwin.(Q+v)^T is computed for
// the 32-row window starting at the sub-tile's smallest offset (two more MFMA tiles) and the skewed
// read BD[i][j] = G[i][15 - (i - ib) + (j - jb)] goes through a 2.3 KB per-wave LDS patch (the
// rel_shift of the reference, never materialised beyond 16 x 32).  The projected table rows a
// (64 query x 64 key) block can touch (127) are staged in LDS next to the K and V^T tiles.
// -------------------------------------------------------------------------------------------------
constexpr int PWIN = 2 * KT;          // staged table rows (127 used, last one zero)
constexpr size_t kRelposLds = (size_t)(KT * LDT + DH * LDT + PWIN * LDT + 4 * 16 * LDG) * sizeof(float);

//
// SPLIT (single utterance, few query tiles): the key tiles are cut into p.ksplit groups of p.ktiles_per_split, one workgroup
// per (query tile, group, head) -- blockIdx.x = group * query_tiles + query_tile.  Each parks its un-normalised (o, m, l) in
// its register layout (5 b128 per thread, agent-scope sc1 stores), then bumps the (query tile, head) counter; the workgroup
// whose bump completes the count merges ALL groups in group order (so the result does not depend on who merges), writes O
// and zeroes the counter.  Same hand-off rules as conv_sk2: sc1 b128 stores -> vmcnt(0) -> barrier -> relaxed agent-scope
// atomic; sc1 loads on the other side (MI355X_MICROARCH.md: per-XCD L2s are not coherent).  Nobody waits for anybody.
template <bool SPLIT>
__global__ __launch_bounds__(256) void attention_relpos_mfma_kernel(AttnArgs p) {
  if (!SPLIT && p.nseg > 0 && !seg_rebase(p, MQ, true)) return;
  extern __shared__ __attribute__((aligned(16))) float smem_rp[];
  float* Ks = smem_rp;                  // [key][d]
  float* Vt = Ks + KT * LDT;            // [d][key]
  float* Ps = Vt + DH * LDT;            // [table row][d]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  float* Gs = Ps + PWIN * LDT + wave * 16 * LDG;
  const int r = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, hoff = h * DH;
  int qt = blockIdx.x, sp = 0;
  if (SPLIT) { const int nqt = gridDim.x / p.ksplit; sp = blockIdx.x / nqt; qt = blockIdx.x - sp * nqt; }
  const int i0 = qt * MQ;
  const int q0 = p.q0;
  const int iq = i0 + wave * 16 + r;                 // this lane's query row (relative to Q); absolute position q0 + iq
  const bool q_ok = iq < p.Tq;

  f32x4 quf[4], qvf[4];
  load_qu_qv(quf, qvf, p.Q, p.ldq, iq, q_ok, p.bias_u, p.bias_v, hoff, g);
  f32x4 o[4];
#pragma unroll
  for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m_run = -INFINITY, l_run = 0.f;

  const int kmax = chunk_bound(p.Tk, p.chunk, min(i0 + MQ, p.Tq) - 1 + q0);   // block-uniform loop bound
  const int lim = q_ok ? chunk_bound(p.Tk, p.chunk, iq + q0) : 0;               // this lane's own visibility bound
  int jbeg = 0, jend = kmax, s_eff = 1;
  if (SPLIT) {
    const int span = p.ktiles_per_split * KT;
    s_eff = (kmax + span - 1) / span;                // groups that hold a visible key of this query tile (chunk mask)
    if (sp >= s_eff) return;
    jbeg = sp * span;
    jend = min(kmax, jbeg + span);
  }

  for (int j0 = jbeg; j0 < jend; j0 += KT) {
    __syncthreads();
    stage_kv_tile(Ks, Vt, p.K, p.V, p.ldk, p.ldv, p.Tk, j0, hoff, t);
    {
      // local row lr <-> table row pbase + lr, pbase = j0 - (q0 + i0 + MQ - 1) + Tk - 1
      const int pbase = j0 - (q0 + i0 + MQ - 1) + p.Tk - 1;
      for (int f = t; f < PWIN * (DH / 4); f += 256) {
        const int row = f >> 4, c4 = (f & 15) * 4;
        const int pr = pbase + row;
        f32x4 pv = {0.f, 0.f, 0.f, 0.f};
        if (row < PWIN - 1 && pr >= 0 && pr < 2 * p.Tk - 1)
          pv = *reinterpret_cast<const f32x4*>(p.P + (size_t)pr * p.ldp + hoff + c4);
        *reinterpret_cast<f32x4*>(Ps + row * LDT + c4) = pv;
      }
    }
    __syncthreads();

    f32x4 s[4];
#pragma unroll
    for (int kt = 0; kt < 4; ++kt) {
      s[kt] = f32x4{0.f, 0.f, 0.f, 0.f};
      f32x4 ga = {0.f, 0.f, 0.f, 0.f}, gb = {0.f, 0.f, 0.f, 0.f};
      const int lrow0 = 16 * (kt - wave) + (MQ - 16);          // first window row of this (wave, sub-tile)
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        const f32x4 kf = *reinterpret_cast<const f32x4*>(Ks + (kt * 16 + r) * LDT + 16 * kk + 4 * g);
        const f32x4 pa = *reinterpret_cast<const f32x4*>(Ps + (lrow0 + r) * LDT + 16 * kk + 4 * g);
        const f32x4 pb = *reinterpret_cast<const f32x4*>(Ps + (lrow0 + 16 + r) * LDT + 16 * kk + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          s[kt] = __builtin_amdgcn_mfma_f32_16x16x4f32(kf[e], quf[kk][e], s[kt], 0, 0, 0);
          ga = __builtin_amdgcn_mfma_f32_16x16x4f32(pa[e], qvf[kk][e], ga, 0, 0, 0);
          gb = __builtin_amdgcn_mfma_f32_16x16x4f32(pb[e], qvf[kk][e], gb, 0, 0, 0);
        }
      }
      s[kt] += bd_skew(Gs, r, g, ga, gb);
    }
    const float corr = softmax_tile(s, j0, lim, p.scale, g, m_run, l_run);
    pv_tile(o, s, Vt, r, g, corr);
  }
  if (SPLIT && s_eff > 1) {
    using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
    const int slot0 = (qt * (int)gridDim.y + h) * p.ksplit;
    {
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(p.part + (size_t)(slot0 + sp) * ATTN_PART_FLOATS), 0, ATTN_PART_FLOATS * 4, 0x00020000);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        u32x4 v;
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __float_as_uint(o[dt][e]);
        __builtin_amdgcn_raw_buffer_store_b128(v, rs, (dt * 256 + t) * 16, 0, 16);      // aux 16 = sc1 (agent scope)
      }
      const u32x4 ml = {__float_as_uint(m_run), __float_as_uint(l_run), 0u, 0u};
      __builtin_amdgcn_raw_buffer_store_b128(ml, rs, (4 * 256 + t) * 16, 0, 16);
    }
    __shared__ int s_last;
    unsigned* cnt = p.cnt + qt * (int)gridDim.y + h;
    if (!split_arrive(cnt, s_eff, &s_last)) return;
    // ---- the last arrival merges every group, in group order ----
    float mx = -INFINITY;
    for (int g2 = 0; g2 < s_eff; ++g2) {
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(p.part + (size_t)(slot0 + g2) * ATTN_PART_FLOATS), 0, ATTN_PART_FLOATS * 4, 0x00020000);
      const u32x4 ml = __builtin_amdgcn_raw_buffer_load_b128(rs, (4 * 256 + t) * 16, 0, 16);
      mx = fmaxf(mx, __uint_as_float(ml[0]));
    }
    float lsum = 0.f;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int g2 = 0; g2 < s_eff; ++g2) {
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(p.part + (size_t)(slot0 + g2) * ATTN_PART_FLOATS), 0, ATTN_PART_FLOATS * 4, 0x00020000);
      u32x4 v[5];
#pragma unroll
      for (int dt = 0; dt < 5; ++dt) v[dt] = __builtin_amdgcn_raw_buffer_load_b128(rs, (dt * 256 + t) * 16, 0, 16);
      const float mg = __uint_as_float(v[4][0]);
      const float f = (mg > -INFINITY) ? expf(mg - mx) : 0.f;
      lsum += __uint_as_float(v[4][1]) * f;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int e = 0; e < 4; ++e) o[dt][e] += __uint_as_float(v[dt][e]) * f;
    }
    l_run = lsum;
    split_reset(cnt);
  }
  if (q_ok) store_rows(p.O, p.ldo, iq, hoff, g, o, l_run);
}

// -------------------------------------------------------------------------------------------------
// Rel-pos attention of a FEW query rows over all keys: the tail rows of the incremental streaming encoder (<= 48 per policy() call,
// 8-16 for the 320-ms agent; ss_encoder_stream_forward).  attention_relpos_mfma_kernel gives such a call one workgroup per (head, key
// split) whose four waves are four 16-query sub-tiles -- three of them empty -- and walks a 64-key tile through LDS (K, V^T and 127
// table rows staged, 192 MFMAs per wave and tile): 14 us per layer, all latency.  Here a workgroup is (16-query tile, 64-key tile,
// head) and its four waves are the four 16-KEY sub-tiles: every operand fragment (q + u, q + v, K rows, the 31 table rows the sub-tile
// can touch, V columns) is loaded straight into registers in ONE round trip, a wave issues 48 + 16 MFMAs, and the waves meet twice in
// LDS (softmax statistics, then the 16 x 64 output sum).  Same arithmetic per score as the tile kernel (the BD term through the per-wave
// skew patch); the softmax is normalised per key tile and merged in key-tile order by the last arriving workgroup of a (query tile,
// head) -- the hand-off protocol of the SPLIT form above.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attention_relpos_q16_kernel(AttnArgs p) {
  using u32x4 = __attribute__((ext_vector_type(4))) unsigned;
  __shared__ __attribute__((aligned(16))) float Gs_all[4 * 16 * LDG];
  __shared__ float ms[4][16], ls[4][16];
  __shared__ __attribute__((aligned(16))) float osum[4][16][Q16_LDO];
  __shared__ int s_last;
  const int t = threadIdx.x, lane = t & 63;
  const int r = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, hoff = h * DH;
  const int nqt = gridDim.x / p.ksplit;
  const int sp = blockIdx.x / nqt, qt = blockIdx.x - sp * nqt;
  const int i0 = qt * 16, q0 = p.q0;
  const int kmax = chunk_bound(p.Tk, p.chunk, min(i0 + 16, p.Tq) - 1 + q0);
  const int s_eff = (kmax + KT - 1) / KT;              // key tiles that hold a visible key of this query tile
  if (sp >= s_eff) return;
  const int iq = i0 + r;
  const bool q_ok = iq < p.Tq;
  const int lim = q_ok ? chunk_bound(p.Tk, p.chunk, iq + q0) : 0;

  f32x4 quf[4], qvf[4], acc;
  float m_run, l_run;
  load_qu_qv(quf, qvf, p.Q, p.ldq, iq, q_ok, p.bias_u, p.bias_v, hoff, g);
  q16_tile(quf, qvf, [&](int j) { return p.K + (size_t)j * p.ldk; }, [&](int j) { return p.V + (size_t)j * p.ldv; }, p.P, p.ldp, p.Tk,
           sp * KT, q0 + i0 + 15, lim, p.scale, hoff, Gs_all, ms, ls, osum, acc, m_run, l_run);
  const int q = t >> 4, d4 = (t & 15) * 4;              // this thread's (query, columns d4 .. d4 + 3) of the tile's output

  if (s_eff > 1) {
    const int slot0 = (qt * (int)gridDim.y + h) * p.ksplit;
    {
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(p.part + (size_t)(slot0 + sp) * ATTN_PART_FLOATS), 0, ATTN_PART_FLOATS * 4, 0x00020000);
      const u32x4 v = {__float_as_uint(acc[0]), __float_as_uint(acc[1]), __float_as_uint(acc[2]), __float_as_uint(acc[3])};
      __builtin_amdgcn_raw_buffer_store_b128(v, rs, (q * 64 + d4) * 4, 0, 16);          // aux 16 = sc1 (agent scope)
      if ((t & 15) == 0) {
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(m_run), rs, (1024 + q) * 4, 0, 16);
        __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(l_run), rs, (1040 + q) * 4, 0, 16);
      }
    }
    unsigned* cnt = p.cnt + qt * (int)gridDim.y + h;
    if (!split_arrive(cnt, s_eff, &s_last)) return;
    // ---- the last arrival merges every key tile, in key-tile order ----
    float mx = -INFINITY;
    for (int g2 = 0; g2 < s_eff; ++g2) {
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(p.part + (size_t)(slot0 + g2) * ATTN_PART_FLOATS), 0, ATTN_PART_FLOATS * 4, 0x00020000);
      mx = fmaxf(mx, __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (1024 + q) * 4, 0, 16)));
    }
    acc = f32x4{0.f, 0.f, 0.f, 0.f};
    l_run = 0.f;
    for (int g2 = 0; g2 < s_eff; ++g2) {
      const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(
          (void*)(p.part + (size_t)(slot0 + g2) * ATTN_PART_FLOATS), 0, ATTN_PART_FLOATS * 4, 0x00020000);
      const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs, (q * 64 + d4) * 4, 0, 16);
      const float mg = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (1024 + q) * 4, 0, 16));
      const float lg = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, (1040 + q) * 4, 0, 16));
      const float f = (mg > -INFINITY) ? expf(mg - mx) : 0.f;
      l_run += lg * f;
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] += __uint_as_float(v[e]) * f;
    }
    split_reset(cnt);
  }
  if (i0 + q < p.Tq) {
    const float inv = 1.0f / l_run;
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[e] *= inv;
    *reinterpret_cast<f32x4*>(p.O + (size_t)(i0 + q) * p.ldo + hoff + d4) = acc;
  }
}

// -------------------------------------------------------------------------------------------------
// The same (16-query tile, 64-key tile, head) arithmetic as attention_relpos_q16_kernel for the tail rows of MANY streaming sessions
// in one launch (PoolAttnArgs, stream_pool.hip).  Workgroup = (16-query tile of some session, head), found through the flattened
// prefix table; its four waves are the four 16-key sub-tiles of a key tile, and it walks the session's key tiles itself, merging each
// tile's normalised partial into a running (max, sum, output) -- no key split across workgroups, so no hand-off state and nothing
// that depends on what else is in the launch: a row's bits are a function of its own session.
// -------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attention_pool_kernel(PoolAttnArgs p) {
  __shared__ __attribute__((aligned(16))) float Gs_all[4 * 16 * LDG];
  __shared__ float ms[4][16], ls[4][16];
  __shared__ __attribute__((aligned(16))) float osum[4][16][Q16_LDO];
  const int t = threadIdx.x, lane = t & 63;
  const int r = lane & 15, g = lane >> 4;
  const int h = blockIdx.y, hoff = h * DH;
  const int gq = blockIdx.x;
  int lo = 0, hi = p.nsess - 1;                        // session of this query tile: last z with qt_pre[z] <= gq
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (p.qt_pre[mid] <= gq) lo = mid; else hi = mid - 1;
  }
  const int* se = p.sess + 8 * lo;
  const int q_start = se[0], Tq = se[1], q0 = se[2], Tk = se[3], slot = se[4], chunk = se[5];
  const int i0 = (gq - p.qt_pre[lo]) * 16;
  const float* Qs = p.Qs + (size_t)q_start * p.ld;
  float* cache = p.cache + (size_t)slot * p.slot_rows * p.ld;
  const float* P = p.P + (size_t)(p.p_tmax - Tk) * p.ldp;
  // q|k|v row of key j: the slot's cache below the first query, the stacked rows from there on (keys past the last: row 0, not read)
  auto krow = [&](int j) -> const float* {
    if (j >= Tk) j = 0;
    return j < q0 ? cache + (size_t)j * p.ld : Qs + (size_t)(j - q0) * p.ld;
  };

  const int q = t >> 4, d4 = (t & 15) * 4;              // thread (query q, columns d4 .. d4 + 3) of the cross-wave stage
  if (i0 + q < Tq) {                                    // this tile's rows of q|k|v (head h) into the slot cache
    const float* src = Qs + (size_t)(i0 + q) * p.ld + hoff + d4;
    float* dst = cache + (size_t)(q0 + i0 + q) * p.ld + hoff + d4;
#pragma unroll
    for (int part = 0; part < 3; ++part)
      *reinterpret_cast<f32x4*>(dst + part * p.H * DH) = *reinterpret_cast<const f32x4*>(src + part * p.H * DH);
  }
  const int kmax = chunk_bound(Tk, chunk, min(i0 + 16, Tq) - 1 + q0);
  const int s_eff = (kmax + KT - 1) / KT;
  const int iq = i0 + r;
  const bool q_ok = iq < Tq;
  const int lim = q_ok ? chunk_bound(Tk, chunk, iq + q0) : 0;
  f32x4 quf[4], qvf[4];
  load_qu_qv(quf, qvf, Qs, p.ld, iq, q_ok, p.bias_u, p.bias_v, hoff, g);
  f32x4 ACC = {0.f, 0.f, 0.f, 0.f};
  float M = -INFINITY, Lsum = 0.f;
  for (int sp = 0; sp < s_eff; ++sp) {
    if (sp > 0) __syncthreads();                        // the previous tile's LDS readers are done
    f32x4 acc;
    float m_t, l_t;
    q16_tile(quf, qvf, [&](int j) { return krow(j) + p.H * DH; }, [&](int j) { return krow(j) + 2 * p.H * DH; }, P, p.ldp, Tk,
             sp * KT, q0 + i0 + 15, lim, p.scale, hoff, Gs_all, ms, ls, osum, acc, m_t, l_t);
    if (sp == 0) {
      ACC = acc; M = m_t; Lsum = l_t;
    } else {                                            // merge the tile into the running (max, sum, output)
      const float mx = fmaxf(M, m_t);
      const float fa = (M > -INFINITY) ? expf(M - mx) : 0.f, fb = (m_t > -INFINITY) ? expf(m_t - mx) : 0.f;
#pragma unroll
      for (int e = 0; e < 4; ++e) ACC[e] = ACC[e] * fa + acc[e] * fb;
      Lsum = Lsum * fa + l_t * fb;
      M = mx;
    }
  }
  if (i0 + q < Tq) {
    const float inv = 1.0f / Lsum;
#pragma unroll
    for (int e = 0; e < 4; ++e) ACC[e] *= inv;
    *reinterpret_cast<f32x4*>(p.O + (size_t)(q_start + i0 + q) * p.ldo + hoff + d4) = ACC;
  }
}

int launch_attention_pool(const PoolAttnArgs& a, hipStream_t stream) {
  if (a.qtiles <= 0) return SS_OK;
  if (a.nsess <= 0 || !a.sess || !a.qt_pre || !a.P || !a.bias_u || !a.bias_v || a.ld != 3 * a.H * DH || (a.ldo & 3) || (a.ldp & 3) ||
      a.slot_rows <= 0 || a.p_tmax <= 0)
    return SS_ERR_ARG;
  hipLaunchKernelGGL(attention_pool_kernel, dim3(a.qtiles, a.H, 1), dim3(256), 0, stream, a);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

int launch_attention(const AttnArgs& a, hipStream_t stream) {
  const int tq = a.nseg > 0 ? a.max_q : a.Tq;
  if (tq <= 0 || (a.nseg == 0 && a.Tk <= 0)) return SS_OK;
  if ((a.ldk & 3) || (a.ldv & 3)) return SS_ERR_ARG;
  const int gz = a.nseg > 0 ? a.nseg : 1;
  if (a.q0 != 0 && (a.nseg > 0 || a.causal)) return SS_ERR_ARG;
  if (a.seg_tail && (a.nseg <= 0 || a.P)) return SS_ERR_ARG;   // per-segment key masks: ragged plain attention only
  if (a.anc) {      // the ancestry-indexed form exists in the ragged decode kernel only
    if (a.nseg <= 0 || a.P || tq > 8 || a.q0 != 0 || a.no_decode_kernel || a.anc_ld <= 0 || a.anc_slots <= 0) return SS_ERR_ARG;
    hipLaunchKernelGGL(attention_decode_kernel<true>, dim3(tq, a.H, gz), dim3(256), 0, stream, a);
    SS_LAUNCH_CHECK();
    return SS_OK;
  }
  if (!a.P && tq <= 8 && a.q0 == 0 && !a.no_decode_kernel) {
    hipLaunchKernelGGL(attention_decode_kernel<false>, dim3(tq, a.H, gz), dim3(256), 0, stream, a);
    SS_LAUNCH_CHECK();
    return SS_OK;
  }
  if (!a.P && a.q0 == 0 && !disp().attn_no_mfma && ((a.ldq | a.ldo) & 3) == 0) {
    hipLaunchKernelGGL(attention_mfma_kernel, dim3(cdiv(tq, MQ), a.H, gz), dim3(256), 0, stream, a);
    SS_LAUNCH_CHECK();
    return SS_OK;
  }
  dim3 grid(cdiv(tq, QB), a.H, gz);
  if (a.P) {
    if ((a.nseg == 0 && a.q0 + a.Tq != a.Tk) || (a.ldp & 3) || !a.bias_u || !a.bias_v) return SS_ERR_ARG;
    if (a.nseg > 0 && a.p_tmax <= 0) return SS_ERR_ARG;
    if (!disp().attn_no_mfma && ((a.ldq | a.ldo) & 3) == 0 && a.k_mask_tail == 0 && !a.causal) {
      const int nqt = cdiv(tq, MQ), nkt = cdiv(a.Tk, KT);
      // a few query rows over all keys (the incremental streaming encoder's tail rows): 16-query tiles, one workgroup per key tile
      if (a.nseg == 0 && tq <= 48 && disp().attn_q16 && (nkt == 1 || (a.part && cdiv(tq, 16) * a.H <= a.cnt_slots && cdiv(tq, 16) * a.H * nkt <= a.part_slots))) {
        AttnArgs b = a;
        b.ksplit = nkt; b.ktiles_per_split = 1;
        hipLaunchKernelGGL(attention_relpos_q16_kernel, dim3(cdiv(tq, 16) * nkt, a.H, 1), dim3(256), 0, stream, b);
        SS_LAUNCH_CHECK();
        return SS_OK;
      }
      // key split: one utterance with few (query tile, head) pairs and more than one key tile
      if (a.nseg == 0 && a.part && disp().attn_split >= 0 && nkt >= 2 && nqt * a.H <= a.cnt_slots && nqt * a.H < 128) {
        int tps = disp().attn_split > 0 ? disp().attn_split : cdiv(nkt, std::min(16, std::max(1, 256 / (nqt * a.H))));
        tps = std::max(tps, cdiv(nkt, 16));
        const int S = cdiv(nkt, tps);
        if (S >= 2 && nqt * a.H * S <= a.part_slots) {
          AttnArgs b = a;
          b.ksplit = S; b.ktiles_per_split = tps;
          SS_MAX_LDS_ONCE(&attention_relpos_mfma_kernel<true>, kRelposLds);
          hipLaunchKernelGGL(attention_relpos_mfma_kernel<true>, dim3(nqt * S, a.H, 1), dim3(256), kRelposLds, stream, b);
          SS_LAUNCH_CHECK();
          return SS_OK;
        }
      }
      SS_MAX_LDS_ONCE(&attention_relpos_mfma_kernel<false>, kRelposLds);
      hipLaunchKernelGGL(attention_relpos_mfma_kernel<false>, dim3(nqt, a.H, gz), dim3(256), kRelposLds, stream, a);
      SS_LAUNCH_CHECK();
      return SS_OK;
    }
    hipLaunchKernelGGL(attention_kernel<true>, grid, dim3(256), 0, stream, a);
  } else {
    hipLaunchKernelGGL(attention_kernel<false>, grid, dim3(256), 0, stream, a);
  }
  SS_LAUNCH_CHECK();
  return SS_OK;
}

}  // namespace ss
