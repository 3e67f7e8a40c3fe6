// Implicit-GEMM Conv1d / Linear kernel for gfx950, exact-f32 MFMA (see gemm.hpp).
//
// Tiling: a 256-thread workgroup (4 wave64) owns a BM x BN output tile; the K loop walks
// (tap, channel-block) pairs in BK-wide steps.  Per step the A rows (shifted by the tap) and the
// W rows are staged global -> registers -> LDS (register prefetch of step k+1 overlaps the MFMAs
// of step k, one barrier per step), then each wave feeds v_mfma_f32_16x16x4_f32 from LDS with
// ds_read_b128: lane (r = lane&15, g = lane>>4) reads 4 consecutive k of row r at k-offset 4g
// and issues 4 MFMAs; MFMA i therefore contracts k = {i, 4+i, 8+i, 12+i} of the 16-wide slab --
// a permutation of k shared by A and B, which leaves the sum unchanged.
// C/D layout (MI355X guide §3): col = lane&15, row = (lane>>4)*4 + reg.
#include "gemm.hpp"

#include <type_traits>

namespace ss {

using f32x4 = __attribute__((ext_vector_type(4))) float;

// KS > 1: intra-workgroup split-K.  The workgroup has KS groups of 4 waves; every group owns the
// whole BM x BN tile but only 1/KS of the k-steps, with private LDS staging, and the partial tiles
// are summed (fixed order) through LDS before the epilogue.  This fills all 1024 SIMDs when M*N
// alone gives too few tiles (early vocoder stages, M~500 decoder GEMMs) without atomics or a
// second launch.
//
// BLK (the pack-invariant CANON_SEQ form, gemm.hpp): the k walk is cut into blocks of CANON_KBLOCK = 64 -- one accumulator chain inside a
// block, the block sums added in ascending order into a second accumulator set ("tot += acc; acc = 0" every 64 / BK steps).  A
// function of the walk alone (taps, Cin), not of M or the grid.  Rounding of a K-term sum then grows like a 64-term chain + K / 64
// adds instead of a K-term chain (the K = 256 chains sat 1.35-1.5x, the K = 2048 / 5120 ones 2.8-3.8x farther from
// float64 than torch's CPU sgemm on the GPU box; this form: ~0.7x).
template <int BM, int BN, int BK, int WM, int WN, int KS, int PD, bool BLK = false>
__global__ __launch_bounds__(256 * KS) void conv_gemm_kernel(const GemmArgs p) {
  static_assert(WM * WN == 4, "4 waves per k-group");
  static_assert(!BLK || KS == 1, "the blocked chain is the KS = 1 form");
  // row stride in floats: 16-B aligned and = 10 (BK=32) / 6 (BK=16) sixteen-byte slots, which makes the
  // 16-lane groups of ds_read_b128 hit 16 distinct slots (conflict-free; +4 was 2-way)
  constexpr int LDK = BK + 8;
  constexpr int WTM = BM / WM, WTN = BN / WN;
  constexpr int TM = WTM / 16, TN = WTN / 16;
  static_assert(TM >= 1 && TN >= 1, "wave tile must hold a 16x16 MFMA tile");
  constexpr int KQ = BK / 4;
  constexpr int A_F4 = BM * KQ, W_F4 = BN * KQ;
  constexpr int NA = (A_F4 + 255) / 256, NW = (W_F4 + 255) / 256;
  constexpr int STAGE = (BM + BN) * LDK;
  extern __shared__ __attribute__((aligned(16))) float smem_all[];
  const int kg = threadIdx.x >> 8;                     // k-group of this thread
  float* smem = smem_all + kg * 2 * STAGE;

  const int t = threadIdx.x & 255, lane = t & 63, wave = t >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int r = lane & 15, g = lane >> 4;

  int out_start = 0, out_len = p.M, in_start = 0, in_len = p.in_len, m_begin = p.m_begin, chunk = p.chunk;
  const float* A = p.A;
  if (p.nseg > 0) {
    const int* s = p.segs + 4 * blockIdx.z;
    out_start = s[0]; out_len = s[1]; in_start = s[2]; in_len = s[3];
    if (p.seg_mb) { m_begin = p.seg_mb[2 * blockIdx.z]; chunk = p.seg_mb[2 * blockIdx.z + 1]; }
    if (p.seg_A) A = p.seg_A[blockIdx.z];
  }
  const int m0 = blockIdx.x * BM + m_begin;
  if (m0 >= out_len) return;
  const int n0 = blockIdx.y * BN;
  const int kpt = p.Cin / BK;          // k-steps per tap
  const int nk = p.taps * kpt;
  const int Ktot = p.taps * p.Cin;

  // per-thread staging slots
  int a_rin0[NA], a_lim[NA], a_c4[NA], a_lds[NA];
  bool a_ok[NA];
#pragma unroll
  for (int i = 0; i < NA; ++i) {
    const int f = t + i * 256;
    const int row = f / KQ, c4 = f % KQ;
    const int m = m0 + row;
    a_ok[i] = (f < A_F4) && (m < out_len);
    a_rin0[i] = m * p.stride - p.pad;
    a_lim[i] = chunk > 0 ? ((m * p.stride) / chunk + 1) * chunk : 0x7fffffff;
    a_c4[i] = c4 * 4;
    a_lds[i] = row * LDK + c4 * 4;
  }
  int w_c4[NW], w_lds[NW];
  size_t w_off[NW];
  bool w_ok[NW];
#pragma unroll
  for (int i = 0; i < NW; ++i) {
    const int f = t + i * 256;
    const int row = f / KQ, c4 = f % KQ;
    const int n = n0 + row;
    w_ok[i] = (f < W_F4) && (n < p.N);
    w_off[i] = (size_t)n * Ktot + c4 * 4;
    w_c4[i] = c4 * 4;
    w_lds[i] = BM * LDK + row * LDK + c4 * 4;
  }

  // Register ring of PD k-steps: the global loads of step k+PD are issued before the MFMAs of
  // step k, so a load has PD steps of MFMA work to land before its turn to be written to LDS
  // (the leaky-ReLU input activation is applied at that write, never right after the load).
  f32x4 ra[PD][NA], rw[PD][NW];
  auto load_regs = [&](auto SLOT, bool valid, int kb, int tap, int ci0) {
    constexpr int sl = decltype(SLOT)::value;
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int rin = a_rin0[i] + tap * p.dil;
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (valid && a_ok[i] && rin >= 0 && rin < in_len && rin < a_lim[i])
        v = *reinterpret_cast<const f32x4*>(A + (size_t)(in_start + rin) * p.lda + ci0 + a_c4[i]);
      ra[sl][i] = v;
    }
#pragma unroll
    for (int i = 0; i < NW; ++i) {
      f32x4 v = {0.f, 0.f, 0.f, 0.f};
      if (valid && w_ok[i]) v = *reinterpret_cast<const f32x4*>(p.W + w_off[i] + (size_t)tap * p.Cin + ci0);
      rw[sl][i] = v;
    }
  };
  const bool lrelu = p.in_act == ACT_LRELU;
  const float slope = p.in_slope;
  auto store_lds = [&](auto SLOT, int buf) {
    constexpr int sl = decltype(SLOT)::value;
    float* base = smem + buf * STAGE;
#pragma unroll
    for (int i = 0; i < NA; ++i)
      if (t + i * 256 < A_F4) {
        f32x4 v = ra[sl][i];
        if (lrelu) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = v[e] > 0.f ? v[e] : v[e] * slope;
        }
        *reinterpret_cast<f32x4*>(base + a_lds[i]) = v;
      }
#pragma unroll
    for (int i = 0; i < NW; ++i)
      if (t + i * 256 < W_F4) *reinterpret_cast<f32x4*>(base + w_lds[i]) = rw[sl][i];
  };

  f32x4 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};
  [[maybe_unused]] f32x4 tot[BLK ? TM : 1][BLK ? TN : 1];
  [[maybe_unused]] bool flushed = false;
  constexpr int BLK_STEPS = CANON_KBLOCK / BK;

  // k-steps of this group: [kb0, kb1); every group runs `kper` iterations (steps past kb1 load
  // zeros) so barriers and the MFMA body stay uniform
  const int kper = (nk + KS - 1) / KS;
  const int kb0 = kg * kper;
  const int kb1 = min(nk, kb0 + kper);
  // k-step s = (channel block s / taps, tap s % taps): the taps of one channel block run back to back
  // so the tile's A rows are re-read while still in L1/L2 (see conv_sk.hip)
  int nci = (kb0 / p.taps) * BK;             // (tap, channel offset) of the next step to load
  int ntap = kb0 - (kb0 / p.taps) * p.taps;
  auto advance = [&]() { if (++ntap >= p.taps) { ntap = 0; nci += BK; } };
  auto for_slots = [&](auto&& fn) {          // fn(integral_constant<u>) for u = 0..PD-1
    fn(std::integral_constant<int, 0>{});
    if constexpr (PD > 1) fn(std::integral_constant<int, 1>{});
    if constexpr (PD > 2) fn(std::integral_constant<int, 2>{});
    if constexpr (PD > 3) fn(std::integral_constant<int, 3>{});
  };
  for_slots([&](auto U) {
    constexpr int u = decltype(U)::value;
    load_regs(U, kb0 + u < kb1, kb0 + u, ntap, nci);
    advance();
  });
  store_lds(std::integral_constant<int, 0>{}, 0);
  __syncthreads();

  for (int it0 = 0; it0 < kper; it0 += PD) {
    for_slots([&](auto U) {
      constexpr int u = decltype(U)::value;
      const int it = it0 + u;
      if (it < kper) {                       // block-uniform
        const int cur = it & 1;
        load_regs(U, kb0 + it + PD < kb1, kb0 + it + PD, ntap, nci);   // slot u (step it) is already in LDS
        advance();
        const float* As = smem + cur * STAGE + (wm * WTM + r) * LDK + g * 4;
        const float* Ws = smem + cur * STAGE + BM * LDK + (wn * WTN + r) * LDK + g * 4;
#pragma unroll
        for (int kk = 0; kk < BK / 16; ++kk) {
          f32x4 af[TM], bf[TN];
#pragma unroll
          for (int i = 0; i < TM; ++i) af[i] = *reinterpret_cast<const f32x4*>(As + i * 16 * LDK + kk * 16);
#pragma unroll
          for (int j = 0; j < TN; ++j) bf[j] = *reinterpret_cast<const f32x4*>(Ws + j * 16 * LDK + kk * 16);
#pragma unroll
          for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
              for (int j = 0; j < TN; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(bf[j][e], af[i][e], acc[i][j], 0, 0, 0);   // D = W.A^T (see epilogue)
        }
        if constexpr (BLK) {
          if ((it + 1) % BLK_STEPS == 0 && it + 1 < kper) {      // block boundary of the walk (block-uniform)
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
              for (int j = 0; j < TN; ++j) {
#pragma unroll
                for (int e = 0; e < 4; ++e) tot[i][j][e] = flushed ? tot[i][j][e] + acc[i][j][e] : acc[i][j][e];
                acc[i][j] = {0.f, 0.f, 0.f, 0.f};
              }
            flushed = true;
          }
        }
        if (it + 1 < kper) store_lds(std::integral_constant<int, (u + 1) % PD>{}, cur ^ 1);
        __syncthreads();
      }
    });
  }
  if constexpr (BLK) {
    if (flushed) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[i][j][e] = tot[i][j][e] + acc[i][j][e];
    }
  }

  if (KS > 1) {
    // partial tiles of groups 1..KS-1 -> LDS (staging buffers are dead now), group 0 sums in order
    f32x4* red = reinterpret_cast<f32x4*>(smem_all);
    constexpr int PER_GROUP = 4 * TM * TN * 64;
    if (kg > 0) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          red[(kg - 1) * PER_GROUP + ((wave * TM + i) * TN + j) * 64 + lane] = acc[i][j];
    }
    __syncthreads();
    if (kg > 0) return;
#pragma unroll
    for (int s2 = 1; s2 < KS; ++s2)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          const f32x4 o = red[(s2 - 1) * PER_GROUP + ((wave * TM + i) * TN + j) * 64 + lane];
#pragma unroll
          for (int e = 0; e < 4; ++e) acc[i][j][e] += o[e];
        }
  }

  // ---- epilogue ----
  auto activate = [&](float v) -> float { return act_apply(p.act, v, p.act_slope); };
  // The MFMAs are issued with the operands swapped (D = W_tile . A_tile^T): in the C/D layout
  // (col = lane&15, row = 4*(lane>>4) + reg) a lane then holds 4 CONSECUTIVE output channels
  // n = 4g..4g+3 of ONE row m = r, so bias / residual / output move as float4 whenever the leading
  // dimensions allow it (4x fewer memory instructions; scalar fallback otherwise, e.g. N = 1005).
  if (p.glu) {
    if constexpr (TN % 2 == 0) {
      const bool vec = (p.ldc & 3) == 0;
#pragma unroll
      for (int i = 0; i < TM; ++i) {
        const int m = m0 + wm * WTM + i * 16 + r;
        if (m >= out_len) continue;
        float* crow = p.C + (size_t)(out_start + m) * p.ldc;
#pragma unroll
        for (int j = 0; j < TN; j += 2) {
          const int ncol = n0 + wn * WTN + j * 16;      // start of the [value|gate] 32-col block
          if (ncol + 31 >= p.N) continue;
          const int oc = ncol / 2 + g * 4;              // first of this lane's 4 output channels
          f32x4 o;
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const float bv = p.bias ? p.bias[ncol + g * 4 + e] : 0.f;
            const float bg = p.bias ? p.bias[ncol + 16 + g * 4 + e] : 0.f;
            const float val = acc[i][j][e] + bv;
            const float gate = acc[i][j + 1][e] + bg;
            o[e] = val * (1.0f / (1.0f + expf(-gate)));
          }
          if (vec) *reinterpret_cast<f32x4*>(crow + oc) = o;
          else {
#pragma unroll
            for (int e = 0; e < 4; ++e) crow[oc + e] = o[e];
          }
        }
      }
    }
    return;
  }
  const bool vec = ((p.ldc | (p.R ? p.ldr : 0) | (p.R2 ? p.ldr2 : 0) | (p.C2 ? p.ldc2 : 0) | p.N) & 3) == 0;
#pragma unroll
  for (int i = 0; i < TM; ++i) {
    const int m = m0 + wm * WTM + i * 16 + r;
    if (m >= out_len) continue;
    const size_t row = (size_t)(out_start + m);
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      const int n = n0 + wn * WTN + j * 16 + g * 4;
      if (n >= p.N) continue;
      f32x4 v = acc[i][j];
      if (vec) {
        if (p.bias) {
          const f32x4 b = *reinterpret_cast<const f32x4*>(p.bias + n);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += b[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = activate(v[e]) * p.alpha;
        if (p.R) {
          const f32x4 rr = *reinterpret_cast<const f32x4*>(p.R + row * p.ldr + n);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] += rr[e];
        }
        if (p.R2) {
          const f32x4 rr = *reinterpret_cast<const f32x4*>(p.R2 + row * p.ldr2 + n);
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = rr[e] + v[e];
        }
        if (p.div > 0.f) {
#pragma unroll
          for (int e = 0; e < 4; ++e) v[e] = v[e] / p.div;
        }
        *reinterpret_cast<f32x4*>(p.C + row * p.ldc + n) = v;
        if (p.C2) {
          f32x4 w2;
#pragma unroll
          for (int e = 0; e < 4; ++e) w2[e] = v[e] > 0.f ? v[e] : v[e] * p.c2_slope;
          *reinterpret_cast<f32x4*>(p.C2 + row * p.ldc2 + n) = w2;
        }
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          if (n + e >= p.N) continue;
          float x = activate(v[e] + (p.bias ? p.bias[n + e] : 0.f)) * p.alpha;
          if (p.R) x += p.R[row * p.ldr + n + e];
          if (p.R2) x = p.R2[row * p.ldr2 + n + e] + x;
          if (p.div > 0.f) x = x / p.div;
          p.C[row * p.ldc + n + e] = x;
          if (p.C2) p.C2[row * p.ldc2 + n + e] = x > 0.f ? x : x * p.c2_slope;
        }
      }
    }
  }
}


// Store of the two no-LDS kernels below: C[m][n] = act(acc + b) * alpha [+ R[m][n]], act = SiLU / ReLU / none
__device__ __forceinline__ void linear_store(const GemmArgs& p, int m, int n, float acc, float b) {
  float v = acc + b;
  switch (p.act) {
    case ACT_SILU: v = v / (1.0f + expf(-v)); break;
    case ACT_RELU: v = fmaxf(v, 0.f); break;
    default: break;
  }
  v *= p.alpha;
  if (p.R) v += p.R[(size_t)m * p.ldr + n];
  p.C[(size_t)m * p.ldc + n] = v;
}

// =================================================================================================
// Small-M linear layers (M <= 128: every encoder/decoder projection at batch 1, decode steps at
// M = 1).  These are latency-bound, so there is no LDS staging and no barrier in the main loop:
// a workgroup owns 16 rows x (16*WN) columns, its 4 waves are arranged SK (split-K) x WN, and
// each wave feeds v_mfma_f32_16x16x4_f32 straight from global memory -- lane (r, g) loads the
// float4 at [row r][k + 4g] of A and of W (64-B row segments), 4 MFMAs per pair of loads, loads
// of 4 chunks kept in flight.  The SK partial tiles are summed through LDS once at the end.
// Optional fused LayerNorm over K on the A rows (two-pass statistics per wave, rows stay in L1).
// =================================================================================================
template <int SK, int WN, bool LNORM, bool GLU = false>
__global__ __launch_bounds__(256) void smallm_gemm_kernel(const GemmArgs p) {
  static_assert(SK * WN == 4, "4 waves");
  static_assert(!GLU || (SK == 2 && WN == 2), "GLU: wave column 0 = the 16 value columns, 1 = the 16 gate columns of a 32-column block");
  __shared__ f32x4 red[SK > 1 ? (SK - 1) * WN * 64 : 1];
  __shared__ float ln_stat[32];                   // mean[16], rstd[16] of the workgroup's rows
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int sk = wave / WN, wn = wave % WN;
  const int r = lane & 15, g = lane >> 4;
  // n-tiles run fastest and their count is a multiple of 8 (launch_smallm): blocks land on XCD (linear id % 8), so the W rows
  // of an n-tile are fetched by ONE XCD's L2 for all m-tiles instead of by as many XCDs as there are m-tiles (the rows are
  // the small operand here; MI355X_MICROARCH.md "block b runs on XCD b % 8" -- a speed affinity, nothing depends on it)
  if ((int)blockIdx.x * (16 * WN) >= p.N) return;
  const int m0 = blockIdx.y * 16;
  const int n0 = blockIdx.x * (16 * WN) + wn * 16;
  const int K = p.Cin;
  const int KC = K / 16;                          // 16-wide chunks
  const int c_begin = (KC * sk) / SK, c_end = (KC * (sk + 1)) / SK;

  const int am = m0 + r;
  const bool a_ok = am < p.M;
  const float* arow = p.A + (size_t)(a_ok ? am : 0) * p.lda + 4 * g;
  const int wnr = n0 + r;
  const bool w_ok = wnr < p.N;
  const float* wrow = p.W + (size_t)(w_ok ? wnr : 0) * K + 4 * g;

  float mean = 0.f, rstd = 1.f;
  if (LNORM) {
    // 16 threads per row, each keeps its K/16 values in registers (K <= 512): one read, two-pass stats
    const int lr = t >> 4, part = t & 15;
    const bool ok = (m0 + lr) < p.M;
    const float* xr = p.A + (size_t)(ok ? m0 + lr : 0) * p.lda + part * 4;
    f32x4 v[8];
    float sm = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      v[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (j * 64 < K && ok) v[j] = *reinterpret_cast<const f32x4*>(xr + j * 64);
      sm += (v[j][0] + v[j][1]) + (v[j][2] + v[j][3]);
    }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) sm += __shfl_xor(sm, o, 64);
    const float mu = sm / (float)K;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (j * 64 < K) {
#pragma unroll
        for (int e = 0; e < 4; ++e) { const float d = v[j][e] - mu; q += d * d; }
      }
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) q += __shfl_xor(q, o, 64);
    if (part == 0) { ln_stat[lr] = mu; ln_stat[16 + lr] = 1.0f / sqrtf(q / (float)K + 1e-5f); }
    __syncthreads();
    mean = ln_stat[r];
    rstd = ln_stat[16 + r];
  }

  f32x4 acc = {0.f, 0.f, 0.f, 0.f}, acc2 = {0.f, 0.f, 0.f, 0.f};   // 2 chains: MFMA dependent latency 40 > issue 32
  f32x4 tot = {0.f, 0.f, 0.f, 0.f};
  // a wave whose k-range is at most 128 (K <= 512 on four waves) already runs two chains of <= 64 terms: nothing to cut.  A function of
  // (K, SK) alone -- never of M -- so a row's bits stay the same in any pack.
  const bool blocked = (c_end - c_begin) > 8;
  auto load4 = [&](f32x4 (&a)[4], f32x4 (&w)[4], int c) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      a[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      w[u] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (a_ok) a[u] = *reinterpret_cast<const f32x4*>(arow + (c + u) * 16);
      if (w_ok) w[u] = *reinterpret_cast<const f32x4*>(wrow + (c + u) * 16);
    }
  };
  auto mma = [&](f32x4 a, f32x4 w, int c) {
    if (LNORM) {
      const f32x4 gm = *reinterpret_cast<const f32x4*>(p.ln_g + c * 16 + 4 * g);
      const f32x4 bt = *reinterpret_cast<const f32x4*>(p.ln_b + c * 16 + 4 * g);
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] = a_ok ? (a[e] - mean) * rstd * gm[e] + bt[e] : 0.f;
    }
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[0], w[0], acc, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[1], w[1], acc2, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[2], w[2], acc, 0, 0, 0);
    acc2 = __builtin_amdgcn_mfma_f32_16x16x4f32(a[3], w[3], acc2, 0, 0, 0);
    if (blocked && (c & 3) == 3) {  // end of a 64-wide k-block (round 6, gemm.hpp CANON_KBLOCK): block sums added in ascending order
#pragma unroll
      for (int e = 0; e < 4; ++e) { tot[e] += acc[e] + acc2[e]; acc[e] = 0.f; acc2[e] = 0.f; }
    }
  };
  auto mma4 = [&](f32x4 (&a)[4], f32x4 (&w)[4], int c) {
#pragma unroll
    for (int u = 0; u < 4; ++u) mma(a[u], w[u], c + u);
  };
  // groups of 4 chunks, register double-buffered: the loads of group g+1 fly under the MFMAs of g
  const int G = (c_end - c_begin) / 4;
  f32x4 a0[4], w0[4], a1[4], w1[4];
  if (G > 0) load4(a0, w0, c_begin);
  for (int gi = 0; gi < G; gi += 2) {
    const int c = c_begin + 4 * gi;
    if (gi + 1 < G) load4(a1, w1, c + 4);
    mma4(a0, w0, c);
    if (gi + 1 < G) {
      if (gi + 2 < G) load4(a0, w0, c + 8);
      mma4(a1, w1, c + 4);
    }
  }
  for (int c = c_begin + 4 * G; c < c_end; ++c) {
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, w = {0.f, 0.f, 0.f, 0.f};
    if (a_ok) a = *reinterpret_cast<const f32x4*>(arow + c * 16);
    if (w_ok) w = *reinterpret_cast<const f32x4*>(wrow + c * 16);
    mma(a, w, c);
  }
#pragma unroll
  for (int e = 0; e < 4; ++e) acc[e] = tot[e] + (acc[e] + acc2[e]);

  if (SK > 1) {
    if (sk > 0) red[((sk - 1) * WN + wn) * 64 + lane] = acc;
    __syncthreads();
    if (!GLU && sk > 0) return;
    if (sk == 0) {
#pragma unroll
      for (int s2 = 1; s2 < SK; ++s2) {
        const f32x4 o = red[((s2 - 1) * WN + wn) * 64 + lane];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[e] += o[e];
      }
    }
  }
  if constexpr (GLU) {
    // out[m, 16 b + r] = (value + bias) * sigmoid(gate + bias): the gate wave hands its tile to the value wave through LDS
    // (same formula and packing as the tile kernel's GLU epilogue: [16 value | 16 gate] column blocks)
    __shared__ f32x4 gate_tile[64];
    const int ncol = n0 + r;                               // this lane's column of the packed [value | gate] matrix
    const float bcol = (p.bias && ncol < p.N) ? p.bias[ncol] : 0.f;
    if (sk == 0 && wn == 1) {
      f32x4 gt;
#pragma unroll
      for (int e = 0; e < 4; ++e) gt[e] = acc[e] + bcol;
      gate_tile[lane] = gt;
    }
    __syncthreads();
    if (sk != 0 || wn != 0 || ncol + 16 >= p.N) return;
    const f32x4 gt = gate_tile[lane];
    const int oc = (int)blockIdx.x * 16 + r;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int m = m0 + g * 4 + e;
      if (m < p.M) p.C[(size_t)m * p.ldc + oc] = (acc[e] + bcol) * (1.0f / (1.0f + expf(-gt[e])));
    }
    return;
  }
  const int n = n0 + r;
  if (n >= p.N) return;
  const float b = p.bias ? p.bias[n] : 0.f;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const int m = m0 + g * 4 + e;
    if (m < p.M) linear_store(p, m, n, acc[e], b);
  }
}


// =================================================================================================
// GEMV form for decode steps (M <= 4 rows: one new MT token, B = 1): these stream 1-4 MB of weights
// for a few kFLOP, so the matrix cores are irrelevant and what counts is bytes in flight.  One wave
// per output column (KS waves per column when N alone gives too few waves to cover the chip): the
// lanes split K in float4 steps, so every weight row is read as fully coalesced 1-KB wave loads, all
// of a column's loads are issued before the first FMA, and the A rows (optionally LayerNorm'ed in
// registers: each wave holds the whole row) are loaded once per wave.  Wave-shuffle reduction, fused
// bias / activation / alpha / residual.  K % 256 == 0, K <= 2048.
// =================================================================================================
template <int MR, int KS, bool LNORM>
__global__ __launch_bounds__(256) void gemv_kernel(const GemmArgs p) {
  constexpr int WPB = 4;                       // waves per block
  constexpr int CPB = WPB / KS;                // columns per block
  __shared__ float part[WPB][MR];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int col = blockIdx.x * CPB + wave / KS;
  const int ks = wave % KS;
  const int K = p.Cin;
  const int kper = K / KS;                     // this wave's slice of K (multiple of 256)
  const int k0 = ks * kper;
  const int nit = kper / 256;                  // float4 steps per lane (<= 8)
  const bool col_ok = col < p.N;

  // weight slice of the column: issue everything first
  f32x4 wv[8];
  const float* wrow = p.W + (size_t)(col_ok ? col : 0) * K + k0 + 4 * lane;
#pragma unroll
  for (int it = 0; it < 8; ++it) {
    wv[it] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (it < nit && col_ok) wv[it] = *reinterpret_cast<const f32x4*>(wrow + it * 256);
  }
  float acc[MR];
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    acc[m] = 0.f;
    if (m >= p.M) continue;
    const float* xrow = p.A + (size_t)m * p.lda;
    float mean = 0.f, rstd = 1.f;
    if (LNORM) {                               // whole row per wave (K <= 2048: 8 float4 per lane), two-pass statistics
      f32x4 xv[8];
      float sm = 0.f;
#pragma unroll
      for (int it = 0; it < 8; ++it) {
        xv[it] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (it * 256 < K) xv[it] = *reinterpret_cast<const f32x4*>(xrow + it * 256 + 4 * lane);
        sm += (xv[it][0] + xv[it][1]) + (xv[it][2] + xv[it][3]);
      }
      mean = wave_sum(sm) / (float)K;
      float q = 0.f;
#pragma unroll
      for (int it = 0; it < 8; ++it)
        if (it * 256 < K) {
#pragma unroll
          for (int e = 0; e < 4; ++e) { const float d = xv[it][e] - mean; q += d * d; }
        }
      rstd = 1.0f / sqrtf(wave_sum(q) / (float)K + 1e-5f);
    }
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
    for (int it = 0; it < 8; ++it)
      if (it < nit) {
        f32x4 x = *reinterpret_cast<const f32x4*>(xrow + k0 + it * 256 + 4 * lane);
        if (LNORM) {
          const f32x4 gm = *reinterpret_cast<const f32x4*>(p.ln_g + k0 + it * 256 + 4 * lane);
          const f32x4 bt = *reinterpret_cast<const f32x4*>(p.ln_b + k0 + it * 256 + 4 * lane);
#pragma unroll
          for (int e = 0; e < 4; ++e) x[e] = (x[e] - mean) * rstd * gm[e] + bt[e];
          // the waves of column 0 cover the whole row between them: they also publish the normalised row
          if (p.ln_out && blockIdx.x == 0 && wave < KS)
            *reinterpret_cast<f32x4*>(p.ln_out + (size_t)m * K + k0 + it * 256 + 4 * lane) = x;
        }
        a0 = fmaf(x[0], wv[it][0], a0); a1 = fmaf(x[1], wv[it][1], a1);
        a2 = fmaf(x[2], wv[it][2], a2); a3 = fmaf(x[3], wv[it][3], a3);
      }
    acc[m] = wave_sum((a0 + a1) + (a2 + a3));
  }
  if (KS > 1) {
    if (lane == 0) {
#pragma unroll
      for (int m = 0; m < MR; ++m) part[wave][m] = acc[m];
    }
    __syncthreads();
    if (ks != 0) return;
#pragma unroll
    for (int m = 0; m < MR; ++m)
#pragma unroll
      for (int s2 = 1; s2 < KS; ++s2) acc[m] += part[wave + s2][m];
  }
  if (lane != 0 || !col_ok) return;
  const float b = p.bias ? p.bias[col] : 0.f;
#pragma unroll
  for (int m = 0; m < MR; ++m) {
    if (m < p.M) linear_store(p, m, col, acc[m], b);
  }
}

bool gemv_eligible(const GemmArgs& a) {
  return smallm_eligible(a) && !a.glu && a.M <= 4 && a.Cin % 256 == 0 && a.Cin <= 2048;   // (the GEMV has no GLU epilogue)
}

template <int KS>
static int launch_gemv_ks(const GemmArgs& a, hipStream_t stream) {
  dim3 grid(cdiv(a.N, 4 / KS));
  ProfRec rec{}; bool prof = false;
  int rc = prof_begin(a, stream, PROF_SMALLM_4x1, rec, prof);     // profiled with the small-M class (decode GEMVs)
  if (rc != SS_OK) return rc;
  if (a.ln_g) hipLaunchKernelGGL((gemv_kernel<4, KS, true>), grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((gemv_kernel<4, KS, false>), grid, dim3(256), 0, stream, a);
  SS_LAUNCH_CHECK();
  return prof_end(stream, rec, prof);
}

static int launch_gemv(const GemmArgs& a, hipStream_t stream) {
  // waves = N * KS: cover ~1024 SIMDs; KS must divide K/256
  const int kq = a.Cin / 256;
  if (a.N * 1 >= 2048 || kq % 2 != 0) return launch_gemv_ks<1>(a, stream);
  if (a.N * 2 >= 2048 || kq % 4 != 0) return launch_gemv_ks<2>(a, stream);
  return launch_gemv_ks<4>(a, stream);
}


// register prefetch depth: measured flat from 1 to 4 on MI355X (profiles/r01_tile_sweep.txt) -> 1
constexpr int default_pd(int, int) { return 1; }

template <int BM, int BN, int BK, int WM, int WN, int KS = 1, int PD = default_pd(BM, BN), bool BLK = false>
static int launch_cfg(const GemmArgs& a, hipStream_t stream, ProfCls cls) {
  constexpr size_t kLds = (size_t)KS * 2 * (BM + BN) * (BK + 8) * sizeof(float);
  static_assert(kLds <= 160 * 1024, "LDS budget");
  static_assert((size_t)(KS - 1) * BM * BN * sizeof(float) <= kLds, "reduction scratch fits the staging buffers");
  if constexpr (kLds > 64 * 1024) SS_MAX_LDS_ONCE((&conv_gemm_kernel<BM, BN, BK, WM, WN, KS, PD, BLK>), kLds);
  const int mmax = (a.nseg > 0 ? a.max_seg_out : a.M) - a.m_begin;
  dim3 grid(cdiv(mmax, BM), cdiv(a.N, BN), a.nseg > 0 ? a.nseg : 1);
  // XCD affinity (speed only): blocks land on XCD (linear id % 8).  With a multiple of 8 m-tiles per grid row every n-tile
  // column keeps m-tile i on XCD i % 8, so each XCD's L2 fetches 1/8 of the A rows (and all of W) instead of all of both --
  // the 3.0-3.9x counter-over-algorithmic traffic of the K = 256 encoder GEMMs (profiles/r02_pmc_traffic.json) was exactly
  // 8 x (A + W) + C.  The padding blocks leave at once (m0 >= out_len); not worth it for a handful of tiles.
  if (grid.x >= 32 && grid.y * grid.z > 1) grid.x = (grid.x + 7) & ~7u;
  ProfRec rec{}; bool prof = false;
  int rc = prof_begin(a, stream, cls, rec, prof);
  if (rc != SS_OK) return rc;
  hipLaunchKernelGGL((conv_gemm_kernel<BM, BN, BK, WM, WN, KS, PD, BLK>), grid, dim3(256 * KS), kLds, stream, a);
  SS_LAUNCH_CHECK();
  return prof_end(stream, rec, prof);
}

// pick the k-split so that tiles * 4 * KS waves cover the 1024 SIMDs (each group keeps >= 2 k-steps)
template <int BM, int BN, int BK, int WM, int WN, int MAXKS>
static int launch_cfg_ks(const GemmArgs& a, hipStream_t stream, ProfCls cls, long tiles) {
  const int nk = a.taps * (a.Cin / BK);
  int ks = 1;
  while (ks < MAXKS && tiles * 4 * ks < 1024 && nk / (ks * 2) >= 2) ks *= 2;
  if constexpr (MAXKS >= 4) { if (ks >= 4) return launch_cfg<BM, BN, BK, WM, WN, 4>(a, stream, cls); }
  if constexpr (MAXKS >= 2) { if (ks >= 2) return launch_cfg<BM, BN, BK, WM, WN, 2>(a, stream, cls); }
  return launch_cfg<BM, BN, BK, WM, WN, 1>(a, stream, cls);
}

template <int SK, int WN, bool GLU = false>
static int launch_smallm(const GemmArgs& a, hipStream_t stream, ProfCls cls) {
  if (a.ln_g && a.Cin > 512) return SS_ERR_ARG;   // fused LayerNorm keeps the row in registers (D <= 512); refused BEFORE prof_begin: the census counts launches
  dim3 grid((cdiv(a.N, 16 * WN) + 7) & ~7, cdiv(a.M, 16));   // see the kernel: n-tiles fastest, a multiple of 8 of them
  ProfRec rec{}; bool prof = false;
  int rc = prof_begin(a, stream, cls, rec, prof);
  if (rc != SS_OK) return rc;
  if (a.ln_g) hipLaunchKernelGGL((smallm_gemm_kernel<SK, WN, true, GLU>), grid, dim3(256), 0, stream, a);
  else hipLaunchKernelGGL((smallm_gemm_kernel<SK, WN, false, GLU>), grid, dim3(256), 0, stream, a);
  SS_LAUNCH_CHECK();
  return prof_end(stream, rec, prof);
}


// One rung of the tile ladder: the blocked-chain form (BLK: one k-group), or the plain form with the k-split that lets
// tiles * 4 * KS waves cover the SIMDs, up to MAXKS (1: none)
template <bool BLK, int BM, int BN, int BK, int WM, int WN, int MAXKS>
static int launch_rung(const GemmArgs& a, hipStream_t stream, ProfCls cls, long tiles) {
  if constexpr (BLK) return launch_cfg<BM, BN, BK, WM, WN, 1, 1, true>(a, stream, cls);
  else return launch_cfg_ks<BM, BN, BK, WM, WN, MAXKS>(a, stream, cls, tiles);
}

// The 32x64 rung over `tiles` 32x64 tiles: no k-split from 768 tiles on (big batched problems: ~90 TFLOP/s)
template <bool BLK>
static int launch_32x64(const GemmArgs& a, hipStream_t stream, long tiles) {
  if (a.Cin % 32 != 0) return launch_rung<BLK, 32, 64, 16, 2, 2, 4>(a, stream, PROF_GEMM_32x64x16, tiles);
  if (tiles >= 768) return launch_rung<BLK, 32, 64, 32, 2, 2, 1>(a, stream, PROF_GEMM_32x64x32, tiles);
  return launch_rung<BLK, 32, 64, 32, 2, 2, 4>(a, stream, PROF_GEMM_32x64x32, tiles);
}

// Shape-to-tile ladder of the LDS-tiled kernel, M rows in each of nseg segments.  BLK: the pack-invariant forms -- the rungs may
// depend on M, because every BLK tile gives a row the same bits.
// Tile choice (tools/conv_bench.py sweep on MI355X, profiles/r01_tile_sweep.txt): these problems are a few GFLOP at most, so what
// matters is an even spread over 1024 SIMDs with several resident workgroups per CU -- small 32x32 tiles, plus intra-workgroup
// split-K when even those are few.  (128x128 tiles lose to 32x64 even at batch scale: profiles/r01_tile_sweep_batch.txt)
template <bool BLK>
static int launch_tiles(const GemmArgs& a, hipStream_t stream, int M, int nseg) {
  const bool k32 = (a.Cin % 32) == 0;
  const long t128 = (long)cdiv(M, 128) * nseg;
  if (a.N <= 16) return launch_rung<BLK, 128, 16, 16, 4, 1, 2>(a, stream, PROF_GEMM_128x16x16, t128);
  if (a.N <= 32 && !a.glu)
    return k32 ? launch_rung<BLK, 128, 32, 32, 4, 1, 2>(a, stream, PROF_GEMM_128x32x32, t128) : launch_rung<BLK, 128, 32, 16, 4, 1, 2>(a, stream, PROF_GEMM_128x32x16, t128);
  if (M <= 16) return k32 ? launch_rung<BLK, 16, 128, 32, 1, 4, 1>(a, stream, PROF_GEMM_16x128x32, 0) : launch_rung<BLK, 16, 128, 16, 1, 4, 1>(a, stream, PROF_GEMM_16x128x16, 0);
  const long t3264 = (long)cdiv(M, 32) * cdiv(a.N, 64) * nseg;
  if (!k32 || a.glu || t3264 >= 768) return launch_32x64<BLK>(a, stream, t3264);
  if constexpr (BLK) return launch_cfg<32, 32, 32, 2, 2, 1, 1, true>(a, stream, PROF_GEMM_32x32x32);
  const long t3232 = (long)cdiv(M, 32) * cdiv(a.N, 32) * nseg;
  const int nk = a.taps * (a.Cin / 32);
  if (t3232 >= 700 || nk < 4) return launch_cfg<32, 32, 32, 2, 2, 1>(a, stream, PROF_GEMM_32x32x32);
  if (t3232 >= 300 || nk < 8) return launch_cfg<32, 32, 32, 2, 2, 2>(a, stream, PROF_GEMM_32x32x32);
  return launch_cfg<32, 32, 32, 2, 2, 4>(a, stream, PROF_GEMM_32x32x32);
}

// What both routes to the no-LDS kernel need of a launch: a plain linear layer with a bias / SiLU / ReLU / alpha / residual epilogue.
// GLU (the conformer conv module's pointwise conv 1): only in its plain form -- no activation, scale or residual on top
static bool plain_linear(const GemmArgs& a) {
  const bool glu_ok = !a.glu || (a.N % 32 == 0 && a.act == ACT_NONE && a.alpha == 1.f && !a.R);
  return a.taps == 1 && a.stride == 1 && a.pad == 0 && glu_ok && a.nseg == 0 && a.chunk == 0 && a.in_act == ACT_NONE && !a.R2 &&
         !a.C2 && a.div == 0.f && (a.act == ACT_NONE || a.act == ACT_SILU || a.act == ACT_RELU) && a.Cin % 64 == 0 && (a.lda & 3) == 0;
}

// CANON_SMALLM: what the no-LDS kernel computes at all (smallm_eligible minus the tuning hooks)
static bool smallm_shape_ok(const GemmArgs& a) {
  return plain_linear(a) && !a.ln_out && a.M > 0 && a.M <= 1024 && (!a.ln_g || a.Cin <= 512);     // (rows = utterances of a lock-step pack: 16-row tiles are independent, any count gives a row the same bits)
}

// Pack-invariant routes (GemmArgs::canon): see gemm.hpp.  Nothing here may make the BITS depend on M; the choice among kernels
// that give the same bits may.
static int launch_canon(const GemmArgs& a, hipStream_t stream) {
  const int M = a.nseg > 0 ? a.max_seg_out : a.M;
  const int nseg = a.nseg > 0 ? a.nseg : 1;
  if (a.ln_out) return SS_ERR_ARG;
  if (a.canon == CANON_SMALLM) {
    if (!smallm_shape_ok(a)) return SS_ERR_ARG;
    if (a.glu) return launch_smallm<2, 2, true>(a, stream, PROF_SMALLM_2x2);
    // split-K form by (N, K) alone: 4 waves on one 16-column tile's k-quarters, or 2 x 2 when N alone fills the chip
    if (a.Cin >= 1024 || a.N <= 4096) return launch_smallm<4, 1>(a, stream, PROF_SMALLM_4x1);
    return launch_smallm<2, 2>(a, stream, PROF_SMALLM_2x2);
  }
  // ---- CANON_SEQ: one accumulator chain per output element ----
  if (a.seg_mb || a.seg_A) {     // per-segment row starts / inputs: one tile form whatever the rows (a row's bits never depend on them)
    if (a.nseg <= 0 || a.ln_g) return SS_ERR_ARG;
    return launch_32x64<true>(a, stream, 0);
  }
  if (rtlin_shape_ok(a) && (a.ln_g || rtlin_eligible(a))) return launch_rtlin(a, stream);
  if (a.ln_g) return SS_ERR_ARG;            // LayerNorm prologue: the row-tile kernel only (K = 256); callers normalise first otherwise
  if (rtlin_kb_eligible(a)) return launch_rtlin_kb(a, stream);      // K = 512 ... : row tile through LDS per 256-wide k-block (same bits as the BLK tiles below)
  // (rounds 4-5 sent big N % 128 == 0 shapes to conv_sk2 cut on whole tiles -- ONE chain over all of K; its 128 accumulator
  //  registers per wave leave no room for the second accumulator set the blocked chain needs, so CANON_SEQ no longer routes there)
  // LDS-tiled kernel, one k-group, blocked chain (BLK)
  return launch_tiles<true>(a, stream, M, nseg);
}

bool smallm_eligible(const GemmArgs& a) {
  if (disp().force_bm > 1) return false;
  const int M = a.nseg > 0 ? a.max_seg_out : a.M;
  // row limit of the no-LDS kernel (Dispatch::smallm_max_rows, SS_SMALLM_MAX_ROWS: tuning knob, tools/latency_breakdown.py): every
  // 16-row tile re-streams its W columns from L2, so it only pays while the whole problem is latency-bound
  // 192: a single utterance of 5-7.7 s (T' = 129..192 encoder rows, a third of the CVSS-C length distribution) keeps its 12 x 9
  // linears on this kernel instead of the 32x32-tile kernel, whose k-loop is one global-load round trip per k-step when a
  // launch is this small: 6.43 -> 6.26 ms per utterance at T' = 131 (tools/b1_profile.py); beyond ~200 rows the re-streaming
  // costs what the tiles' latency did (8.24 vs 8.18 ms at T' = 201 with 256), and the 500-row unit decoder loses 2x.
  return plain_linear(a) && M <= disp().smallm_max_rows && M > 0;
}


int launch_conv_gemm(const GemmArgs& a_in, hipStream_t stream) {
  GemmArgs a = a_in;
  const int M = a.nseg > 0 ? a.max_seg_out : a.M;
  if (M <= 0 || a.N <= 0) return SS_OK;
  if (a.Wf16) return launch_conv_f16(a, stream);      // the opt-in FP16 form (ss_vocoder_set_f16): that kernel or an error, never another path
  if (a.Cin % 16 != 0 || (a.lda & 3) != 0 || a.taps < 1) return SS_ERR_ARG;
  if (a.glu && (a.N % 32 != 0 || a.C2)) return SS_ERR_ARG;
  const bool k32 = (a.Cin % 32) == 0;
  const int nseg = a.nseg > 0 ? a.nseg : 1;
  if (a.canon == CANON_NONE) a.canon = canon_mode();
  if (a.canon != CANON_NONE && !disp().force_bm) { a.m_begin = 0; return launch_canon(a, stream); }
  if (a.seg_mb || a.seg_A) return SS_ERR_ARG;      // the CANON_SEQ tile form only
  if (a.m_begin > 0) {       // a row range of a strided conv (ss_encoder_stream_forward): only the LDS-tile kernel starts anywhere but row 0
    if (a.nseg > 0 || a.m_begin >= a.M || a.ln_g || a.ln_out || a.N <= 32) return SS_ERR_ARG;
    return launch_32x64<false>(a, stream, (long)cdiv(a.M - a.m_begin, 32) * cdiv(a.N, 64));    // (that rung whatever the shape: routing as it was)
  }
  // a forced tile (tuning hook) keeps M <= 4 launches off the GEMV -- except when the caller asked for ln_out, which only the GEMV writes
  if ((!disp().force_bm || a.ln_out) && gemv_eligible(a)) return launch_gemv(a, stream);
  if (a.ln_out) return SS_ERR_ARG;      // only the GEMV form publishes the normalised rows
  if (smallm_eligible(a)) {
    if (a.glu) return launch_smallm<2, 2, true>(a, stream, PROF_SMALLM_2x2);   // value / gate tiles side by side in one workgroup
    const long wgs16 = (long)cdiv(M, 16) * cdiv(a.N, 16);
    if (a.Cin >= 1024 || wgs16 <= 1024) return launch_smallm<4, 1>(a, stream, PROF_SMALLM_4x1);
    if (wgs16 <= 4096) return launch_smallm<2, 2>(a, stream, PROF_SMALLM_2x2);
    return launch_smallm<1, 4>(a, stream, PROF_SMALLM_1x4);
  }
  // 64-channel vocoder stage of a packed batch: input slab in LDS once, W fragments from L2 (conv_c64.hip)
  if (!disp().force_bm && conv_c64_eligible(a)) return conv_c64w_eligible(a) ? launch_conv_c64w(a, stream) : launch_conv_c64(a, stream);
  if (!disp().force_bm && conv_wide_winograd_eligible(a, 128)) return launch_conv_c128w(a, stream);
  if (!disp().force_bm && conv_wide_winograd_eligible(a, 256)) return launch_conv_c256w(a, stream);
  if (!disp().force_bm && conv_c32_eligible(a)) return conv_c32w_eligible(a) ? launch_conv_c32w(a, stream) : launch_conv_c32(a, stream);
  if (!disp().force_bm && conv_c16_eligible(a)) return launch_conv_c16(a, stream);
  // K = 256 linears of packed batches (encoder projections, CTC heads, cross K|V): row tile in LDS, W fragments from L2 (rtlin.hip)
  if (!disp().force_bm && rtlin_eligible(a)) return launch_rtlin(a, stream);
  if (a.ln_g) return SS_ERR_ARG;  // LayerNorm fusion exists only on the small-M and row-tile paths
  if (disp().force_bm == 1 && conv_sk_eligible(a)) return launch_conv_sk(a, stream, disp().force_ks);   // tuning hook: stream-K, grid = ks (0 = auto)
  if (disp().force_bm == 4 && conv_sk2_eligible(a)) return launch_conv_sk2(a, stream, disp().force_ks);  // tuning hook: 2nd-generation stream-K
  if (disp().force_bm == 5 && conv_sk2_eligible(a)) { GemmArgs b = a; b.x3 = 1; return launch_conv_sk2(b, stream, disp().force_ks); }  // ... its split-bf16 variant (tests, tools/sk2_bench.py)
  // Big "same" convs / linears (packed vocoder batches, unit-decoder FFN): persistent stream-K
  // 128-wide tiles, 95-110 TFLOP/s against 75-90 for the 32x64 kernel (profiles/r01_sk_sweep.txt).
  // They need enough k-steps per workgroup to amortise the fix-up + epilogue: >= 12 at BN = 128;
  // at BN = 64 (half the MFMA work per k-step) only the k >= 7 convs qualify.
  if (!disp().force_bm && conv_sk_eligible(a) && 2.0 * (double)a.M * a.N * a.taps * a.Cin >= disp().sk_min_flops) {
    const long long nk = (long long)a.taps * (a.Cin / 32);
    const bool wide = a.N % 128 == 0;
    const long long units = (long long)cdiv(a.M, 128) * (a.N / (wide ? 128 : 64)) * nk;
    const long long min_units = disp().sk_min_units;   // (SS_SK_MIN_UNITS; SS_NO_SK2: first-generation kernel only; SS_SK2_MINK64: smallest taps * Cin for conv_sk2<64>)
    if (!disp().no_sk2 && conv_sk2_eligible(a) && (wide ? units >= min_units : a.taps * a.Cin >= disp().sk2_min_k64)) return launch_conv_sk2(a, stream);
    if (wide ? units >= min_units : a.taps * a.Cin >= 448) return launch_conv_sk(a, stream);
  }
  if (disp().force_bm && a.N > 32 && k32) {   // tuning hook (tools/conv_bench.py): ks = KS*10 + PD
    const int f = disp().force_bm * 10000 + (disp().force_bn % 100) * 100 + disp().force_ks;   // 128x128 -> bn code 28... see cases
    switch (f) {
#define SS_CASE(BM_, BN_, KS_, PD_, CLS_) case BM_ * 10000 + BN_ * 100 + KS_ * 10 + PD_: return launch_cfg<BM_, BN_, 32, 2, 2, KS_, PD_>(a, stream, CLS_);
      SS_CASE(64, 64, 1, 1, PROF_GEMM_64x64x32) SS_CASE(64, 64, 1, 2, PROF_GEMM_64x64x32) SS_CASE(64, 64, 1, 3, PROF_GEMM_64x64x32)
      SS_CASE(64, 64, 2, 2, PROF_GEMM_64x64x32) SS_CASE(64, 64, 2, 3, PROF_GEMM_64x64x32)
      SS_CASE(32, 64, 1, 1, PROF_GEMM_32x64x32) SS_CASE(32, 64, 1, 2, PROF_GEMM_32x64x32) SS_CASE(32, 64, 1, 3, PROF_GEMM_32x64x32) SS_CASE(32, 64, 1, 4, PROF_GEMM_32x64x32)
      SS_CASE(32, 64, 2, 3, PROF_GEMM_32x64x32) SS_CASE(32, 64, 4, 3, PROF_GEMM_32x64x32)
      SS_CASE(32, 32, 1, 1, PROF_GEMM_32x32x32) SS_CASE(32, 32, 1, 2, PROF_GEMM_32x32x32) SS_CASE(32, 32, 1, 3, PROF_GEMM_32x32x32) SS_CASE(32, 32, 1, 4, PROF_GEMM_32x32x32)
      SS_CASE(32, 32, 2, 3, PROF_GEMM_32x32x32) SS_CASE(32, 32, 4, 3, PROF_GEMM_32x32x32)
#undef SS_CASE
      case 128 * 10000 + 28 * 100 + 11: return launch_cfg<128, 128, 16, 2, 2, 1, 1>(a, stream, PROF_GEMM_128x128x16);
      case 128 * 10000 + 64 * 100 + 11: return launch_cfg<128, 64, 32, 2, 2, 1, 1>(a, stream, PROF_GEMM_128x64x32);
      default: break;
    }
  }
  // narrow vocoder stages: weights + input slab in LDS, one HBM pass (conv_slab.hip)
  if (disp().force_bm != 2 && conv_slab_eligible(a) && a.M >= 2048) return launch_conv_slab(a, stream);
  return launch_tiles<false>(a, stream, M, nseg);
}

}  // namespace ss
