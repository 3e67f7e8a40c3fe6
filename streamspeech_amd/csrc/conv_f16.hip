// Opt-in FP16 matrix-core form of the wide vocoder stages' ResBlock convs (ss_vocoder_set_f16): Cin = N = 64 / 128 / 256, k = 3 / 7 / 11,
// dilation 1 / 3 / 5, "same" rows, single utterance or ragged pack (reference fairseq/models/text_to_speech/hifigan.py:52-172).
//
// Direct-form dilated implicit GEMM on v_mfma_f32_16x16x32_f16: FP16 operands, FP32 accumulation, FP32 tensors in HBM.  The structure
// is that of conv_c64.hip:
//   * persistent workgroups (one per CU), a block of BM output rows at a time; the block's input slab (BM + (k - 1) dil rows x CH
//     channels) goes global -> registers -> [zero padding, input leaky-ReLU, saturation to +-65504, FP16] -> LDS once, so the MFMA
//     loop carries no VALU work; every tap reads the same slab at a row offset;
//   * the weights are converted once per blob (launch_f16_pack) into the MFMA fragment layout: fragment (tap, 32-channel block kb,
//     column tile nt) is 64 lanes x 16 B, lane l holding W[16 nt + (l & 15)][tap * CH + 32 kb + 8 (l >> 4) + 0..7] -- the srcA
//     layout of the 16x16x32 MFMA (cdna_hip_programming.md §3); each wave streams its fragments from L2 into a register ring two
//     k-steps ahead, wrapping into the next block;
//   * 4 waves as WR x WC (rows x columns), each 128 rows (8 row tiles) x 64 columns (4 column tiles): per 32-wide k-step 8 LDS
//     fragments (ds_read_b128) + 4 L2 fragments for 32 MFMAs;
//   * swapped operands D = W . X^T, so a lane ends with 4 consecutive channels of one row: the float4 epilogue of the slab kernels
//     (slab_common.hpp: bias, epilogue leaky-ReLU, residual, MRF sum, mean, pre-activated twin C2).
// Deterministic and pack-invariant: an output element's k walk (tap-major, 32-channel blocks ascending) and its MFMA chain are the
// same wherever its row sits in the block or the pack, and the slab rows outside its utterance read as zero.
#include "slab_common.hpp"

#ifndef F16_FENCE
#define F16_FENCE 1      // as conv_c64.hip: without a fence per step hipcc sinks the weight loads to just before their use
#endif
#if F16_FENCE
#define F16_STEP_FENCE __builtin_amdgcn_sched_barrier(0)
#else
#define F16_STEP_FENCE do { } while (0)
#endif

namespace ss {

using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f16x4 = __attribute__((ext_vector_type(4))) _Float16;
using u32x4 = __attribute__((ext_vector_type(4))) unsigned;

namespace {
constexpr int F16_MAXHALO = 64;                // (taps - 1) * dil <= 64 (k = 11, dil = 5: 50)
constexpr int F16_MAXSEG = 1024;               // segments per launch (larger packs: several launches over slices of the table)
constexpr int F16_WM = 8;                      // 16-row MFMA tiles per wave
constexpr float F16_MAX = 65504.f;

template <int CH>
struct F16Cfg {
  static constexpr int WC = CH / 64;           // waves across the columns (64 columns each)
  static constexpr int WR = 4 / WC;            // ... and across the rows
  static constexpr int BM = WR * F16_WM * 16;  // output rows per block: 512 / 256 / 128 at CH = 64 / 128 / 256
  static constexpr int LDH = CH + 8;           // padded slab row (halves; 16-B aligned rows)
  static constexpr int KB = CH / 32;           // 32-channel k-blocks per tap
  static constexpr int NT = CH / 16;           // column tiles
};

// +-65504 for any finite or infinite input, NaN stays NaN; round to nearest even
__device__ __forceinline__ _Float16 to_f16_sat(float v) {
  v = v > F16_MAX ? F16_MAX : (v < -F16_MAX ? -F16_MAX : v);
  return (_Float16)v;
}
}  // namespace

template <int CH, bool LRELU>
__global__ __launch_bounds__(256, 1) void conv_f16_kernel(const GemmArgs p, const u32x4* __restrict__ Wf, const int slab_rows) {
#if __HIP_DEVICE_COMPILE__
  using Cfg = F16Cfg<CH>;
  constexpr int BM = Cfg::BM, LDH = Cfg::LDH, KB = Cfg::KB, NT = Cfg::NT, WM = F16_WM, C4 = CH / 4;
  extern __shared__ __attribute__((aligned(16))) _Float16 smem_h[];
  _Float16* sA = smem_h;                                                                     // slab [slab_rows][LDH]
  int* s_blk = reinterpret_cast<int*>(smem_h + ((slab_rows * LDH + 7) & ~7));                  // block prefix per segment

  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wr = wave / Cfg::WC, wc = wave % Cfg::WC;
  const int r = lane & 15, g = lane >> 4;
  const int S = p.taps * KB;                   // k-steps per block (even: KB >= 2)

  SlabWalk<GemmArgs> w(p, s_blk, BM);
  __syncthreads();
  const int nblocks = w.nblocks();
  const float slope = p.in_slope;

  // weight fragment of k-step s, column tile j of this wave
  const u32x4* wbase = Wf + (size_t)(wc * 4) * 64 + lane;
  auto wload = [&](int s, int j) -> u32x4 { return wbase[((size_t)s * NT + j) * 64]; };

  int blk = blockIdx.x;
  if (blk >= nblocks) return;
  u32x4 ring[2][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) { ring[0][j] = wload(0, j); ring[1][j] = wload(1, j); }

  for (; blk < nblocks; blk += gridDim.x) {
    w.locate(blk, p.in_len);
    const int m0 = w.m0, seg_lo = w.seg_lo, seg_hi = w.seg_hi;
    const int m_hi = p.nseg > 0 ? seg_hi : min(seg_hi, p.M);
    __syncthreads();                                       // previous block's slab reads are done
    // ---- slab: global -> registers (8 float4 per thread in flight) -> [zero padding, leaky-ReLU, FP16] -> LDS ----
    {
      const int n4 = slab_rows * C4;
      for (int base = t; base < n4; base += 8 * 256) {
        f32x4 pre[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int idx = min(base + u * 256, n4 - 1);
          const int rho = idx / C4, c4 = idx % C4;
          const int gc = min(max(m0 - p.pad + rho, seg_lo), seg_hi - 1);
          pre[u] = *reinterpret_cast<const f32x4*>(p.A + (size_t)gc * p.lda + c4 * 4);
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
          const int idx = base + u * 256;
          if (idx < n4) {
            const int rho = idx / C4, c4 = idx % C4;
            const int gin = m0 - p.pad + rho;
            const bool ok = gin >= seg_lo && gin < seg_hi;
            f16x4 h;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
              float v = ok ? pre[u][e] : 0.f;
              if (LRELU) v = fmaxf(v, v * slope);            // 0 < slope < 1 (checked on the host)
              h[e] = to_f16_sat(v);
            }
            *reinterpret_cast<f16x4*>(sA + rho * LDH + c4 * 4) = h;
          }
        }
      }
    }
    __syncthreads();

    f32x4 acc[WM][4];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const _Float16* pa = sA + (wr * 16 * WM + r) * LDH + 8 * g;    // + i*16*LDH + tap*dil*LDH + kb*32
    const int tap_step = p.dil * LDH;
    auto xoff = [&](int s) { return (s / KB) * tap_step + (s % KB) * 32; };
    f16x8 xa[WM];
#pragma unroll
    for (int i = 0; i < WM; ++i) xa[i] = *reinterpret_cast<const f16x8*>(pa + i * 16 * LDH);
#pragma unroll 1
    for (int s0 = 0; s0 < S; s0 += 2) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        const int s = s0 + h;
        const int sn = s + 1 < S ? s + 1 : s;                        // (after the last step: a harmless re-read)
        f16x8 xb[WM];
        const _Float16* pn = pa + xoff(sn);
#pragma unroll
        for (int i = 0; i < WM; ++i) xb[i] = *reinterpret_cast<const f16x8*>(pn + i * 16 * LDH);
        u32x4 wf[4];
        const int sp = s + 2 < S ? s + 2 : s + 2 - S;                // two steps ahead, wrapping into the next block
#pragma unroll
        for (int j = 0; j < 4; ++j) { wf[j] = ring[h][j]; ring[h][j] = wload(sp, j); }
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8, wf[j]), xa[i], acc[i][j], 0, 0, 0);   // D = W . X^T
#pragma unroll
        for (int i = 0; i < WM; ++i) xa[i] = xb[i];
        F16_STEP_FENCE;
      }
    }

    // ---- epilogue: lane holds channels 64 wc + 16 j + 4g .. +3 of row r of row tile i ----
    int le = lane;
    asm volatile("" : "+v"(le));               // addresses derived from `le` cannot be hoisted above the contraction
    const int r_e = le & 15, g_e = le >> 4;
    const int n_base = wc * 64 + g_e * 4;
    f32x4 bb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      bb[j] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (p.bias) bb[j] = *reinterpret_cast<const f32x4*>(p.bias + n_base + j * 16);
    }
#pragma unroll
    for (int i = 0; i < WM; ++i) {
      const int m = m0 + wr * 16 * WM + i * 16 + r_e;
      const int mc = min(m, m_hi - 1);
      f32x4 rr[4], rr2[4];
      if (p.R) {
#pragma unroll
        for (int j = 0; j < 4; ++j) rr[j] = *reinterpret_cast<const f32x4*>(p.R + (size_t)mc * p.ldr + n_base + j * 16);
      }
      if (p.R2) {
#pragma unroll
        for (int j = 0; j < 4; ++j) rr2[j] = *reinterpret_cast<const f32x4*>(p.R2 + (size_t)mc * p.ldr2 + n_base + j * 16);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const f32x4 v = slab_epi_apply(p, acc[i][j], bb[j], rr[j], rr2[j]);
        if (m < m_hi) slab_epi_store(p, m, n_base + j * 16, v);
      }
    }
  }
#endif
}

// FP32 [CH][taps * CH] (tap-major) -> FP16 fragments [taps][CH / 32][CH / 16][64 lanes][8], saturated like the activations
__global__ void f16_pack_kernel(const float* __restrict__ W, u32x4* __restrict__ Wf, int CH, int taps) {
  const int KB = CH / 32, NT = CH / 16;
  const long long total = (long long)taps * KB * NT * 64;
  const long long q = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= total) return;
  const int lane = (int)(q % 64), nt = (int)(q / 64 % NT), s = (int)(q / 64 / NT);
  const int tap = s / KB, kb = s % KB;
  const int n = nt * 16 + (lane & 15), k0 = tap * CH + kb * 32 + 8 * (lane >> 4);
  f16x8 h;
#pragma unroll
  for (int e = 0; e < 8; ++e) h[e] = to_f16_sat(W[(size_t)n * taps * CH + k0 + e]);
  Wf[q] = __builtin_bit_cast(u32x4, h);
}

// ---- host side ---------------------------------------------------------------------------------
size_t f16_pack_halves(int C, int taps) { return (size_t)taps * C * C; }

int launch_f16_pack(const float* W, void* Wf, int C, int taps, hipStream_t stream) {
  if (!(C == 64 || C == 128 || C == 256) || taps < 1 || !W || !Wf) return SS_ERR_ARG;
  const long long lanes = (long long)taps * (C / 32) * (C / 16) * 64;
  hipLaunchKernelGGL(f16_pack_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, stream, W, reinterpret_cast<u32x4*>(Wf), C, taps);
  SS_LAUNCH_CHECK();
  return SS_OK;
}

bool conv_f16_geometry_ok(int C, int taps, int dil) {
  return (C == 64 || C == 128 || C == 256) && taps >= 1 && dil >= 1 && (long long)(taps - 1) * dil <= F16_MAXHALO;
}

bool conv_f16_eligible(const GemmArgs& a) {
  const int c = a.Cin;
  return a.Wf16 && conv_f16_geometry_ok(c, a.taps, a.dil) && slab_conv_ok(a, c) && a.pad >= 0 && a.pad <= (a.taps - 1) * a.dil && a.nseg >= 0 &&
         (a.nseg > 0 || (a.M == a.in_len && slab_rows_ok(a.M))) && (a.nseg == 0 || (a.segs && slab_rows_ok(a.M)));
}

template <int CH, bool LRELU>
static int launch_f16_t(const GemmArgs& a, hipStream_t stream) {
  constexpr int BM = F16Cfg<CH>::BM;
  const int slab_rows = BM + (a.taps - 1) * a.dil;
  const size_t lds = (size_t)((slab_rows * F16Cfg<CH>::LDH + 7) & ~7) * 2 + (F16_MAXSEG + 2) * sizeof(int);
  SS_MAX_LDS_ONCE((&conv_f16_kernel<CH, LRELU>), 128 * 1024);
  int cus = 0;
  int rc = device_cus(cus);
  if (rc != SS_OK) return rc;
  const ProfCls cls = CH == 64 ? PROF_CONV_F16_64 : CH == 128 ? PROF_CONV_F16_128 : PROF_CONV_F16_256;
  // a pack of more than F16_MAXSEG utterances: one launch per slice of the segment table (segments are independent)
  const int nseg = a.nseg;
  for (int s0 = 0; s0 == 0 || s0 < nseg; s0 += F16_MAXSEG) {
    GemmArgs b = a;
    if (nseg > 0) { b.segs = a.segs + 4 * s0; b.nseg = std::min(F16_MAXSEG, nseg - s0); }
    if (nseg > F16_MAXSEG) b.algo_flops = 2.0 * a.M * a.N * a.taps * a.Cin * b.nseg / nseg;   // (the census: rows of a slice are not known on the host)
    const int grid = slab_grid(1, cus, a.M, BM, b.nseg);
    ProfRec rec{}; bool prof = false;
    rc = prof_begin(b, stream, cls, rec, prof);
    if (rc != SS_OK) return rc;
    hipLaunchKernelGGL((conv_f16_kernel<CH, LRELU>), dim3(grid), dim3(256), lds, stream, b,
                       reinterpret_cast<const u32x4*>(a.Wf16), slab_rows);
    SS_LAUNCH_CHECK();
    rc = prof_end(stream, rec, prof);
    if (rc != SS_OK) return rc;
  }
  return SS_OK;
}

int launch_conv_f16(const GemmArgs& a, hipStream_t stream) {
  if (!conv_f16_eligible(a)) return SS_ERR_ARG;
  const bool lr = a.in_act == ACT_LRELU;
  switch (a.Cin) {
    case 64: return lr ? launch_f16_t<64, true>(a, stream) : launch_f16_t<64, false>(a, stream);
    case 128: return lr ? launch_f16_t<128, true>(a, stream) : launch_f16_t<128, false>(a, stream);
    default: return lr ? launch_f16_t<256, true>(a, stream) : launch_f16_t<256, false>(a, stream);
  }
}

}  // namespace ss
