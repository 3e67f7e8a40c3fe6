// Dispatch settings: every tuning / A-B knob and test hook that decides WHICH kernel a launch takes.
//
// Through round 4 these were ~30 plain file-scope globals (`static int g_... = getenv(...)`) written by the ss_debug_* test hooks
// and read by every launching thread.  Now:
//   * `Dispatch` is one plain struct; the PROCESS settings (environment defaults + whatever the ss_debug_* hooks edited) live
//     behind a mutex and carry a generation number;
//   * every execution context (ss_model / ss_vocoder: one host thread at a time, by the C ABI's contract) owns a private COPY,
//     refreshed only at the start of an entry point and only if the generation moved -- never in the middle of a call; the
//     launchers read the calling thread's scoped copy (`disp()`), i.e. memory no other thread writes;
//   * launches outside any context (the ss_op_* unit-test entry points) read a thread-local copy kept the same way.
// Environment variables are read ONCE, when the process settings are first touched.
#pragma once
#include <functional>

namespace ss {

struct Dispatch {
  // attention.hip
  int attn_no_mfma = 0;            // test hook: plain attention on the VALU kernel
  int attn_q16 = 1;                // SS_ATTN_Q16=0: rel-pos attention of <= 48 query rows on the 64-query tile kernel instead of attention_relpos_q16_kernel
  int attn_split = 0;              // -1 never split keys, 0 heuristic, n > 0 key tiles per split        SS_ATTN_NO_SPLIT
  // per-conv slab kernels of the vocoder stages (conv_c16 / c32 / c64.hip) and their Winograd forms (conv_c64w.hip)
  int c16_off = 0, c32_off = 0, c64_off = 0;                                          // SS_NO_CONV_C16 / C32 / C64
  long long c16_min_rows = 131072, c32_min_rows = 65536, c64_min_rows = 32768;        // SS_CONV_C16 / C32 / C64_MIN_ROWS
  int c64w_on = 1, c128w_on = 1, c256w_on = 1, c32w_on = 1;                           // SS_CONV_C64 / C128 / C256 / C32_WINOGRAD
  int c64w_min_k = 3;                                                                 // SS_CONV_C64_WINOGRAD_MIN_K
  long long c128w_min_rows = 65536, c256w_min_rows = 32768;                           // SS_CONV_C128 / C256_MIN_ROWS
  int c256w_rows = 128;            // SS_CONV_C256_ROWS / ss_debug_conv_c256_rows: block height of the 256-channel Winograd form, 128 (all 256 columns, one workgroup) or 256 (two workgroups by column half)
  int c32_min_k = 7, c16_min_k = 11;   // SS_CONV_C32 / C16_MIN_K: smallest kernel size whose ResBlock convs run conv by conv instead of as one fused launch (vocoder.hip)
  int slab_grid_cap = 0;           // test hook (ss_debug_slab): > 0 caps the persistent grid of every slab kernel (slab_grid, gemm.hpp)
  // conv_sk.hip
  int sk_groups = 0;               // XCD tile grouping of the first-generation stream-K kernel (tuning hook)
  // conv_sk2.hip
  int sk2_spare_cus = 0;           // SS_SK2_SPARE_CUS: CUs left without a workgroup (tuning knob, measured flat)
  // ffn.hip / encoder FFN routing
  int ffn_force_g = 0;             // fixed grid (tests)
  int ffn_wm = 3, ffn_wm_forced = 0;   // 16-row MFMA tiles per wave; forced by SS_FFN_WM / ss_debug_ffn
  int ffn_wm_env = 0;              // SS_FFN_WM as read at start-up (0: unset): what ss_debug_ffn(rows = 0) puts back
  int ffn_fusion = 1;              // SS_NO_FFN_FUSION
  int ffn_min_rows = 1000;         // SS_FFN_MIN_ROWS
  // gemm.hip
  int force_bm = 0, force_bn = 0, force_ks = 0;   // ss_debug_force_tile
  double sk_min_flops = 4e9;       // SS_SK_MIN_GFLOP
  int smallm_max_rows = 192;       // SS_SMALLM_MAX_ROWS: row limit of the no-LDS small-M kernel (smallm_eligible)
  long long sk_min_units = 12 * 512;   // SS_SK_MIN_UNITS: (tile, k-step) units from which an N % 128 == 0 shape goes to stream-K
  int no_sk2 = 0;                  // SS_NO_SK2: A/B knob, first-generation stream-K kernel only
  int sk2_min_k64 = 192;           // SS_SK2_MINK64: N % 128 == 64, smallest taps * Cin for conv_sk2<64>
  // vocoder ResBlock fusion (model.hip)
  int no_resblock_fusion = 0, no_pair_fusion = 0;   // SS_NO_RESBLOCK_FUSION / SS_NO_PAIR_FUSION, ss_debug_force_tile(6 | 3)
  // rtlin.hip
  int rt_off = 0, rt_min_rows = 193, rt_force_g = 0;   // SS_NO_RTLIN, SS_RTLIN_MIN_ROWS, ss_debug_rtlin
  long long rt_min_units = 4000;                       // SS_RTLIN_MIN_UNITS
  int rt_wg_per_cu = 0;                                // SS_RTLIN_WG_PER_CU: resident rt_linear workgroups per CU (0: by the launch's unit count)
  long long rt_kb_min_units = 256;                     // SS_RTLIN_KB_MIN_UNITS: (48-row tile, 64-column group) units from which rt_linear_kb takes a K > 256 linear
  int rt_kb_xmap = 1;                                  // SS_RTLIN_KB_XMAP: 0 = every workgroup walks a contiguous (tile, column group) range; 1 = the column groups of a row tile run side by side on one XCD
  int rt_kb_uw = 0;                                    // SS_RTLIN_KB_UW / ss_debug_rtlin_kb: 16-column units per wave and column group (0: by the launch's unit count; 1 / 2 / 4 force)
  int rt_kb_order = 1;                                 // test hook (ss_debug_rtlin_kb): 0 contiguous unit ranges, 1 by the launch (rt_kb_xmap and its conditions), 2 the XCD-aware order or SS_ERR_ARG
  // work the outputs never see (batch.hip, fbank.hip): both switches give the same bits
  int unit_l0_distinct = 1;        // SS_UNIT_L0_DISTINCT=0 / ss_debug_unit_l0_distinct: LayerNorm + QKV of the unit decoder's first layer over all 25 n upsampled rows instead of the n distinct ones (pack-invariant packs only; otherwise always all rows)
  int fbank_dense = 0;             // SS_FBANK_DENSE=1 / ss_debug_fbank_dense: every mel row walks all 257 bins and the FFT twiddles come from sincospif in the kernel, instead of the model's FbankTables
};

// The calling thread's settings: the scoped context's private copy, else this thread's own copy of the process settings.
const Dispatch& disp();
// ss_debug_* hooks: edit the process settings (under the lock; bumps the generation -- contexts pick the edit up at their next call)
void dispatch_edit(const std::function<void(Dispatch&)>& fn);

// A context's private copy (member of SkWorkspace: every ss_model / ss_vocoder has one).
struct CtxDispatch {
  Dispatch d;
  unsigned gen = 0xffffffffu;
  const Dispatch* refresh();       // re-copy iff the process generation moved; returns &d
};
struct DispatchScope {             // RAII: disp() of the calling thread = *d until the scope ends
  explicit DispatchScope(const Dispatch* d);
  ~DispatchScope();
  const Dispatch* prev;
};

}  // namespace ss
