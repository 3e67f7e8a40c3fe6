// Launch profiler shared by every kernel launcher (prof.hip): optional per-launch timing with HIP events recorded on the launch
// stream (bench.py roofline leg), the always-on launch census and the SS_SHAPE_LOG table.
#pragma once
#include "common.hpp"

namespace ss {

struct GemmArgs;

// Kernel classes, in the order of their names (kTileNames in prof.hip; tests and bench.py look them up by name):
enum ProfCls : int {
  PROF_GEMM_128x16x16 = 0, PROF_GEMM_128x32x32 = 1, PROF_GEMM_128x32x16 = 2, PROF_GEMM_16x128x32 = 3, PROF_GEMM_16x128x16 = 4,
  PROF_GEMM_128x128x16 = 5, PROF_GEMM_128x64x32 = 6, PROF_GEMM_64x64x32 = 7, PROF_GEMM_64x64x16 = 8, PROF_GEMM_32x64x32 = 9,
  PROF_GEMM_32x64x16 = 10, PROF_GEMM_32x32x32 = 11,
  PROF_SMALLM_4x1 = 12, PROF_SMALLM_2x2 = 13, PROF_SMALLM_1x4 = 14,
  PROF_CONV_SK = 15, PROF_CONV_SLAB32 = 16, PROF_CONV_SLAB16 = 17, PROF_CONV_SK2 = 18, PROF_CONV_SK2_BF16X3 = 19,
  PROF_RESBLOCK32 = 20, PROF_RESBLOCK16 = 21, PROF_FFN = 22, PROF_RTLIN = 23,
  PROF_CONV_C64 = 24, PROF_CONV_C32 = 25, PROF_CONV_C16 = 26,
  PROF_CONV_C64W = 27, PROF_CONV_C128W = 28, PROF_CONV_C32W = 29, PROF_CONV_C256W = 30,   // the Winograd forms (prof_begin: issued FLOPs)
  PROF_RTLIN_KB = 31,
  PROF_CONV_F16_64 = 32, PROF_CONV_F16_128 = 33, PROF_CONV_F16_256 = 34,   // the opt-in FP16 form of the wide stages (conv_f16.hip)
};
constexpr int kNumTileCfg = PROF_CONV_F16_256 + 1;
void prof_enable(int cls_mask);   // bit i set -> bracket launches of tile config i (< 32) with events; 0 = off
void prof_enable_hi(int cls_mask);   // the same for tile configs 32 + i
void prof_reset();
int prof_read(int cls, double* ms_total, double* flops_total, long long* launches, double* bytes_total = nullptr);  // synchronises
const char* prof_cfg_name(int cls);
int prof_totals(int cls, double* flops, double* bytes, long long* launches);   // always-on census since library load
int prof_read_issued(int cls, double* issued_flops_total);   // of the bracketed launches: FLOPs the kernel ISSUES as MFMAs (the Winograd forms issue 4 ceil(k/3) / (2 k) of the algorithmic count)
// Per-shape dispatch table (which kernel class took which (N, taps, Cin, operands) shape): SS_SHAPE_LOG=<path> writes it at exit;
// prof_shape_log(1) collects it from now on in-process, prof_shape_dump writes "class N taps Cin operands launches mean_rows
// gflop_per_launch mbyte_per_launch" lines into buf (returns the bytes needed, buf may be null) -- bench.py's `dispatch` object.
void prof_shape_log(int on);
int prof_shape_dump(char* buf, int cap);

// Event-profiler scope shared by every kernel launcher.
struct ProfRec { hipEvent_t e0, e1; double flops, bytes, issued; int cls; };
int prof_begin(const GemmArgs& a, hipStream_t stream, ProfCls cls, ProfRec& rec, bool& prof);
int prof_end(hipStream_t stream, ProfRec& rec, bool prof);

}  // namespace ss
