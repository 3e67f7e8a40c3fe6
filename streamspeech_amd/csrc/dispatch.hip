// Process-wide dispatch state: the Dispatch settings store (dispatch.hpp), the test hooks that edit it, the calling thread's
// pack-invariance mode (CanonScope) and the per-context state that SkScope ties to the store -- the stream-K workspaces and the
// device's CU count (gemm.hpp).
#include "gemm.hpp"

#include <atomic>
#include <cstdlib>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

namespace ss {

// ---- dispatch settings (dispatch.hpp) ---------------------------------------------------------------
namespace {
std::mutex g_disp_mu;
std::atomic<unsigned> g_disp_gen{1};
Dispatch env_defaults() {
  Dispatch d;
  auto I = [](const char* k, int dflt) { const char* e = getenv(k); return e ? atoi(e) : dflt; };
  auto L = [](const char* k, long long dflt) { const char* e = getenv(k); return e ? atoll(e) : dflt; };
  d.attn_split = I("SS_ATTN_NO_SPLIT", 0) ? -1 : 0; d.attn_q16 = I("SS_ATTN_Q16", d.attn_q16);
  d.c16_off = I("SS_NO_CONV_C16", 0) ? 1 : 0; d.c32_off = I("SS_NO_CONV_C32", 0) ? 1 : 0; d.c64_off = I("SS_NO_CONV_C64", 0) ? 1 : 0;
  d.c16_min_rows = L("SS_CONV_C16_MIN_ROWS", d.c16_min_rows); d.c32_min_rows = L("SS_CONV_C32_MIN_ROWS", d.c32_min_rows);
  d.c64_min_rows = L("SS_CONV_C64_MIN_ROWS", d.c64_min_rows);
  d.c64w_on = I("SS_CONV_C64_WINOGRAD", 1); d.c128w_on = I("SS_CONV_C128_WINOGRAD", 1); d.c256w_on = I("SS_CONV_C256_WINOGRAD", 1);
  d.c32w_on = I("SS_CONV_C32_WINOGRAD", 1); d.c64w_min_k = I("SS_CONV_C64_WINOGRAD_MIN_K", 3);
  d.c128w_min_rows = L("SS_CONV_C128_MIN_ROWS", d.c128w_min_rows); d.c256w_min_rows = L("SS_CONV_C256_MIN_ROWS", d.c256w_min_rows);
  if (const int r = I("SS_CONV_C256_ROWS", d.c256w_rows); r == 128 || r == 256) d.c256w_rows = r;
  if (getenv("SS_FFN_WM")) { d.ffn_wm = I("SS_FFN_WM", 3); d.ffn_wm_forced = 1; d.ffn_wm_env = d.ffn_wm; }
  d.ffn_fusion = I("SS_NO_FFN_FUSION", 0) ? 0 : 1; d.ffn_min_rows = I("SS_FFN_MIN_ROWS", d.ffn_min_rows);
  if (getenv("SS_SK_MIN_GFLOP")) d.sk_min_flops = 1e9 * atof(getenv("SS_SK_MIN_GFLOP"));
  d.no_resblock_fusion = I("SS_NO_RESBLOCK_FUSION", 0); d.no_pair_fusion = I("SS_NO_PAIR_FUSION", 0);
  d.rt_off = I("SS_NO_RTLIN", 0) ? 1 : 0; d.rt_min_rows = I("SS_RTLIN_MIN_ROWS", d.rt_min_rows); d.rt_min_units = L("SS_RTLIN_MIN_UNITS", d.rt_min_units);
  d.rt_kb_min_units = L("SS_RTLIN_KB_MIN_UNITS", d.rt_kb_min_units); d.rt_kb_uw = I("SS_RTLIN_KB_UW", d.rt_kb_uw); d.rt_kb_xmap = I("SS_RTLIN_KB_XMAP", d.rt_kb_xmap);
  d.smallm_max_rows = I("SS_SMALLM_MAX_ROWS", d.smallm_max_rows); d.sk_min_units = L("SS_SK_MIN_UNITS", d.sk_min_units);
  d.no_sk2 = I("SS_NO_SK2", 0) ? 1 : 0; d.sk2_min_k64 = I("SS_SK2_MINK64", d.sk2_min_k64); d.sk2_spare_cus = I("SS_SK2_SPARE_CUS", 0);
  d.rt_wg_per_cu = I("SS_RTLIN_WG_PER_CU", 0); d.c32_min_k = I("SS_CONV_C32_MIN_K", d.c32_min_k); d.c16_min_k = I("SS_CONV_C16_MIN_K", d.c16_min_k);
  d.unit_l0_distinct = I("SS_UNIT_L0_DISTINCT", 1) ? 1 : 0; d.fbank_dense = I("SS_FBANK_DENSE", 0) ? 1 : 0;
  return d;
}
Dispatch& process_settings() { static Dispatch d = env_defaults(); return d; }      // (callers hold g_disp_mu)
thread_local const Dispatch* t_disp = nullptr;
thread_local CtxDispatch t_disp_own;          // launches outside any context (ss_op_* unit-test entry points)
}  // namespace
void dispatch_edit(const std::function<void(Dispatch&)>& fn) {
  std::lock_guard<std::mutex> lk(g_disp_mu);
  fn(process_settings());
  g_disp_gen.fetch_add(1, std::memory_order_release);
}
void slab_debug(int grid, long long min_rows) {
  const Dispatch dflt = env_defaults();
  dispatch_edit([=](Dispatch& d) {
    d.slab_grid_cap = grid > 0 ? grid : 0;
    const bool set = min_rows >= 0;
    d.c16_min_rows = set ? min_rows : dflt.c16_min_rows; d.c32_min_rows = set ? min_rows : dflt.c32_min_rows;
    d.c64_min_rows = set ? min_rows : dflt.c64_min_rows;
    d.c128w_min_rows = set ? min_rows : dflt.c128w_min_rows; d.c256w_min_rows = set ? min_rows : dflt.c256w_min_rows;
  });
}
// block height of the 256-channel Winograd form (conv_c64w.hip): 128 or 256; 0 puts the process default back
int conv_c256w_rows_debug(int rows) {
  if (rows != 0 && rows != 128 && rows != 256) return SS_ERR_ARG;
  const int dflt = env_defaults().c256w_rows;
  dispatch_edit([=](Dispatch& d) { d.c256w_rows = rows ? rows : dflt; });
  return SS_OK;
}
const Dispatch* CtxDispatch::refresh() {
  const unsigned now = g_disp_gen.load(std::memory_order_acquire);
  if (gen != now) {
    std::lock_guard<std::mutex> lk(g_disp_mu);
    d = process_settings();
    gen = g_disp_gen.load(std::memory_order_relaxed);
  }
  return &d;
}
const Dispatch& disp() { return t_disp ? *t_disp : *t_disp_own.refresh(); }
DispatchScope::DispatchScope(const Dispatch* d) : prev(t_disp) { t_disp = d; }
DispatchScope::~DispatchScope() { t_disp = prev; }

void debug_force_tile(int bm, int bn, int ks) {
  dispatch_edit([=](Dispatch& d) { d.force_bm = bm; d.force_bn = bn; d.force_ks = ks; d.sk_groups = (bm == 1 && bn == 8); });
}
bool debug_tile_forced() { return disp().force_bm != 0; }

static thread_local int t_canon = CANON_NONE;
CanonScope::CanonScope(int mode) : prev(t_canon) { t_canon = mode; }
CanonScope::~CanonScope() { t_canon = prev; }
int canon_mode() { return t_canon; }
void canon_debug_set(int mode) { t_canon = mode; }

// ---- stream-K workspaces (see gemm.hpp) -----------------------------------------------------------
constexpr size_t SKW_SYNC_BYTES = (16 + 1024) * sizeof(unsigned) + 256;      // >= both kernels' flag tables
static std::mutex g_skw_mu;
static std::vector<SkWorkspace*> g_skw_live;                                 // for the error count only
static std::map<std::pair<int, hipStream_t>, SkWorkspace*> g_skw_fallback;  // launches outside any context scope
static thread_local SkWorkspace* t_skw = nullptr;

SkWorkspace* sk_workspace_new() {
  SkWorkspace* w = new SkWorkspace();
  std::lock_guard<std::mutex> lk(g_skw_mu);
  g_skw_live.push_back(w);
  return w;
}
void sk_workspace_free(SkWorkspace* w) {
  if (!w) return;
  {
    std::lock_guard<std::mutex> lk(g_skw_mu);
    for (size_t i = 0; i < g_skw_live.size(); ++i)
      if (g_skw_live[i] == w) { g_skw_live.erase(g_skw_live.begin() + i); break; }
  }
  if (w->ws) (void)hipFree(w->ws);
  if (w->sync1) (void)hipFree(w->sync1);
  if (w->sync2) (void)hipFree(w->sync2);
  if (w->sync3) (void)hipFree(w->sync3);
  if (w->dbg) (void)hipFree(w->dbg);
  delete w;
}
SkScope::SkScope(SkWorkspace* w) : prev(t_skw), prev_disp(t_disp) { t_skw = w; t_disp = w ? w->disp.refresh() : nullptr; }
SkScope::~SkScope() { t_skw = prev; t_disp = prev_disp; }

int sk_workspace_acquire(hipStream_t stream, SkWorkspace** out) {
  *out = nullptr;
  int dev = 0;
  SS_HIP_CHECK(hipGetDevice(&dev));
  SkWorkspace* w = t_skw;
  if (!w) {
    std::lock_guard<std::mutex> lk(g_skw_mu);
    SkWorkspace*& slot = g_skw_fallback[std::make_pair(dev, stream)];
    if (!slot) { slot = new SkWorkspace(); g_skw_live.push_back(slot); }
    w = slot;
  }
  if (!w->ws) {
    int cus = 0;
    SS_HIP_CHECK(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
    if (cus <= 0) cus = 256;
    if (cus > 512) cus = 512;
    w->dev = dev; w->cus = cus;
    SS_HIP_CHECK(hipMalloc(&w->ws, (size_t)cus * 256 * 128 * sizeof(float)));
    SS_HIP_CHECK(hipMalloc(&w->sync1, SKW_SYNC_BYTES));
    SS_HIP_CHECK(hipMalloc(&w->sync2, SKW_SYNC_BYTES));
    SS_HIP_CHECK(hipMemsetAsync(w->sync1, 0, SKW_SYNC_BYTES, stream));
    SS_HIP_CHECK(hipMemsetAsync(w->sync2, 0, SKW_SYNC_BYTES, stream));
    SS_HIP_CHECK(hipMalloc(&w->sync3, 4096 * sizeof(unsigned)));
    SS_HIP_CHECK(hipMemsetAsync(w->sync3, 0, 4096 * sizeof(unsigned), stream));
    SS_HIP_CHECK(hipStreamSynchronize(stream));   // once per context: a later call may arrive on another stream and must see the zeros
  } else if (w->dev != dev) {
    return SS_ERR_ARG;                 // a context belongs to the device it first ran on
  }
  *out = w;
  return SS_OK;
}

// (the launchers without a stream-K workspace: conv_slab / conv_pair / resblock_fused)
int device_cus(int& cus) {
  static std::mutex mu;
  static int n[128] = {0};
  int dev = 0;
  SS_HIP_CHECK(hipGetDevice(&dev));
  if (dev < 0 || dev >= 128) return SS_ERR_ARG;
  std::lock_guard<std::mutex> lk(mu);
  if (n[dev] == 0) {
    int v = 0;
    SS_HIP_CHECK(hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev));
    n[dev] = v > 0 ? v : 256;
  }
  cus = n[dev];
  return SS_OK;
}

int sk_workspace_error_count() {
  std::lock_guard<std::mutex> lk(g_skw_mu);
  int total = 0;
  for (SkWorkspace* w : g_skw_live)
    for (unsigned* sy : {w->sync1, w->sync2}) {
      unsigned v = 0;
      if (sy && hipMemcpy(&v, sy + 8, sizeof(v), hipMemcpyDeviceToHost) == hipSuccess) total += (int)v;
    }
  return total;
}

}  // namespace ss
