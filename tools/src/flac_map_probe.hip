// Which mapping restores FLAC subframes faster at the bench shape (2,500 subframes of 4,096 samples, tools/flac_bench.py)?
//   wave: one wave per subframe, the taps across lanes, DPP reduction -- the kernel of csrc/flac.hip, included here as it is;
//   lane: one lane per subframe, the history in registers, instantiated per compile-time order bucket (written here only).
// The integer work does not depend on the data, so the records are synthetic: every subframe LPC of one order, 16-bit residuals.
// Both mappings must give the same samples.  Prints one line per order with the median of 20 timed launches each.
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/src/flac_map_probe.hip -o tools/bin/flac_map_probe
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "../../streamspeech_amd/csrc/flac.hip"

template <int ORD, typename U, typename S>
__global__ __launch_bounds__(64) void lane_kernel(const int32_t* __restrict__ res, const ss_flac_subframe* __restrict__ rec,
                                                  int n_rec, int32_t* __restrict__ work) {
  const int idx = blockIdx.x * 64 + threadIdx.x;
  if (idx >= n_rec) return;
  const ss_flac_subframe r = rec[idx];
  const int n = r.block_size, order = r.order, shift = r.shift;
  const int32_t* src = res + r.res_offset;
  int32_t* dst = work + r.res_offset;
  int32_t c[ORD], h[ORD];
#pragma unroll
  for (int j = 0; j < ORD; ++j) { c[j] = j < order ? r.coef[j] : 0; h[j] = 0; }
  for (int i = 0; i < n; ++i) {
    U acc = 0;
#pragma unroll
    for (int j = 0; j < ORD; ++j) acc += (U)(S)c[j] * (U)(S)h[j];
    const int32_t rv = src[i];
    const int32_t v = i < order ? rv : flac::add_wrap(rv, (int32_t)((S)acc >> shift));
#pragma unroll
    for (int j = ORD - 1; j > 0; --j) h[j] = h[j - 1];
    h[0] = v;
    dst[i] = v;
  }
}

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

template <class F>
static int time_ms(F launch, float* med) {
  hipEvent_t e0, e1;
  CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
  for (int i = 0; i < 3; ++i) launch();
  CHECK(hipDeviceSynchronize());
  std::vector<float> t;
  for (int i = 0; i < 20; ++i) {
    CHECK(hipEventRecord(e0, 0));
    launch();
    CHECK(hipEventRecord(e1, 0));
    CHECK(hipEventSynchronize(e1));
    float ms;
    CHECK(hipEventElapsedTime(&ms, e0, e1));
    t.push_back(ms);
  }
  CHECK(hipGetLastError());
  std::sort(t.begin(), t.end());
  *med = t[t.size() / 2];
  return 0;
}

int main() {
  const int n_rec = 2500, block = 4096;
  const int64_t n_res = (int64_t)n_rec * block;
  std::vector<int32_t> res(n_res);
  uint64_t x = 88172645463325252ull;
  for (auto& v : res) { x ^= x << 13; x ^= x >> 7; x ^= x << 17; v = (int32_t)(x % 2001) - 1000; }
  int32_t *d_res, *d_work, *d_work2;
  ss_flac_subframe* d_rec;
  float* d_out;
  void* d_tab;
  CHECK(hipMalloc(&d_res, n_res * 4)); CHECK(hipMalloc(&d_work, n_res * 4)); CHECK(hipMalloc(&d_work2, n_res * 4));
  CHECK(hipMalloc(&d_rec, sizeof(ss_flac_subframe) * n_rec)); CHECK(hipMalloc(&d_out, n_res * 4)); CHECK(hipMalloc(&d_tab, 4096));
  CHECK(hipMemcpy(d_res, res.data(), n_res * 4, hipMemcpyHostToDevice));
  for (int order : {4, 8, 12, 32}) {
    for (int wide = 0; wide < 2; ++wide) {
      std::vector<ss_flac_subframe> rec(n_rec);
      for (int i = 0; i < n_rec; ++i) {
        ss_flac_subframe& r = rec[i];
        memset(&r, 0, sizeof(r));
        r.res_offset = (int64_t)i * block; r.sample_start = (int64_t)i * block; r.block_size = block; r.type = SS_FLAC_LPC; r.order = (uint8_t)order;
        r.bps = wide ? 24 : 16; r.shift = 12; r.precision = wide ? 15 : 11;
        for (int j = 0; j < order; ++j) r.coef[j] = (int16_t)((j % 2 ? -1 : 1) * (2000 / (j + 2)));   // 11 bits; sum |c| < 2^12: stable
      }
      if (flac::needs_wide(rec[0]) != (wide != 0)) { fprintf(stderr, "width rule\n"); return 1; }
      CHECK(hipMemcpy(d_rec, rec.data(), sizeof(ss_flac_subframe) * n_rec, hipMemcpyHostToDevice));
      // the library's kernel over one mono file
      std::vector<ss_flac_file> files(1);
      files[0] = {0, 0, n_rec, 1, wide ? 24 : 16, (int32_t)n_res};   // one file of 2,500 frames
      std::vector<int64_t> gpre = {0, n_rec};
      CHECK(hipMemcpy(d_tab, files.data(), sizeof(ss_flac_file), hipMemcpyHostToDevice));
      CHECK(hipMemcpy((char*)d_tab + 256, gpre.data(), 16, hipMemcpyHostToDevice));
      float wave_ms = 0, lane_ms = 0;
      if (time_ms([&] {
            hipLaunchKernelGGL(flac_restore_kernel, dim3(n_rec), dim3(64), 0, 0, d_res, d_rec, n_res, (const FileDev*)d_tab,
                               (const int64_t*)((char*)d_tab + 256), 1, 1, d_work, d_out);
          }, &wave_ms)) return 1;
      auto lane = [&] {
        const dim3 g((n_rec + 63) / 64), b(64);
#define LANE(ORD)                                                                                                      \
  if (wide) hipLaunchKernelGGL((lane_kernel<ORD, uint64_t, int64_t>), g, b, 0, 0, d_res, d_rec, n_rec, d_work2);        \
  else hipLaunchKernelGGL((lane_kernel<ORD, uint32_t, int32_t>), g, b, 0, 0, d_res, d_rec, n_rec, d_work2)
        if (order <= 4) { LANE(4); } else if (order <= 8) { LANE(8); } else if (order <= 12) { LANE(12); } else { LANE(32); }
#undef LANE
      };
      if (time_ms(lane, &lane_ms)) return 1;
      std::vector<int32_t> a(n_res), b(n_res);
      CHECK(hipMemcpy(a.data(), d_work, n_res * 4, hipMemcpyDeviceToHost));
      CHECK(hipMemcpy(b.data(), d_work2, n_res * 4, hipMemcpyDeviceToHost));
      printf("order %2d %s accumulator: wave-per-subframe %.3f ms (with decorrelation + float store), lane-per-subframe %.3f ms, samples %s\n",
             order, wide ? "64-bit" : "32-bit", wave_ms, lane_ms, a == b ? "equal" : "DIFFER");
    }
  }
  return 0;
}
