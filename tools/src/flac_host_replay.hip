// Host-parser hygiene for the FLAC ingest (csrc/flac_host.hip), run on a CPU under AddressSanitizer + UBSan:
//   hipcc -Xarch_host -fsanitize=address,undefined -O1 -g tools/src/flac_host_replay.hip -o tools/bin/flac_host_replay
//   tools/bin/flac_host_replay tests/golden/flac/libflac_16k_mono.flac
// Replays the stream whole, cut at many lengths, and with a few thousand seeded bit flips through ss_flac_probe, ss_flac_unpack and
// ss_flac_restore_host.  Every input is copied into a heap block of exactly its size and every output buffer has exactly the size
// the probe reports, so a read or write past either end is caught.  No GPU call is made; this is not a pytest and not a GPU job.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../../streamspeech_amd/csrc/flac_host.hip"

static int run(const uint8_t* src, size_t n, long* frames) {
  uint8_t* d = (uint8_t*)malloc(n ? n : 1);
  memcpy(d, src, n);
  ss_flac_info info;
  int rc = ss_flac_probe(d, n, &info);
  if (rc == SS_OK) {
    const int64_t n_res = info.samples * info.channels;
    int32_t* res = (int32_t*)malloc(sizeof(int32_t) * (size_t)(n_res ? n_res : 1));
    ss_flac_subframe* rec = (ss_flac_subframe*)malloc(sizeof(ss_flac_subframe) * (size_t)(info.subframes ? info.subframes : 1));
    ss_flac_info again;
    rc = ss_flac_unpack(d, n, info.subframes, res, rec, n_res, &again);
    if (rc != SS_OK || again.samples != info.samples || again.frames != info.frames) { fprintf(stderr, "probe and unpack disagree: rc %d, %ld/%ld samples, %d/%d frames at %zu bytes\n", rc, (long)again.samples, (long)info.samples, again.frames, info.frames, n); abort(); }
    ss_flac_file f = {0, 0, info.frames, info.channels, info.bits_per_sample, (int32_t)info.samples};
    float* out = (float*)malloc(sizeof(float) * (size_t)(n_res ? n_res : 1));
    int32_t* pcm = (int32_t*)malloc(sizeof(int32_t) * (size_t)(n_res ? n_res : 1));
    if (ss_flac_restore_host(res, rec, info.subframes, &f, 1, 0, out, pcm) != SS_OK) abort();
    if (ss_flac_restore_host(res, rec, info.subframes, &f, 1, 1, out, nullptr) != SS_OK) abort();
    // capacities one short are refused, not overrun
    if (info.subframes > 0 && ss_flac_unpack(d, n, info.subframes - 1, res, rec, n_res, nullptr) != SS_ERR_CAPACITY) abort();
    if (n_res > 0 && ss_flac_unpack(d, n, info.subframes, res, rec, n_res - 1, nullptr) != SS_ERR_CAPACITY) abort();
    *frames += info.frames;
    free(pcm); free(out); free(rec); free(res);
  }
  free(d);
  return rc;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s stream.flac [flips]\n", argv[0]); return 2; }
  FILE* fp = fopen(argv[1], "rb");
  if (!fp) { perror(argv[1]); return 2; }
  std::vector<uint8_t> data;
  uint8_t buf[65536];
  size_t got;
  while ((got = fread(buf, 1, sizeof(buf), fp)) > 0) data.insert(data.end(), buf, buf + got);
  fclose(fp);
  const long flips = argc > 2 ? atol(argv[2]) : 4000;
  long counts[9] = {0}, frames = 0, runs = 0;
  counts[run(data.data(), data.size(), &frames)]++; ++runs;
  if (counts[0] != 1) { fprintf(stderr, "the whole stream is refused\n"); return 1; }
  // truncations: every length through the metadata and the first frames, then a stride, then every length of the tail
  for (size_t n = 0; n < data.size(); n += (n < 6000 || n + 3000 > data.size()) ? 1 : 61) { counts[run(data.data(), n, &frames)]++; ++runs; }
  // seeded single-bit flips (xorshift64), in the whole file, header and metadata included
  uint64_t x = 0x9e3779b97f4a7c15ull;
  std::vector<uint8_t> copy;
  for (long i = 0; i < flips; ++i) {
    x ^= x << 13; x ^= x >> 7; x ^= x << 17;
    const size_t bit = (size_t)(x % (data.size() * 8));
    copy = data;
    copy[bit >> 3] ^= (uint8_t)(0x80 >> (bit & 7));
    if (i % 4 == 0) {                                // some with a second flip close by
      x ^= x << 13; x ^= x >> 7; x ^= x << 17;
      const size_t b2 = (bit + x % 64) % (data.size() * 8);
      copy[b2 >> 3] ^= (uint8_t)(0x80 >> (b2 & 7));
    }
    counts[run(copy.data(), copy.size(), &frames)]++; ++runs;
  }
  printf("%ld runs over %zu bytes: ok %ld, bitstream %ld, unsupported %ld, other %ld; %ld frames decoded\n", runs, data.size(), counts[0],
         counts[SS_ERR_BITSTREAM], counts[SS_ERR_UNSUPPORTED], runs - counts[0] - counts[SS_ERR_BITSTREAM] - counts[SS_ERR_UNSUPPORTED],
         frames);
  return 0;
}
