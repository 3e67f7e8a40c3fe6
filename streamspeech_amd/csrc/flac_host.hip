// FLAC ingest, host stage: container, metadata chain, frame headers (CRC-8), subframes (Rice / escape residuals) and the frame
// CRC-16 of a native FLAC stream (RFC 9639).  Output: one ss_flac_subframe record per subframe + one int32 per sample, which
// flac.hip turns into PCM on the device; ss_flac_restore_host does the same arithmetic here.  Pure host code: no global mutable
// state (the CRC tables are built once, thread-safely), no HIP runtime call, every read bounds-checked.
#include <string.h>

#include <type_traits>
#include <vector>

#include "../../include/streamspeech_hip.h"
#include "common.hpp"
#include "flac.hpp"

namespace {

struct Crc {
  uint8_t c8[256];
  uint16_t c16[256];
  Crc() {
    for (int i = 0; i < 256; ++i) {
      uint8_t a = (uint8_t)i;
      for (int b = 0; b < 8; ++b) a = (uint8_t)((a & 0x80) ? ((a << 1) ^ 0x07) : (a << 1));
      c8[i] = a;
      uint16_t w = (uint16_t)(i << 8);
      for (int b = 0; b < 8; ++b) w = (uint16_t)((w & 0x8000) ? ((w << 1) ^ 0x8005) : (w << 1));
      c16[i] = w;
    }
  }
};

const Crc& crc() {
  static const Crc t;                                // C++11 magic static: built once, then read-only
  return t;
}

// ---- bit reader over [p, p + n); reading past the end yields zeros and sets `over` ----------------------------------------------
struct Bits {
  const uint8_t* p;
  int64_t nbits, pos;
  bool over = false;
  Bits(const uint8_t* p_, int64_t nbytes, int64_t at_byte) : p(p_), nbits(nbytes * 8), pos(at_byte * 8) {}
  uint32_t get(int n) {                              // 0 <= n <= 32
    if (n == 0) return 0;
    if (pos + n > nbits) { over = true; pos = nbits; return 0; }
    uint64_t v = 0;
    const int64_t b0 = pos >> 3, b1 = (pos + n - 1) >> 3;      // at most 5 bytes
    for (int64_t b = b0; b <= b1; ++b) v = (v << 8) | p[b];
    const int drop = (int)((b1 + 1) * 8 - (pos + n));
    pos += n;
    v >>= drop;
    return (uint32_t)(n == 32 ? v : (v & ((1ull << n) - 1)));
  }
  int32_t sget(int n) {                              // two's complement, n <= 32
    if (n == 0) return 0;
    const uint32_t v = get(n);
    return n == 32 ? (int32_t)v : (int32_t)(v << (32 - n)) >> (32 - n);
  }
  // zeros before the next 1 bit (the 1 is consumed); the end of the data sets `over`
  uint32_t unary() {
    uint32_t q = 0;
    for (;;) {
      if (pos >= nbits) { over = true; return q; }
      const int off = (int)(pos & 7);
      const uint32_t byte = (uint32_t)(p[pos >> 3] << off) & 0xff;           // remaining bits of this byte, left-aligned
      if (byte == 0) { q += 8 - off; pos += 8 - off; continue; }
      const int lead = __builtin_clz(byte) - 24;
      q += lead; pos += lead + 1;
      return q;
    }
  }
  void align() { pos = (pos + 7) & ~(int64_t)7; }
};

const int kFixedTaps[5][4] = {{0, 0, 0, 0}, {1, 0, 0, 0}, {2, -1, 0, 0}, {3, -3, 1, 0}, {4, -6, 4, -1}};

struct Walk {
  ss_flac_info info;
  int64_t n_rec = 0, n_res = 0;
};

int64_t skip_id3v2(const uint8_t* d, size_t n) {
  int64_t at = 0;
  while ((size_t)at + 10 <= n && d[at] == 'I' && d[at + 1] == 'D' && d[at + 2] == '3') {
    if ((d[at + 6] | d[at + 7] | d[at + 8] | d[at + 9]) & 0x80) break;
    const int64_t len = ((int64_t)d[at + 6] << 21) | (d[at + 7] << 14) | (d[at + 8] << 7) | d[at + 9];
    at += 10 + len + ((d[at + 5] & 0x10) ? 10 : 0);            // footer flag
  }
  return at;
}

// marker + metadata chain -> *audio = the first frame's byte offset
int read_metadata(const uint8_t* d, size_t n, ss_flac_info& info, int64_t* audio, bool first_only) {
  memset(&info, 0, sizeof(info));
  int64_t at = skip_id3v2(d, n);
  if (at < 0 || (size_t)at + 4 > n) return SS_ERR_BITSTREAM;
  if (!memcmp(d + at, "OggS", 4)) return SS_ERR_UNSUPPORTED;
  if (memcmp(d + at, "fLaC", 4)) return SS_ERR_BITSTREAM;
  at += 4;
  bool first = true;
  for (;;) {
    if ((size_t)at + 4 > n) return SS_ERR_BITSTREAM;
    const int last = d[at] >> 7, type = d[at] & 0x7f;
    const int64_t len = ((int64_t)d[at + 1] << 16) | (d[at + 2] << 8) | d[at + 3];
    at += 4;
    if ((size_t)(at + len) > n) return SS_ERR_BITSTREAM;
    if (type == 127) return SS_ERR_BITSTREAM;
    if (first) {
      if (type != 0 || len < 34) return SS_ERR_BITSTREAM;       // STREAMINFO is required and comes first
      const uint8_t* s = d + at;
      info.min_block = (s[0] << 8) | s[1];
      info.max_block = (s[2] << 8) | s[3];
      info.sample_rate = (s[10] << 12) | (s[11] << 4) | (s[12] >> 4);
      info.channels = ((s[12] >> 1) & 7) + 1;
      info.bits_per_sample = (((s[12] & 1) << 4) | (s[13] >> 4)) + 1;
      info.total_samples = ((int64_t)(s[13] & 0xf) << 32) | ((int64_t)s[14] << 24) | (s[15] << 16) | (s[16] << 8) | s[17];
      memcpy(info.md5, s + 18, 16);
      if (info.sample_rate == 0) return SS_ERR_BITSTREAM;
      if (info.bits_per_sample > 24) return SS_ERR_UNSUPPORTED;
      if (info.bits_per_sample < 4) return SS_ERR_BITSTREAM;
      first = false;
      if (first_only) { *audio = at + len; return SS_OK; }
    } else if (type == 0) {
      return SS_ERR_BITSTREAM;                                  // a second STREAMINFO
    }
    at += len;
    if (last) break;
  }
  *audio = at;
  return SS_OK;
}

// One frame at byte `at`.  -> SS_OK and *next (a complete frame), kTruncated (drop it and stop), or an SS_ERR_*.
// h_rec / h_res NULL: count only.
const int kTruncated = -1;

int read_frame(const uint8_t* d, size_t n, int64_t at, const ss_flac_info& si, int64_t sample_start, int64_t cap, int64_t res_cap,
               ss_flac_subframe* h_rec, int32_t* h_res, Walk& w, int64_t* next, int32_t* block_out) {
  if ((size_t)at + 2 > n) return kTruncated;
  if (d[at] != 0xff || (d[at + 1] & 0xfe) != 0xf8) return SS_ERR_BITSTREAM;     // sync code 11111111 111110, reserved bit 0
  Bits b(d, (int64_t)n, at);
  b.get(15);
  const int variable = (int)b.get(1);
  const int bs_code = (int)b.get(4), sr_code = (int)b.get(4), ch_code = (int)b.get(4), ss_code = (int)b.get(3);
  const int reserved = (int)b.get(1);
  if (b.over) return kTruncated;
  if (reserved || bs_code == 0 || sr_code == 15 || ch_code > 10 || ss_code == 3) return SS_ERR_BITSTREAM;
  // UTF-8-coded frame (fixed blocking, <= 31 bits) or sample (variable, <= 36 bits) number
  {
    const uint32_t x = b.get(8);
    if (b.over) return kTruncated;
    int extra;
    if (!(x & 0x80)) extra = 0;
    else if ((x & 0xe0) == 0xc0) extra = 1;
    else if ((x & 0xf0) == 0xe0) extra = 2;
    else if ((x & 0xf8) == 0xf0) extra = 3;
    else if ((x & 0xfc) == 0xf8) extra = 4;
    else if ((x & 0xfe) == 0xfc) extra = 5;
    else if (x == 0xfe && variable) extra = 6;
    else return SS_ERR_BITSTREAM;
    for (int i = 0; i < extra; ++i) {
      const uint32_t c = b.get(8);
      if (b.over) return kTruncated;
      if ((c & 0xc0) != 0x80) return SS_ERR_BITSTREAM;
    }
  }
  int32_t block;
  if (bs_code == 1) block = 192;
  else if (bs_code <= 5) block = 576 << (bs_code - 2);
  else if (bs_code == 6) block = (int32_t)b.get(8) + 1;
  else if (bs_code == 7) block = (int32_t)b.get(16) + 1;
  else block = 256 << (bs_code - 8);
  static const int kRates[12] = {0, 88200, 176400, 192000, 8000, 16000, 22050, 24000, 32000, 44100, 48000, 96000};
  int64_t rate;
  if (sr_code < 12) rate = sr_code ? kRates[sr_code] : si.sample_rate;
  else if (sr_code == 12) rate = (int64_t)b.get(8) * 1000;
  else if (sr_code == 13) rate = b.get(16);
  else rate = (int64_t)b.get(16) * 10;
  if (b.over) return kTruncated;
  {
    uint8_t c = 0;
    for (int64_t i = at; i < (b.pos >> 3); ++i) c = crc().c8[c ^ d[i]];
    const uint32_t want = b.get(8);
    if (b.over) return kTruncated;
    if (want != c) return SS_ERR_BITSTREAM;
  }
  static const int kDepth[8] = {0, 8, 12, 0, 16, 20, 24, 32};
  const int depth = ss_code ? kDepth[ss_code] : si.bits_per_sample;
  if (depth > 24) return SS_ERR_UNSUPPORTED;
  const int channels = ch_code < 8 ? ch_code + 1 : 2;
  const int assignment = ch_code < 8 ? SS_FLAC_INDEPENDENT : ch_code - 7;
  if (rate != si.sample_rate || channels != si.channels || depth != si.bits_per_sample) return SS_ERR_BITSTREAM;

  // a frame the buffers have no room for is still walked, without output: only a COMPLETE frame is a capacity error (a truncated
  // last frame is dropped, as it is by the probe that sized the buffers)
  const bool no_room = h_rec && h_res && (w.n_rec + channels > cap || w.n_res + (int64_t)block * channels > res_cap);
  const bool out = h_rec && h_res && !no_room;
  for (int c = 0; c < channels; ++c) {
    const bool side = (assignment == SS_FLAC_LEFT_SIDE && c == 1) || (assignment == SS_FLAC_RIGHT_SIDE && c == 0) ||
                      (assignment == SS_FLAC_MID_SIDE && c == 1);
    ss_flac_subframe rec;
    memset(&rec, 0, sizeof(rec));
    rec.res_offset = w.n_res + (int64_t)c * block;
    rec.sample_start = sample_start;
    rec.block_size = block;
    rec.bps = (uint8_t)(depth + (side ? 1 : 0));
    rec.assignment = (uint8_t)assignment;
    rec.channel = (uint8_t)c;
    int32_t* res = out ? h_res + rec.res_offset : nullptr;
    if (b.get(1)) return b.over ? kTruncated : SS_ERR_BITSTREAM;              // the padding bit
    const int type = (int)b.get(6);
    if (b.get(1)) {
      const uint32_t k = b.unary() + 1;
      if (b.over) return kTruncated;
      if ((int)k >= rec.bps) return SS_ERR_BITSTREAM;
      rec.wasted = (uint8_t)k;
    }
    if (b.over) return kTruncated;
    const int sb = rec.bps - rec.wasted;                                      // bits of a sample as the subframe codes it
    if (type == 0) {
      rec.type = SS_FLAC_CONSTANT;
      const int32_t v = b.sget(sb);
      if (out) { memset(res, 0, sizeof(int32_t) * (size_t)block); res[0] = v; }
    } else if (type == 1) {
      rec.type = SS_FLAC_VERBATIM;
      if (b.pos + (int64_t)sb * block > b.nbits) return kTruncated;
      for (int32_t i = 0; i < block; ++i) { const int32_t v = b.sget(sb); if (out) res[i] = v; }
    } else if ((type & 0x38) == 0x08 || (type & 0x20)) {
      if (type & 0x20) { rec.type = SS_FLAC_LPC; rec.order = (uint8_t)((type & 0x1f) + 1); }
      else { rec.type = SS_FLAC_FIXED; rec.order = (uint8_t)(type & 7); if (rec.order > 4) return SS_ERR_BITSTREAM; }
      const int order = rec.order;
      if (order > block) return SS_ERR_BITSTREAM;
      for (int i = 0; i < order; ++i) { const int32_t v = b.sget(sb); if (out) res[i] = v; }
      if (rec.type == SS_FLAC_LPC) {
        const int prec = (int)b.get(4) + 1;
        if (prec == 16) return b.over ? kTruncated : SS_ERR_BITSTREAM;
        const int32_t shift = b.sget(5);
        if (shift < 0) return b.over ? kTruncated : SS_ERR_BITSTREAM;
        rec.precision = (uint8_t)prec; rec.shift = (uint8_t)shift;
        for (int i = 0; i < order; ++i) rec.coef[i] = (int16_t)b.sget(prec);
      } else {
        rec.precision = 4;
        for (int i = 0; i < order; ++i) rec.coef[i] = (int16_t)kFixedTaps[order][i];
      }
      // residual: coding method, partition order, partitions
      const int method = (int)b.get(2), po = (int)b.get(4);
      if (b.over) return kTruncated;
      if (method > 1) return SS_ERR_BITSTREAM;
      const int pbits = method ? 5 : 4, esc = method ? 31 : 15;
      const int32_t psize = block >> po;
      if (((int64_t)psize << po) != block || psize < order || (po > 0 && psize == 0)) return SS_ERR_BITSTREAM;
      int32_t i = order;
      for (int part = 0; part < (1 << po); ++part) {
        const int32_t cnt = psize - (part == 0 ? order : 0);
        const int k = (int)b.get(pbits);
        if (k == esc) {
          const int nb = (int)b.get(5);
          if (b.pos + (int64_t)nb * cnt > b.nbits) return kTruncated;
          for (int32_t j = 0; j < cnt; ++j, ++i) { const int32_t v = b.sget(nb); if (out) res[i] = v; }
        } else {
          for (int32_t j = 0; j < cnt; ++j, ++i) {
            const uint32_t q = b.unary();
            const uint32_t u = (uint32_t)(((uint64_t)q << k) | b.get(k));
            if (b.over) return kTruncated;
            if (out) res[i] = (int32_t)(u >> 1) ^ -(int32_t)(u & 1);
          }
        }
        if (b.over) return kTruncated;
      }
    } else {
      return SS_ERR_BITSTREAM;                                                // reserved subframe types
    }
    if (b.over) return kTruncated;
    if (out) h_rec[w.n_rec + c] = rec;
  }
  b.align();
  {
    const int64_t end = b.pos >> 3;
    const uint32_t want = b.get(16);
    if (b.over) return kTruncated;
    uint16_t c = 0;
    for (int64_t i = at; i < end; ++i) c = (uint16_t)((c << 8) ^ crc().c16[(c >> 8) ^ d[i]]);
    if (want != c) return SS_ERR_BITSTREAM;
  }
  if (no_room) return SS_ERR_CAPACITY;
  w.n_rec += channels;
  w.n_res += (int64_t)block * channels;
  *next = b.pos >> 3;
  *block_out = block;
  return SS_OK;
}

int walk(const uint8_t* d, size_t n, int64_t cap, int64_t res_cap, ss_flac_subframe* h_rec, int32_t* h_res, ss_flac_info* h_info) {
  if (!d) return SS_ERR_ARG;
  Walk w;
  int64_t at = 0;
  int rc = read_metadata(d, n, w.info, &at, false);
  if (rc) return rc;
  int64_t samples = 0;
  int32_t frames = 0;
  while ((size_t)at < n) {
    int64_t next = at;
    int32_t block = 0;
    rc = read_frame(d, n, at, w.info, samples, cap, res_cap, h_rec, h_res, w, &next, &block);
    if (rc == kTruncated) break;                     // a truncated last frame is dropped
    if (rc) return rc;
    if (frames == 0x7fffffff) return SS_ERR_CAPACITY;
    ++frames;
    samples += block;
    at = next;
  }
  w.info.frames = frames;
  w.info.subframes = w.n_rec;
  w.info.samples = samples;
  if (h_info) *h_info = w.info;
  return SS_OK;
}

template <typename Acc>
void restore_lpc(int32_t* s, const ss_flac_subframe& r) {
  typedef typename std::conditional<sizeof(Acc) == 8, uint64_t, uint32_t>::type U;
  const int order = r.order, n = r.block_size, shift = r.shift;
  for (int i = order; i < n; ++i) {
    U acc = 0;
    for (int j = 0; j < order; ++j) acc += (U)(Acc)r.coef[j] * (U)(Acc)s[i - 1 - j];
    s[i] = flac::add_wrap(s[i], (int32_t)((Acc)acc >> shift));
  }
}

}  // namespace

extern "C" int ss_flac_streaminfo(const uint8_t* h_data, size_t n_bytes, ss_flac_info* h_info) {
  if (!h_data || !h_info) return SS_ERR_ARG;
  int64_t at;
  return read_metadata(h_data, n_bytes, *h_info, &at, true);
}

extern "C" int ss_flac_probe(const uint8_t* h_data, size_t n_bytes, ss_flac_info* h_info) {
  if (!h_data || !h_info) return SS_ERR_ARG;
  return walk(h_data, n_bytes, 0, 0, nullptr, nullptr, h_info);
}

extern "C" int ss_flac_unpack(const uint8_t* h_data, size_t n_bytes, int64_t cap, int32_t* h_res, ss_flac_subframe* h_rec,
                              int64_t res_cap, ss_flac_info* h_info) {
  if (!h_data || !h_res || !h_rec || cap < 0 || res_cap < 0) return SS_ERR_ARG;
  return walk(h_data, n_bytes, cap, res_cap, h_rec, h_res, h_info);
}

extern "C" int ss_flac_restore_host(const int32_t* h_res, const ss_flac_subframe* h_rec, int64_t n_rec, const ss_flac_file* h_files,
                                    int n_files, int mono, float* h_out, int32_t* h_pcm) {
  if (n_files < 0 || n_rec < 0 || (n_files > 0 && (!h_files || !h_res || !h_rec))) return SS_ERR_ARG;
  int64_t pcm_at = 0;
  std::vector<int32_t> buf;
  for (int f = 0; f < n_files; ++f) {
    const ss_flac_file& F = h_files[f];
    if (F.channels < 1 || F.channels > 8 || F.bps < 4 || F.bps > 24 || F.frames < 0 || F.n_out < 0 || F.rec_offset < 0 ||
        F.out_offset < 0 || F.rec_offset + (int64_t)F.frames * F.channels > n_rec)
      return SS_ERR_ARG;
    const int nch = F.channels;
    const float scale = flac::scale_of(F.bps), inv = 1.0f / (float)nch;
    for (int g = 0; g < F.frames; ++g) {
      const ss_flac_subframe* R = h_rec + F.rec_offset + (int64_t)g * nch;
      const int32_t n = R[0].block_size;
      bool ok = true;
      for (int c = 0; c < nch; ++c)
        ok = ok && flac::record_ok(R[c], INT64_MAX, F.n_out) && R[c].block_size == n && R[c].sample_start == R[0].sample_start;
      if (!ok) continue;                              // as the device stage: such a frame writes nothing
      buf.resize((size_t)n * nch);
      for (int c = 0; c < nch; ++c) {
        const ss_flac_subframe& r = R[c];
        int32_t* s = buf.data() + (size_t)c * n;
        const int32_t* src = h_res + r.res_offset;
        if (r.type == SS_FLAC_CONSTANT) { for (int i = 0; i < n; ++i) s[i] = src[0]; }
        else {
          memcpy(s, src, sizeof(int32_t) * (size_t)n);
          if (r.order > 0) { if (flac::needs_wide(r)) restore_lpc<int64_t>(s, r); else restore_lpc<int32_t>(s, r); }
        }
        if (r.wasted) for (int i = 0; i < n; ++i) s[i] = flac::shl_wrap(s[i], r.wasted);
      }
      if (nch == 2)
        for (int i = 0; i < n; ++i) flac::undo_stereo(R[0].assignment, buf[i], buf[n + i], buf[i], buf[n + i]);
      const int64_t t0 = R[0].sample_start;
      for (int i = 0; i < n; ++i) {
        if (h_pcm) for (int c = 0; c < nch; ++c) h_pcm[pcm_at + (int64_t)c * F.n_out + t0 + i] = buf[(size_t)c * n + i];
        if (!h_out) continue;
        if (mono) {
          float acc = (float)buf[i] * scale;
          for (int c = 1; c < nch; ++c) acc += (float)buf[(size_t)c * n + i] * scale;
          h_out[F.out_offset + t0 + i] = nch > 1 ? acc * inv : acc;
        } else {
          for (int c = 0; c < nch; ++c) h_out[F.out_offset + (int64_t)c * F.n_out + t0 + i] = (float)buf[(size_t)c * n + i] * scale;
        }
      }
    }
    pcm_at += (int64_t)F.n_out * nch;
  }
  return SS_OK;
}
