// MP3 ingest, host stage: container, frame headers, side info, bit reservoir, scalefactors and Huffman decoding of MPEG-1 /
// MPEG-2 LSF / MPEG-2.5 Layer III (ISO/IEC 11172-3 §2.4, ISO/IEC 13818-3).  Output: one ss_mp3_granule record + int16 q[576]
// per granule-channel, which mp3.hip turns into PCM on the device.  Pure host code: no global mutable state (the Huffman trees
// are built once, thread-safely, from the constant tables), no HIP runtime call, every read bounds-checked.
#include <string.h>

#include <vector>

#include "../../include/streamspeech_hip.h"
#include "common.hpp"
#include "mp3_tables.hpp"

namespace {

// ---- Huffman trees: node n has children tree[2n], tree[2n+1]; a value >= 0 is a leaf (symbol), < 0 the next node's -index ----
struct HuffTree { std::vector<int32_t> t; };

HuffTree build_tree(const uint16_t* cod, const uint8_t* len, int n) {
  HuffTree h;
  h.t.assign(2, 0x7fffffff);                         // root; 0x7fffffff = no child (an invalid code)
  for (int s = 0; s < n; ++s) {
    int node = 0;
    for (int b = len[s] - 1; b >= 0; --b) {
      int bit = (cod[s] >> b) & 1;
      int32_t& c = h.t[2 * node + bit];
      if (b == 0) { c = s; break; }
      if (c == 0x7fffffff) {
        c = -(int32_t)(h.t.size() / 2);
        h.t.push_back(0x7fffffff); h.t.push_back(0x7fffffff);
      }
      node = -h.t[2 * node + bit];
    }
  }
  return h;
}

struct Trees {
  HuffTree big[32];
  HuffTree quad[2];
  Trees() {
    for (int i = 0; i < 32; ++i) {
      const mp3t::HuffTable& ht = mp3t::kBigValueTables[i];
      if (ht.cod) big[i] = build_tree(ht.cod, ht.len, ht.dim * ht.dim);
    }
    quad[0] = build_tree(mp3t::hA_cod, mp3t::hA_len, 16);
    quad[1] = build_tree(mp3t::hB_cod, mp3t::hB_len, 16);
  }
};

const Trees& trees() {
  static const Trees t;                              // C++11 magic static: built once, then read-only
  return t;
}

// ---- bit reader over [p, p + nbits); reading past the end yields zeros and sets `over` --------------------------------------
struct Bits {
  const uint8_t* p;
  int64_t nbits, pos = 0;
  bool over = false;
  Bits(const uint8_t* p_, int64_t nbytes) : p(p_), nbits(nbytes * 8) {}
  uint32_t get(int n) {
    uint32_t v = 0;
    for (int i = 0; i < n; ++i) {
      int b = 0;
      if (pos < nbits) b = (p[pos >> 3] >> (7 - (pos & 7))) & 1;
      else over = true;
      ++pos;
      v = (v << 1) | (uint32_t)b;
    }
    return v;
  }
  int huff(const HuffTree& h) {
    int node = 0;
    for (int depth = 0; depth < 24; ++depth) {
      int32_t c = h.t[2 * node + (int)get(1)];
      if (c == 0x7fffffff) return -1;
      if (c >= 0) return c;
      node = -c;
    }
    return -1;
  }
};

// ---- frame header ---------------------------------------------------------------------------------------------------------------
struct Hdr {
  int ver;        // 3 = MPEG-1, 2 = MPEG-2, 0 = MPEG-2.5
  int layer;      // 1 = Layer III (the header's code), 2 = II, 3 = I
  int prot, bri, sri, pad, mode, modext, emph;
  int sr_index, nch, ngr, side_len, len;
};

const int kBrMpeg1L3[15] = {0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320};
const int kBrLsfL3[15] = {0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160};

enum { H_OK = 0, H_NOSYNC, H_RESERVED, H_UNSUPPORTED };

int parse_header(const uint8_t* b, Hdr& h) {
  uint32_t v = ((uint32_t)b[0] << 24) | ((uint32_t)b[1] << 16) | ((uint32_t)b[2] << 8) | b[3];
  if ((v >> 21) != 0x7ff) return H_NOSYNC;
  h.ver = (v >> 19) & 3; h.layer = (v >> 17) & 3; h.prot = (v >> 16) & 1; h.bri = (v >> 12) & 15; h.sri = (v >> 10) & 3;
  h.pad = (v >> 9) & 1; h.mode = (v >> 6) & 3; h.modext = (v >> 4) & 3; h.emph = v & 3;
  if (h.ver == 1 || h.layer == 0 || h.bri == 15 || h.sri == 3 || h.emph == 2) return H_RESERVED;
  if (h.layer != 1 || h.bri == 0) return H_UNSUPPORTED;           // Layer I / II, free-format bitrate
  h.sr_index = (h.ver == 3 ? 0 : h.ver == 2 ? 3 : 6) + h.sri;
  h.nch = h.mode == 3 ? 1 : 2;
  h.ngr = h.ver == 3 ? 2 : 1;
  h.side_len = h.ver == 3 ? (h.nch == 1 ? 17 : 32) : (h.nch == 1 ? 9 : 17);
  const int sr = mp3t::kSampleRates[h.sr_index];
  h.len = h.ver == 3 ? 144000 * kBrMpeg1L3[h.bri] / sr + h.pad : 72000 * kBrLsfL3[h.bri] / sr + h.pad;
  return H_OK;
}

bool agrees(const Hdr& a, const Hdr& b) { return a.ver == b.ver && a.sri == b.sri && a.nch == b.nch; }

// ---- the resumable core -----------------------------------------------------------------------------------------------------
// Everything a stream carries between pushes besides its unconsumed bytes; a plain value, so a push works on a copy and commits
// it only when it succeeds.  The whole-file calls run the same code in one pass over the file with finished = true.
constexpr int kMaxFrame = 1441;                      // 320 kbit/s at 32 kHz, or 160 kbit/s at 8 kHz, with padding
constexpr int kReservoir = 511;                      // main_data_begin is 9 bits: nothing further back is ever read

struct Core {
  int64_t id3_skip = 0;           // bytes of an ID3v2 tag still to pass over
  bool tags_done = false;         // the ID3v2 tags at the start are behind us
  bool at_audio_start = true;     // the next header examined is the first one after the tags
  bool have_first = false;
  bool finished = false;
  Hdr first{};
  int delay = -1, padding = -1;
  int join = 0;
  int res_len = 0;                // bytes of main data kept, the last min(received, 511)
  uint8_t res[kReservoir];
  uint8_t sf_prev[2][22];
  int64_t frames = 0, granules = 0, skipped = 0, bytes_in = 0;
  Core() { memset(res, 0, sizeof(res)); memset(sf_prev, 0, sizeof(sf_prev)); }
};

// where the frames of a run go: a scan keeps positions and headers, a decode writes records
struct Scan {
  std::vector<int64_t> pos;       // audio frames
  std::vector<Hdr> hdr;
  int delay = -1, padding = -1;
};

struct Out {
  Scan* scan = nullptr;           // non-NULL: collect, do not decode
  int64_t cap = 0, n_rec = 0;
  int16_t* q = nullptr;
  ss_mp3_granule* rec = nullptr;
  int32_t* bits = nullptr;
};

uint32_t be32(const uint8_t* p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

void fill_info(const Scan& s, ss_mp3_info* info) {
  memset(info, 0, sizeof(*info));
  info->delay = s.delay;
  info->padding = s.padding;
  if (s.hdr.empty()) return;
  const Hdr& h = s.hdr[0];
  info->version = h.ver == 3 ? 1 : h.ver == 2 ? 2 : 25;
  info->sample_rate = mp3t::kSampleRates[h.sr_index];
  info->sr_index = h.sr_index;
  info->channels = h.nch;
  info->frames = (int32_t)s.pos.size();
  info->granules = info->frames * h.ngr;
  info->granule_channels = info->granules * h.nch;
  int64_t total = (int64_t)info->granules * 576, skip = 0, tail = 0;
  if (s.delay >= 0) {
    skip = s.delay + 529;
    tail = s.padding - 529 > 0 ? s.padding - 529 : 0;
  }
  if (skip > total) skip = total;
  info->skip = (int32_t)skip;
  info->samples = total - skip - tail > 0 ? total - skip - tail : 0;
}

// ---- side info ------------------------------------------------------------------------------------------------------------------
struct GrInfo {
  int part2_3, big_values, global_gain, sfc, ws, block_type, mixed, table[3], sbg[3], r0, r1, preflag, sfscale, c1table;
};

const int kSlen1[16] = {0, 0, 0, 0, 3, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4};
const int kSlen2[16] = {0, 1, 2, 3, 0, 1, 2, 3, 1, 2, 3, 1, 2, 3, 2, 3};
// ISO/IEC 13818-3 Table B.1 (no intensity stereo): scalefactor counts per partition, [sfc range][long, short, mixed][4]
const int kLsfNr[3][3][4] = {{{6, 5, 5, 5}, {9, 9, 9, 9}, {6, 9, 9, 9}},
                             {{6, 5, 7, 3}, {9, 9, 12, 6}, {6, 9, 12, 6}},
                             {{11, 10, 0, 0}, {18, 18, 0, 0}, {15, 18, 0, 0}}};

int decode_granule(Bits& br, int64_t end, const GrInfo& g, const Hdr& h, int gr, int ch, const int scfsi[4],
                   uint8_t sf_prev_l[22], int16_t* q, ss_mp3_granule* rec) {
  const Trees& T = trees();
  memset(rec, 0, sizeof(*rec));
  rec->global_gain = (int16_t)g.global_gain;
  rec->scalefac_scale = (uint8_t)g.sfscale;
  rec->block_type = (uint8_t)g.block_type;
  rec->mixed = (uint8_t)g.mixed;
  rec->sr_index = (uint8_t)h.sr_index;
  for (int w = 0; w < 3; ++w) rec->subblock_gain[w] = (uint8_t)g.sbg[w];
  const bool shortb = g.block_type == 2;
  int preflag = g.preflag;
  // -- scalefactors (part 2)
  if (h.ver == 3) {
    const int s1 = kSlen1[g.sfc], s2 = kSlen2[g.sfc];
    if (shortb) {
      if (g.mixed) for (int b = 0; b < 8; ++b) rec->sf_l[b] = (uint8_t)br.get(s1);
      for (int b = g.mixed ? 3 : 0; b < 12; ++b)
        for (int w = 0; w < 3; ++w) rec->sf_s[b][w] = (uint8_t)br.get(b < 6 ? s1 : s2);
    } else {
      static const int kGroup[5] = {0, 6, 11, 16, 21};
      for (int k = 0; k < 4; ++k)
        for (int b = kGroup[k]; b < kGroup[k + 1]; ++b)
          rec->sf_l[b] = (gr == 1 && scfsi[k]) ? sf_prev_l[b] : (uint8_t)br.get(k < 2 ? s1 : s2);
    }
    memcpy(sf_prev_l, rec->sf_l, 22);
  } else {
    int sfc = g.sfc, slen[4], row;
    if (sfc < 400) { slen[0] = (sfc >> 4) / 5; slen[1] = (sfc >> 4) % 5; slen[2] = (sfc & 15) >> 2; slen[3] = sfc & 3; row = 0; preflag = 0; }
    else if (sfc < 500) { sfc -= 400; slen[0] = (sfc >> 2) / 5; slen[1] = (sfc >> 2) % 5; slen[2] = sfc & 3; slen[3] = 0; row = 1; preflag = 0; }
    else { sfc -= 500; slen[0] = sfc / 3; slen[1] = sfc % 3; slen[2] = 0; slen[3] = 0; row = 2; preflag = 1; }
    const int col = shortb ? (g.mixed ? 2 : 1) : 0;
    int k = 0;                                       // running scalefactor index in the granule's order
    for (int part = 0; part < 4; ++part)
      for (int i = 0; i < kLsfNr[row][col][part]; ++i, ++k) {
        uint8_t v = (uint8_t)br.get(slen[part]);
        if (!shortb) rec->sf_l[k] = v;
        else if (g.mixed && k < 6) rec->sf_l[k] = v;
        else {
          int j = g.mixed ? k - 6 + 9 : k;           // mixed: short part starts at band 3
          rec->sf_s[j / 3][j % 3] = v;
        }
      }
  }
  rec->preflag = (uint8_t)preflag;
  // -- Huffman (part 3)
  memset(q, 0, 576 * sizeof(int16_t));
  const int bv2 = g.big_values * 2;
  int r1, r2;
  if (g.ws) {
    r1 = (shortb && !g.mixed) ? mp3t::kSfbShort[h.sr_index][3] * 3 : mp3t::kSfbLong[h.sr_index][8];
    r2 = 576;
  } else {
    int a = g.r0 + 1, b = g.r0 + g.r1 + 2;
    r1 = mp3t::kSfbLong[h.sr_index][a > 22 ? 22 : a];
    r2 = mp3t::kSfbLong[h.sr_index][b > 22 ? 22 : b];
  }
  if (r1 > bv2) r1 = bv2;
  if (r2 > bv2) r2 = bv2;
  int i = 0;
  for (; i < bv2; i += 2) {
    const int t = g.table[i < r1 ? 0 : i < r2 ? 1 : 2];
    if (t == 0) continue;
    const mp3t::HuffTable& ht = mp3t::kBigValueTables[t];
    if (!ht.cod) return SS_ERR_BITSTREAM;            // tables 4 and 14 do not exist
    int s = br.huff(T.big[t]);
    if (s < 0) return SS_ERR_BITSTREAM;
    int x = s / ht.dim, y = s % ht.dim;
    if (ht.linbits && x == 15) x += (int)br.get(ht.linbits);
    if (x && br.get(1)) x = -x;
    if (ht.linbits && y == 15) y += (int)br.get(ht.linbits);
    if (y && br.get(1)) y = -y;
    q[i] = (int16_t)x;
    q[i + 1] = (int16_t)y;
  }
  if (br.pos > end || br.over) return SS_ERR_BITSTREAM;
  while (br.pos < end && i + 4 <= 576) {
    int s = br.huff(T.quad[g.c1table]);
    if (s < 0) return SS_ERR_BITSTREAM;
    int v[4] = {(s >> 3) & 1, (s >> 2) & 1, (s >> 1) & 1, s & 1};
    for (int k = 0; k < 4; ++k)
      if (v[k] && br.get(1)) v[k] = -v[k];
    if (br.pos > end) return SS_ERR_BITSTREAM;       // the last quadruple overran part2_3_length
    for (int k = 0; k < 4; ++k) q[i + k] = (int16_t)v[k];
    i += 4;
  }
  if (br.over) return SS_ERR_BITSTREAM;
  int nz = 576;
  while (nz > 0 && q[nz - 1] == 0) --nz;
  rec->nz = (int16_t)nz;
  (void)ch;
  return SS_OK;
}

// One accepted audio frame `fr` (h.len bytes): side info, reservoir, both granules -> records at o.n_rec.
int decode_frame(Core& c, const Hdr& h, const uint8_t* fr, Out& o) {
  const int crc = h.prot ? 0 : 2;
  Bits si(fr + 4 + crc, h.side_len);
  const bool m1 = h.ver == 3;
  const int mdb = (int)si.get(m1 ? 9 : 8);
  si.get(m1 ? (h.nch == 1 ? 5 : 3) : (h.nch == 1 ? 1 : 2));
  int scfsi[2][4] = {{0}};
  if (m1)
    for (int ch = 0; ch < h.nch; ++ch)
      for (int k = 0; k < 4; ++k) scfsi[ch][k] = (int)si.get(1);
  GrInfo gi[2][2];
  for (int gr = 0; gr < h.ngr; ++gr)
    for (int ch = 0; ch < h.nch; ++ch) {
      GrInfo& g = gi[gr][ch];
      g.part2_3 = (int)si.get(12); g.big_values = (int)si.get(9); g.global_gain = (int)si.get(8);
      g.sfc = (int)si.get(m1 ? 4 : 9); g.ws = (int)si.get(1);
      if (g.ws) {
        g.block_type = (int)si.get(2); g.mixed = (int)si.get(1);
        g.table[0] = (int)si.get(5); g.table[1] = (int)si.get(5); g.table[2] = 0;
        for (int w = 0; w < 3; ++w) g.sbg[w] = (int)si.get(3);
        g.r0 = g.r1 = 0;
        if (g.block_type == 0) return SS_ERR_BITSTREAM;
        if (g.mixed && h.sr_index == 8) return SS_ERR_UNSUPPORTED;    // mixed blocks at 8 kHz: long / short split undefined
      } else {
        g.block_type = 0; g.mixed = 0;
        for (int k = 0; k < 3; ++k) g.table[k] = (int)si.get(5);
        g.r0 = (int)si.get(4); g.r1 = (int)si.get(3);
        g.sbg[0] = g.sbg[1] = g.sbg[2] = 0;
      }
      g.preflag = m1 ? (int)si.get(1) : 0;
      g.sfscale = (int)si.get(1); g.c1table = (int)si.get(1);
      if (g.big_values > 288) return SS_ERR_BITSTREAM;
    }
  // main data of this frame joins the reservoir; this frame's data starts main_data_begin bytes before it.  Only the last 511
  // bytes of the earlier main data can be pointed at, so that is all the reservoir keeps.
  const int md_off = 4 + crc + h.side_len, md_len = h.len - md_off;
  uint8_t md[kReservoir + kMaxFrame];
  memcpy(md, c.res, (size_t)c.res_len);
  memcpy(md + c.res_len, fr + md_off, (size_t)md_len);
  const int total = c.res_len + md_len;
  const int start = c.res_len - mdb;
  const bool decodable = start >= 0;
  if (!decodable && !c.join) return SS_ERR_BITSTREAM;
  if (decodable) {
    const int nrec = h.ngr * h.nch;
    if (o.cap - o.n_rec < nrec) return SS_ERR_CAPACITY;
    Bits br(md, total);
    br.pos = (int64_t)start * 8;
    const bool ms = h.mode == 1 && (h.modext & 2);
    int64_t rec = o.n_rec;
    for (int gr = 0; gr < h.ngr; ++gr)
      for (int ch = 0; ch < h.nch; ++ch, ++rec) {
        const int64_t gstart = br.pos, gend = gstart + gi[gr][ch].part2_3;
        if (gend > br.nbits) return SS_ERR_BITSTREAM;
        int rc = decode_granule(br, gend, gi[gr][ch], h, gr, ch, scfsi[ch], c.sf_prev[ch], o.q + rec * 576, o.rec + rec);
        if (rc != SS_OK) return rc;
        o.rec[rec].ms = ms ? 1 : 0;
        if (o.bits) o.bits[rec] = (int32_t)(br.pos - gstart);
        br.pos = gend;
      }
    o.n_rec = rec;
    ++c.frames;
    c.granules += h.ngr;
  } else {
    ++c.skipped;                                     // joined mid-stream: its main data began before we listened
  }
  const int keep = total < kReservoir ? total : kReservoir;
  memmove(c.res, md + total - keep, (size_t)keep);
  c.res_len = keep;
  return SS_OK;
}

// Advance over d[0, n): the bytes not consumed yet followed by the new ones.  *used = bytes that need not be seen again; the rest
// (fewer than one frame + 4) is what the caller keeps for the next run.  With `finished` nothing more will come.
int run(Core& c, const uint8_t* d, int64_t n, bool finished, Out& o, int64_t* used) {
  int64_t pos = 0;
  *used = 0;
  while (!c.tags_done) {                                                                      // ID3v2 (+ footer)
    if (c.id3_skip > 0) {
      const int64_t take = c.id3_skip < n - pos ? c.id3_skip : n - pos;
      pos += take;
      c.id3_skip -= take;
      if (c.id3_skip > 0) { *used = pos; return SS_OK; }
    }
    if (n - pos < 10) {
      if (!finished) { *used = pos; return SS_OK; }
      c.tags_done = true;
    } else if (d[pos] == 'I' && d[pos + 1] == 'D' && d[pos + 2] == '3') {
      if ((d[pos + 6] | d[pos + 7] | d[pos + 8] | d[pos + 9]) & 0x80) return SS_ERR_BITSTREAM;
      int64_t sz = ((int64_t)d[pos + 6] << 21) | ((int64_t)d[pos + 7] << 14) | ((int64_t)d[pos + 8] << 7) | d[pos + 9];
      c.id3_skip = 10 + sz + ((d[pos + 5] & 0x10) ? 10 : 0);
    } else {
      c.tags_done = true;
    }
  }
  while (pos + 4 <= n) {
    Hdr h;
    int r = parse_header(d + pos, h);
    if (c.at_audio_start) {
      c.at_audio_start = false;
      if (r == H_RESERVED || r == H_UNSUPPORTED) return SS_ERR_UNSUPPORTED;
    }
    if (r != H_OK || (c.have_first && !agrees(h, c.first))) { ++pos; continue; }
    if (pos + h.len > n) {                                                                   // truncated last frame, or not all here yet
      if (finished) pos = n;
      break;
    }
    bool ok = pos + h.len + 4 > n;                                                           // last frame (or < 4 bytes of tail)
    if (ok && !finished) break;                                                              // the look-ahead has not arrived
    if (!ok) {
      Hdr nx;
      ok = parse_header(d + pos + h.len, nx) == H_OK && agrees(h, nx);
    }
    if (!ok) { ++pos; continue; }
    const int crc = h.prot ? 0 : 2;
    if (4 + crc + h.side_len > h.len) { ++pos; continue; }
    if (h.mode == 1 && (h.modext & 1)) return SS_ERR_UNSUPPORTED;                           // intensity stereo
    if (!c.have_first) {
      c.have_first = true;
      c.first = h;
      const uint8_t* x = d + pos + 4 + crc + h.side_len;                                     // Xing / Info frame?
      int64_t room = h.len - (4 + crc + h.side_len);
      if (room >= 8 && (memcmp(x, "Xing", 4) == 0 || memcmp(x, "Info", 4) == 0)) {
        uint32_t flags = be32(x + 4);
        int64_t t = 8 + ((flags & 1) ? 4 : 0) + ((flags & 2) ? 4 : 0) + ((flags & 4) ? 100 : 0) + ((flags & 8) ? 4 : 0);
        if (t + 24 <= room && (memcmp(x + t, "LAME", 4) == 0 || memcmp(x + t, "Lavc", 4) == 0 || memcmp(x + t, "Lavf", 4) == 0)) {
          const uint8_t* q = x + t + 21;
          c.delay = (q[0] << 4) | (q[1] >> 4);
          c.padding = ((q[1] & 15) << 8) | q[2];
        }
        pos += h.len;
        continue;
      }
    }
    if (o.scan) {
      o.scan->pos.push_back(pos);
      o.scan->hdr.push_back(h);
    } else {
      int rc = decode_frame(c, h, d + pos, o);
      if (rc != SS_OK) return rc;
    }
    pos += h.len;
  }
  if (finished) { c.finished = true; pos = n; }
  *used = pos;
  return SS_OK;
}

// ---- whole files: the trailing tags are cut first (they need the end of the data), then one finished run -------------------------
int64_t audio_end(const uint8_t* d, size_t n_bytes) {
  int64_t n = (int64_t)n_bytes, pos = 0;
  while (pos + 10 <= n && d[pos] == 'I' && d[pos + 1] == 'D' && d[pos + 2] == '3') {        // where run() will start the audio
    if ((d[pos + 6] | d[pos + 7] | d[pos + 8] | d[pos + 9]) & 0x80) break;                   // run() refuses it
    int64_t sz = ((int64_t)d[pos + 6] << 21) | ((int64_t)d[pos + 7] << 14) | ((int64_t)d[pos + 8] << 7) | d[pos + 9];
    pos += 10 + sz + ((d[pos + 5] & 0x10) ? 10 : 0);
  }
  int64_t end = n;
  if (end - pos >= 128 && memcmp(d + end - 128, "TAG", 3) == 0) end -= 128;                 // ID3v1
  if (end - pos >= 32 && memcmp(d + end - 32, "APETAGEX", 8) == 0) {                        // APEv2 footer
    const uint8_t* f = d + end - 32;
    int64_t sz = (int64_t)f[12] | ((int64_t)f[13] << 8) | ((int64_t)f[14] << 16) | ((int64_t)f[15] << 24);
    bool has_hdr = (f[23] & 0x80) != 0;
    int64_t cut = sz + (has_hdr ? 32 : 0);
    if (cut >= 32 && cut <= end - pos) end -= cut;
  }
  return end;
}

int scan(const uint8_t* d, size_t n_bytes, Scan& s) {
  Core c;
  Out o;
  o.scan = &s;
  int64_t used;
  int rc = run(c, d, audio_end(d, n_bytes), true, o, &used);
  s.delay = c.delay;
  s.padding = c.padding;
  return rc;
}

int unpack(const uint8_t* d, size_t n_bytes, const Scan& s, int64_t cap, int16_t* h_q, ss_mp3_granule* h_rec, int32_t* h_bits) {
  if (s.hdr.empty()) return SS_OK;
  const Hdr& h0 = s.hdr[0];
  const int64_t need = (int64_t)s.hdr.size() * h0.ngr * h0.nch;
  if (cap < need) return SS_ERR_CAPACITY;
  Core c;
  Out o;
  o.cap = cap; o.q = h_q; o.rec = h_rec; o.bits = h_bits;
  int64_t used;
  return run(c, d, audio_end(d, n_bytes), true, o, &used);
}

void stream_info(const Core& c, int64_t buffered, ss_mp3_stream_info* info) {
  memset(info, 0, sizeof(*info));
  info->delay = c.delay;
  info->padding = c.padding;
  info->buffered = (int32_t)buffered;
  info->finished = c.finished ? 1 : 0;
  info->frames = c.frames;
  info->granules = c.granules;
  info->skipped_frames = c.skipped;
  info->bytes_in = c.bytes_in;
  if (!c.have_first) return;
  const Hdr& h = c.first;
  info->version = h.ver == 3 ? 1 : h.ver == 2 ? 2 : 25;
  info->sample_rate = mp3t::kSampleRates[h.sr_index];
  info->sr_index = h.sr_index;
  info->channels = h.nch;
  if (c.delay >= 0) {
    info->skip = c.delay + 529;
    info->hold = c.padding - 529 > 0 ? c.padding - 529 : 0;
  }
  const int64_t left = c.granules * 576 - info->skip - info->hold;
  info->samples = left > 0 ? left : 0;
}

}  // namespace

struct ss_mp3_stream {
  Core core;
  std::vector<uint8_t> carry;     // unconsumed bytes: fewer than one frame + 4
};

extern "C" int ss_mp3_stream_create(int join, ss_mp3_stream** out) {
  if (!out) return SS_ERR_ARG;
  ss_mp3_stream* s = new ss_mp3_stream();
  s->core.join = join ? 1 : 0;
  *out = s;
  return SS_OK;
}

extern "C" void ss_mp3_stream_destroy(ss_mp3_stream* s) { delete s; }

extern "C" int ss_mp3_stream_reset(ss_mp3_stream* s) {
  if (!s) return SS_ERR_ARG;
  const int join = s->core.join;
  s->core = Core();
  s->core.join = join;
  s->carry.clear();
  return SS_OK;
}

extern "C" int64_t ss_mp3_stream_bound(const ss_mp3_stream* s, size_t n_bytes) {
  if (!s) return 0;
  return 2 * (((int64_t)s->carry.size() + (int64_t)n_bytes) / 24 + 1);
}

extern "C" int ss_mp3_stream_query(const ss_mp3_stream* s, ss_mp3_stream_info* h_info) {
  if (!s || !h_info) return SS_ERR_ARG;
  stream_info(s->core, (int64_t)s->carry.size(), h_info);
  return SS_OK;
}

extern "C" int ss_mp3_stream_copy(ss_mp3_stream* dst, const ss_mp3_stream* src) {
  if (!dst || !src) return SS_ERR_ARG;
  if (dst != src) *dst = *src;
  return SS_OK;
}

extern "C" int ss_mp3_stream_push(ss_mp3_stream* s, const uint8_t* h_data, size_t n_bytes, int finished, int64_t cap, int16_t* h_q,
                                  ss_mp3_granule* h_rec, int32_t* h_bits, int64_t* n_rec, ss_mp3_stream_info* h_info) {
  if (!s || !n_rec || cap < 0 || (n_bytes > 0 && !h_data) || (cap > 0 && (!h_q || !h_rec))) return SS_ERR_ARG;
  *n_rec = 0;
  if (h_info) stream_info(s->core, (int64_t)s->carry.size(), h_info);
  if (s->core.finished) return SS_ERR_ARG;
  // the run sees the kept bytes followed by the chunk; state and bytes are committed only when it succeeds
  const uint8_t* d = h_data;
  int64_t n = (int64_t)n_bytes;
  std::vector<uint8_t> joined;
  if (!s->carry.empty()) {
    joined.reserve(s->carry.size() + n_bytes);
    joined.insert(joined.end(), s->carry.begin(), s->carry.end());
    if (n_bytes) joined.insert(joined.end(), h_data, h_data + n_bytes);
    d = joined.data();
    n = (int64_t)joined.size();
  }
  Core c = s->core;
  Out o;
  o.cap = cap; o.q = h_q; o.rec = h_rec; o.bits = h_bits;
  int64_t used = 0;
  int rc = run(c, d, n, finished != 0, o, &used);
  if (rc != SS_OK) return rc;
  c.bytes_in += (int64_t)n_bytes;
  s->core = c;
  std::vector<uint8_t> rest(d + used, d + n);
  s->carry.swap(rest);
  *n_rec = o.n_rec;
  if (h_info) stream_info(s->core, (int64_t)s->carry.size(), h_info);
  return SS_OK;
}

extern "C" int ss_mp3_probe(const uint8_t* h_data, size_t n_bytes, ss_mp3_info* h_info) {
  if (!h_data || !h_info) return SS_ERR_ARG;
  Scan s;
  int rc = scan(h_data, n_bytes, s);
  if (rc != SS_OK) return rc;
  if (s.pos.empty()) return SS_ERR_BITSTREAM;
  fill_info(s, h_info);
  return SS_OK;
}

extern "C" int ss_mp3_unpack(const uint8_t* h_data, size_t n_bytes, int64_t cap, int16_t* h_q, ss_mp3_granule* h_rec,
                             int32_t* h_bits) {
  if (!h_data || !h_q || !h_rec) return SS_ERR_ARG;
  Scan s;
  int rc = scan(h_data, n_bytes, s);
  if (rc != SS_OK) return rc;
  if (s.pos.empty()) return SS_ERR_BITSTREAM;
  return unpack(h_data, n_bytes, s, cap, h_q, h_rec, h_bits);
}
