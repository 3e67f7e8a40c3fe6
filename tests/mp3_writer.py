"""Test-side Layer III stream writer: valid frames from chosen quantised values, scalefactors and side info -- no psychoacoustics.
Main data is one byte stream cut into the frames' payloads, so main_data_begin spans frames whenever earlier frames have room
left (the bit reservoir).  Huffman codes come from csrc/mp3_tables.hpp (the tables under test), parsed by tests/mp3_ref.py.
Covers MPEG-1 / MPEG-2 / MPEG-2.5, mono / stereo / MS, long / start / short / stop / mixed blocks, CRC words, an Info frame with
a LAME tag, ID3v2 / ID3v1 wrapping, and hand-made headers the decoder must refuse."""
import numpy as np

import mp3_ref as R

SR_CODES = {44100: (3, 0), 48000: (3, 1), 32000: (3, 2), 22050: (2, 0), 24000: (2, 1), 16000: (2, 2),
            11025: (0, 0), 12000: (0, 1), 8000: (0, 2)}
BR1 = [0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320]
BR2 = [0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160]
SLEN1 = [0, 0, 0, 0, 3, 1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4]
SLEN2 = [0, 1, 2, 3, 0, 1, 2, 3, 1, 2, 3, 1, 2, 3, 2, 3]
LINBITS = {16: 1, 17: 2, 18: 3, 19: 4, 20: 6, 21: 8, 22: 10, 23: 13, 24: 4, 25: 5, 26: 6, 27: 7, 28: 8, 29: 9, 30: 11, 31: 13}


def _codes(t):
    base = 16 if 16 <= t < 24 else 24 if t >= 24 else t
    return R.table("h%d_cod" % base).astype(int), R.table("h%d_len" % base).astype(int), {1: 2, 2: 3, 3: 3, 5: 4, 6: 4}.get(
        base, 6 if base in (7, 8, 9) else 8 if base in (10, 11, 12) else 16)


class BitWriter:
    def __init__(self):
        self.bits = []

    def put(self, v, n):
        for i in range(n - 1, -1, -1):
            self.bits.append((int(v) >> i) & 1)

    def tobytes(self):
        b = self.bits + [0] * (-len(self.bits) % 8)
        return bytes(int("".join(map(str, b[i:i + 8])), 2) for i in range(0, len(b), 8))


def _table_for(m):
    if m == 0:
        return 0
    for t, lim in ((1, 1), (2, 2), (5, 3), (7, 5), (10, 7), (13, 15)):
        if m <= lim:
            return t
    for t in range(16, 24):
        if m - 15 < (1 << LINBITS[t]):
            return t
    raise ValueError("value too large")


class Granule:
    """One granule-channel as the writer takes it."""

    def __init__(self, q, global_gain=170, block_type=0, mixed=False, sbg=(0, 0, 0), sf_l=None, sf_s=None, scalefac_scale=0,
                 preflag=0, count1table=0, lsf_row=0):
        self.q = np.asarray(q, int)
        self.global_gain, self.block_type, self.mixed, self.sbg = global_gain, block_type, mixed, tuple(sbg)
        self.sf_l = np.zeros(22, int) if sf_l is None else np.asarray(sf_l, int)
        self.sf_s = np.zeros((13, 3), int) if sf_s is None else np.asarray(sf_s, int)
        self.scalefac_scale, self.preflag, self.count1table = scalefac_scale, preflag, count1table
        self.lsf_row = lsf_row                       # LSF only: 0 = scalefac_compress < 400, 1 = 400..499 (preflag: 500..511)


# ISO/IEC 13818-3 scalefactor partitions (no intensity stereo): scalefac_compress < 400 / 400..499 / 500..511 (the last sets
# preflag), [long, short, mixed] counts per partition, and the widest slen each partition can be given in that range
LSF_NR = {0: [[6, 5, 5, 5], [9, 9, 9, 9], [6, 9, 9, 9]], 1: [[6, 5, 7, 3], [9, 9, 12, 6], [6, 9, 12, 6]],
          2: [[11, 10, 0, 0], [18, 18, 0, 0], [15, 18, 0, 0]]}
LSF_MAXSLEN = {0: [4, 4, 3, 3], 1: [4, 4, 3, 0], 2: [3, 2, 0, 0]}


def _lsf_slots(g):
    """(array, index) of every scalefactor an LSF granule carries, in bitstream order."""
    if g.block_type == 2 and g.mixed:
        return [(g.sf_l, (b,)) for b in range(6)] + [(g.sf_s, (b, w)) for b in range(3, 12) for w in range(3)]
    if g.block_type == 2:
        return [(g.sf_s, (b, w)) for b in range(12) for w in range(3)]
    return [(g.sf_l, (b,)) for b in range(21)]


def fit_lsf(g, rng=None):
    """Clip an LSF granule's scalefactors to what its scalefac_compress range can carry (row 2 when preflag is set); with `rng`,
    each partition is clipped to a random narrower width, so scalefac_compress takes many values of its range."""
    row = 2 if g.preflag else g.lsf_row
    col = 2 if (g.block_type == 2 and g.mixed) else 1 if g.block_type == 2 else 0
    slots, k = _lsf_slots(g), 0
    for n, m in zip(LSF_NR[row][col], LSF_MAXSLEN[row]):
        m = int(rng.integers(0, m + 1)) if rng is not None else m
        for a, i in slots[k:k + n]:
            a[i] = min(int(a[i]), (1 << m) - 1)
        k += n
    for a, i in slots[k:]:
        a[i] = 0
    return g


def _encode_granule(g: Granule, sr_index: int, mpeg1: bool):
    """-> (side-info fields dict, main-data BitWriter of part 2 + part 3)."""
    bw = BitWriter()
    shortb, ws = g.block_type == 2, g.block_type != 0
    # ---- part 2: scalefactors
    if mpeg1:
        if shortb:
            vals = ([(g.sf_l[b], 1) for b in range(8)] if g.mixed else []) + \
                   [(g.sf_s[b][w], 1 if b < 6 else 2) for b in range(3 if g.mixed else 0, 12) for w in range(3)]
        else:
            vals = [(g.sf_l[b], 1 if b < 11 else 2) for b in range(21)]
        m1 = max([v for v, k in vals if k == 1] + [0])
        m2 = max([v for v, k in vals if k == 2] + [0])
        sfc = next(i for i in range(16) if (1 << SLEN1[i]) > m1 and (1 << SLEN2[i]) > m2)
        for v, k in vals:
            bw.put(v, SLEN1[sfc] if k == 1 else SLEN2[sfc])
    else:
        row = 2 if g.preflag else g.lsf_row
        col = 2 if (shortb and g.mixed) else 1 if shortb else 0
        seq = [int(a[i]) for a, i in _lsf_slots(g)]
        parts, k = [], 0
        for n in LSF_NR[row][col]:
            parts.append(seq[k:k + n]); k += n
        slen = [int(max(p + [0])).bit_length() for p in parts]
        assert all(sl <= m for sl, m in zip(slen, LSF_MAXSLEN[row])), "scalefactors do not fit: fit_lsf() first"
        if row == 0:
            sfc = ((slen[0] * 5 + slen[1]) << 4) | (slen[2] << 2) | slen[3]
        elif row == 1:
            sfc = 400 + (((slen[0] * 5 + slen[1]) << 2) | slen[2])
        else:
            sfc = 500 + slen[0] * 3 + slen[1]
        for p, sl in zip(parts, slen):
            for v in p:
                bw.put(v, sl)
    part2 = len(bw.bits)
    # ---- part 3: Huffman
    q = g.q
    nzl = int(np.nonzero(q)[0].max()) + 1 if q.any() else 0
    big = int(np.nonzero(np.abs(q) > 1)[0].max()) + 1 if (np.abs(q) > 1).any() else 0
    big += big % 2
    c1_end = big + -(-(nzl - big) // 4) * 4 if nzl > big else big
    assert c1_end <= 576
    sfl, sfs = R.SFB_LONG[sr_index], R.SFB_SHORT[sr_index]
    if ws:
        r1 = sfs[3] * 3 if (shortb and not g.mixed) else sfl[8]
        r2, r0c, r1c = 576, 0, 0
    else:
        r0c, r1c = 7, 7
        r1, r2 = sfl[r0c + 1], sfl[r0c + r1c + 2]
    bounds = [0, min(r1, big), min(r2, big), big]
    tables = [_table_for(int(np.abs(q[bounds[i]:bounds[i + 1]]).max()) if bounds[i + 1] > bounds[i] else 0) for i in range(3)]
    if ws:                                           # two regions: region 1 runs to the end of big_values
        tables = [tables[0], _table_for(int(np.abs(q[bounds[1]:big]).max()) if big > bounds[1] else 0), 0]
    for i in range(0, big, 2):
        reg = 0 if i < r1 else 1 if (i < r2 or ws) else 2
        t = tables[reg]
        if t == 0:
            continue
        cod, ln, dim = _codes(t)
        lb = LINBITS.get(t, 0)
        x, y = abs(q[i]), abs(q[i + 1])
        xi, yi = min(x, 15) if lb else x, min(y, 15) if lb else y
        bw.put(cod[xi * dim + yi], ln[xi * dim + yi])
        if lb and xi == 15:
            bw.put(x - 15, lb)
        if x:
            bw.put(q[i] < 0, 1)
        if lb and yi == 15:
            bw.put(y - 15, lb)
        if y:
            bw.put(q[i + 1] < 0, 1)
    cc, cl = (R.table("hA_cod"), R.table("hA_len")) if g.count1table == 0 else (R.table("hB_cod"), R.table("hB_len"))
    for i in range(big, c1_end, 4):
        v = [abs(int(q[i + k])) if i + k < 576 else 0 for k in range(4)]
        assert max(v) <= 1
        idx = v[0] * 8 + v[1] * 4 + v[2] * 2 + v[3]
        bw.put(int(cc[idx]), int(cl[idx]))
        for k in range(4):
            if v[k]:
                bw.put(q[i + k] < 0, 1)
    side = dict(part2_3=len(bw.bits), big_values=big // 2, global_gain=g.global_gain, sfc=sfc, ws=int(ws),
                block_type=g.block_type, mixed=int(g.mixed), tables=tables, sbg=g.sbg, r0c=r0c, r1c=r1c,
                preflag=g.preflag, sfscale=g.scalefac_scale, c1=g.count1table, part2=part2)
    return side, bw


def _crc16(data_bits):
    crc = 0xFFFF
    for b in data_bits:
        top = (crc >> 15) & 1
        crc = ((crc << 1) & 0xFFFF) ^ (0x8005 if top ^ b else 0)
    return crc


def write_stream(granules, sample_rate=48000, bitrate=None, stereo=False, ms=False, crc=False, lame=None, id3=False):
    """granules: [frame][granule][channel] -> Granule.  lame=(delay, padding) writes an Info frame with a LAME tag first.
    Returns (bytes, sides) where sides[i] is the side-info dict of record i (record order)."""
    ver, sri = SR_CODES[sample_rate]
    mpeg1 = ver == 3
    sr_index = {3: 0, 2: 3, 0: 6}[ver] + sri
    nch = 2 if stereo else 1
    ngr = 2 if mpeg1 else 1
    side_len = (17 if nch == 1 else 32) if mpeg1 else (9 if nch == 1 else 17)
    brs = BR1 if mpeg1 else BR2
    bri = brs.index(bitrate) if bitrate else len(brs) - 1
    spf = 144000 if mpeg1 else 72000
    mode = (1 if ms else 0) if stereo else 3
    modext = 2 if ms else 0
    max_mdb = 511 if mpeg1 else 255

    def header(pad):
        return (0x7FF << 21) | (ver << 19) | (1 << 17) | ((0 if crc else 1) << 16) | (bri << 12) | (sri << 10) | (pad << 9) \
            | (mode << 6) | (modext << 4)

    flen = spf * brs[bri] // sample_rate
    cap = flen - 4 - (2 if crc else 0) - side_len
    frames_out, sides = [], []
    if lame is not None:
        pay = bytearray(flen - 4 - (2 if crc else 0))
        o = side_len
        pay[o:o + 4] = b"Info"; pay[o + 4:o + 8] = (1).to_bytes(4, "big"); pay[o + 8:o + 12] = len(granules).to_bytes(4, "big")
        t = o + 12
        pay[t:t + 9] = b"LAME3.100"
        d, p = lame
        pay[t + 21:t + 24] = bytes([d >> 4, ((d & 15) << 4) | (p >> 8), p & 255])
        h = header(0).to_bytes(4, "big")
        frames_out.append(h + (b"\0\0" if crc else b"") + bytes(pay))
    stream = bytearray()                             # main data of all frames
    consumed = 0                                     # payload bytes of the frames written so far
    side_infos = []
    for fr in granules:
        sw = BitWriter()
        enc = [[_encode_granule(fr[gr][c], sr_index, mpeg1) for c in range(nch)] for gr in range(ngr)]
        P = len(stream)
        if consumed - P > max_mdb:                   # reservoir too deep: stuff
            stream += bytes(consumed - max_mdb - P)
            P = len(stream)
        mdb = consumed - P
        assert 0 <= mdb <= max_mdb
        sw.put(mdb, 9 if mpeg1 else 8)
        sw.put(0, (5 if nch == 1 else 3) if mpeg1 else (1 if nch == 1 else 2))
        if mpeg1:
            sw.put(0, 4 * nch)                       # scfsi
        md = BitWriter()
        for gr in range(ngr):
            for c in range(nch):
                s, bw = enc[gr][c]
                sides.append(s)
                sw.put(s["part2_3"], 12); sw.put(s["big_values"], 9); sw.put(s["global_gain"], 8)
                sw.put(s["sfc"], 4 if mpeg1 else 9); sw.put(s["ws"], 1)
                if s["ws"]:
                    sw.put(s["block_type"], 2); sw.put(s["mixed"], 1); sw.put(s["tables"][0], 5); sw.put(s["tables"][1], 5)
                    for w in range(3):
                        sw.put(s["sbg"][w], 3)
                else:
                    for t in s["tables"]:
                        sw.put(t, 5)
                    sw.put(s["r0c"], 4); sw.put(s["r1c"], 3)
                if mpeg1:
                    sw.put(s["preflag"], 1)
                sw.put(s["sfscale"], 1); sw.put(s["c1"], 1)
                md.bits += bw.bits
        stream += md.tobytes()
        assert len(stream) <= consumed + cap, "frame data does not fit: raise the bitrate"
        si = sw.tobytes()
        assert len(si) == side_len
        side_infos.append(si)
        consumed += cap
    # payloads are cut only now: a frame's main data may start in the payload of an earlier frame
    stream += bytes(max(0, consumed - len(stream)))
    for f, si in enumerate(side_infos):
        h = header(0)
        crcb = b""
        if crc:
            bits = [(h >> i) & 1 for i in range(15, -1, -1)] + [int(b) for byte in si for b in format(byte, "08b")]
            crcb = _crc16(bits).to_bytes(2, "big")
        frames_out.append(h.to_bytes(4, "big") + crcb + si + bytes(stream[f * cap:(f + 1) * cap]))
    data = b"".join(frames_out)
    if id3:
        body = b"TIT2\x00\x00\x00\x05\x00\x00\x00test" + bytes(20)
        n = len(body)
        data = b"ID3\x03\x00\x00" + bytes([(n >> 21) & 127, (n >> 14) & 127, (n >> 7) & 127, n & 127]) + body + data
        data += b"TAG" + b"title".ljust(30, b"\0") + bytes(95)
    return data, sides


def random_granule(rng, block_type=0, mixed=False, nz=400, big=120, gain=165, sf_max=3, sfscale=0, preflag=0, lsf=False,
                   lsf_row=0):
    q = np.zeros(576, int)
    q[:big] = rng.integers(-20, 21, big)
    q[big:nz] = rng.integers(-1, 2, nz - big)
    if rng.random() < 0.5:
        q[rng.integers(0, big)] = int(rng.choice([-1, 1])) * int(rng.integers(16, 300))   # a linbits value
    sf_l = rng.integers(0, sf_max + 1, 22); sf_l[21] = 0
    sf_s = rng.integers(0, sf_max + 1, (13, 3)); sf_s[12] = 0
    if block_type == 2:
        if mixed:
            sf_l[6 if lsf else 8:] = 0
            sf_s[:3] = 0
        else:
            sf_l[:] = 0
    else:
        sf_s[:] = 0
    g = Granule(q, gain, block_type, mixed, tuple(int(v) for v in rng.integers(0, 3, 3)) if block_type == 2 else (0, 0, 0),
                sf_l, sf_s, sfscale, preflag, int(rng.integers(0, 2)), lsf_row)
    return fit_lsf(g, rng) if lsf else g


def sequence(rng, n_frames, ngr, nch, blocks=None, **kw):
    """[frame][granule][channel] granules; `blocks` is a list of (block_type, mixed) per granule (cycled), both channels alike."""
    blocks = blocks or [(0, False)]
    out, k = [], 0
    for _ in range(n_frames):
        fr = []
        for _ in range(ngr):
            bt, mx = blocks[k % len(blocks)]
            k += 1
            fr.append([random_granule(rng, bt, mx, **kw) for _ in range(nch)])
        out.append(fr)
    return out


def raw_header(ver=3, layer=1, bri=5, sri=1, mode=3, modext=0, prot=1):
    return ((0x7FF << 21) | (ver << 19) | (layer << 17) | (prot << 16) | (bri << 12) | (sri << 10) | (mode << 6) | (modext << 4)).to_bytes(4, "big")


def catalogue():
    """The writer streams of the tests: name -> (bytes, sides, granules [frame][gr][ch], sample rate, channels, lame)."""
    rng = np.random.default_rng(1234)
    cyc = [(0, False), (1, False), (2, False), (3, False)]
    specs = {
        "mpeg1_stereo_ms": dict(sr=48000, nch=2, ms=True, blocks=cyc, kw=dict(preflag=1, sfscale=1)),
        "mpeg1_mixed": dict(sr=44100, nch=1, blocks=[(2, True), (0, False), (2, True), (2, False)], kw=dict(preflag=1)),
        "mpeg2_24k": dict(sr=24000, nch=2, blocks=cyc, kw=dict(lsf=True)),
        "mpeg2_16k_mixed": dict(sr=16000, nch=1, blocks=[(2, True), (0, False), (2, False)], kw=dict(lsf=True, sfscale=1)),
        "mpeg25_8k": dict(sr=8000, nch=1, blocks=[(0, False), (1, False), (2, False), (3, False)], kw=dict(lsf=True)),
        "mpeg25_12k_stereo_ms": dict(sr=12000, nch=2, ms=True, blocks=[(0, False)], kw=dict(lsf=True)),
        "crc_32k": dict(sr=32000, nch=1, crc=True, blocks=cyc),
        "lame_gapless": dict(sr=48000, nch=1, lame=(576, 1200), blocks=[(0, False)]),
        "id3_wrapped": dict(sr=48000, nch=1, id3=True, blocks=[(0, False)]),
        "mpeg2_22k_sfc400": dict(sr=22050, nch=1, blocks=[(0, False), (2, False), (2, True), (3, False)],
                                 kw=dict(lsf=True, lsf_row=1, sf_max=15)),
        "mpeg25_11k_preflag_ms": dict(sr=11025, nch=2, ms=True, blocks=[(0, False), (2, True), (2, False), (1, False)],
                                      kw=dict(lsf=True, preflag=1, sf_max=7)),
    }
    out = {}
    for name, sp in specs.items():
        ngr = 2 if sp["sr"] >= 32000 else 1
        gr = sequence(rng, 6, ngr, sp["nch"], sp["blocks"], **sp.get("kw", {}))
        data, sides = write_stream(gr, sp["sr"], stereo=sp["nch"] == 2, ms=sp.get("ms", False), crc=sp.get("crc", False),
                                   lame=sp.get("lame"), id3=sp.get("id3", False))
        out[name] = (data, sides, gr, sp["sr"], sp["nch"], sp.get("lame"))
    return out
