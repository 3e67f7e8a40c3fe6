"""A FLAC encoder for tests: integer samples in, a valid native FLAC stream out, with every coding choice in the caller's hand
(block sizes and blocking strategy; subframe type, order, coefficients, precision and shift; partition order, Rice parameters and
method, escape partitions; wasted bits; channel assignment; both CRCs).  It makes no attempt to compress well: it exists so that
the decoder (streamspeech_amd/flac.py) can be driven through every path of the format (RFC 9639) on streams whose PCM is known.
Exact Python integers throughout."""
import hashlib

INDEPENDENT, LEFT_SIDE, RIGHT_SIDE, MID_SIDE = 0, 1, 2, 3
FIXED_TAPS = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}
RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
DEPTH_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6}


def crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xff if c & 0x80 else (c << 1) & 0xff
    return c


def crc16(data: bytes) -> int:
    c = 0
    for b in data:
        c ^= b << 8
        for _ in range(8):
            c = ((c << 1) ^ 0x8005) & 0xffff if c & 0x8000 else (c << 1) & 0xffff
    return c


class BitWriter:
    def __init__(self):
        self.parts = []

    def put(self, value: int, n: int):
        if n:
            assert 0 <= value < (1 << n), (value, n)
            self.parts.append(format(value, "0%db" % n))

    def sput(self, value: int, n: int):
        if n:
            assert -(1 << (n - 1)) <= value < (1 << (n - 1)), (value, n)
            self.put(value & ((1 << n) - 1), n)

    def unary(self, q: int):
        self.parts.append("0" * q + "1")

    def align(self):
        n = sum(len(p) for p in self.parts) % 8
        if n:
            self.parts.append("0" * (8 - n))

    def bytes(self) -> bytes:
        s = "".join(self.parts)
        assert len(s) % 8 == 0
        return int(s, 2).to_bytes(len(s) // 8, "big") if s else b""


def utf8_number(v: int) -> bytes:
    """The frame / sample number of a frame header: UTF-8's scheme extended to 36 bits (7 bytes)."""
    if v < 0x80:
        return bytes([v])
    for extra, lead, bits in ((1, 0xc0, 11), (2, 0xe0, 16), (3, 0xf0, 21), (4, 0xf8, 26), (5, 0xfc, 31), (6, 0xfe, 36)):
        if v < (1 << bits):
            out = [lead | (v >> (6 * extra))]
            for k in range(extra - 1, -1, -1):
                out.append(0x80 | ((v >> (6 * k)) & 0x3f))
            return bytes(out)
    raise ValueError(v)


def block_size_code(n: int, force_trailer: bool = False):
    """-> (4-bit code, trailer bits, trailer value)."""
    if not force_trailer:
        if n == 192:
            return 1, 0, 0
        for c in range(2, 6):
            if n == 576 << (c - 2):
                return c, 0, 0
        for c in range(8, 16):
            if n == 256 << (c - 8):
                return c, 0, 0
    return (6, 8, n - 1) if n <= 256 else (7, 16, n - 1)


def rate_code(sr: int, from_streaminfo: bool = False):
    if from_streaminfo:
        return 0, 0, 0
    if sr in RATE_CODES:
        return RATE_CODES[sr], 0, 0
    if sr % 1000 == 0 and sr < 256000:
        return 12, 8, sr // 1000
    if sr < 65536:
        return 13, 16, sr
    assert sr % 10 == 0 and sr < 655360
    return 14, 16, sr // 10


def predict_residual(s, coefs, shift):
    order = len(coefs)
    return [s[i] - (sum(c * s[i - 1 - j] for j, c in enumerate(coefs)) >> shift) for i in range(order, len(s))]


def rice_param(vals, cap):
    if not vals:
        return 0
    mean = sum(abs(v) for v in vals) / len(vals)
    k = 0
    while (1 << k) < mean and k < cap:
        k += 1
    return k


def write_residual(w: BitWriter, res, block, order, partition_order=0, method=0, rice=None, escape=(), escape_bits=None):
    """rice: None (a parameter per partition from the data), an int, or a list per partition.  escape: partition indices written
    raw ("all" for every one); escape_bits: their width (default: the narrowest that holds them; 0 is used for all-zero ones)."""
    pbits, esc = (5, 31) if method else (4, 15)
    w.put(method, 2)
    w.put(partition_order, 4)
    psize = block >> partition_order
    assert psize << partition_order == block and psize >= order
    at = 0
    for part in range(1 << partition_order):
        cnt = psize - (order if part == 0 else 0)
        vals = res[at:at + cnt]
        at += cnt
        if escape == "all" or part in escape:
            nb = escape_bits
            if nb is None:
                nb = 1 if any(vals) else 0
                while nb and any(not -(1 << (nb - 1)) <= v < (1 << (nb - 1)) for v in vals):
                    nb += 1
            w.put(esc, pbits)
            w.put(nb, 5)
            for v in vals:
                w.sput(v, nb)
            continue
        k = rice if isinstance(rice, int) else (rice[part] if rice is not None else rice_param(vals, esc - 1))
        assert 0 <= k < esc
        w.put(k, pbits)
        for v in vals:
            u = (v << 1) if v >= 0 else ((-v) << 1) - 1
            assert u < (1 << 32)
            w.unary(u >> k)
            w.put(u & ((1 << k) - 1), k)
    assert at == len(res)


def write_subframe(w: BitWriter, s, bps, kind="verbatim", order=0, coefs=None, precision=None, shift=0, wasted=0, **res_opts):
    """s: the subframe's samples (a side channel already formed), bps: its width (+1 for a side channel)."""
    n = len(s)
    if wasted:
        assert all(v % (1 << wasted) == 0 for v in s), "wasted bits need samples that are multiples of 2^wasted"
        s = [v >> wasted for v in s]
    sb = bps - wasted
    w.put(0, 1)
    if kind == "constant":
        assert all(v == s[0] for v in s)
        w.put(0, 6)
    elif kind == "verbatim":
        w.put(1, 6)
    elif kind == "fixed":
        w.put(8 | order, 6)
    elif kind == "lpc":
        w.put(32 | (order - 1), 6)
    else:
        raise ValueError(kind)
    if wasted:
        w.put(1, 1)
        w.unary(wasted - 1)
    else:
        w.put(0, 1)
    if kind == "constant":
        w.sput(s[0], sb)
    elif kind == "verbatim":
        for v in s:
            w.sput(v, sb)
    else:
        taps = FIXED_TAPS[order] if kind == "fixed" else list(coefs)
        assert len(taps) == order <= n
        for v in s[:order]:
            w.sput(v, sb)
        if kind == "lpc":
            w.put(precision - 1, 4)
            w.sput(shift, 5)
            for c in taps:
                w.sput(c, precision)
        res = predict_residual(s, taps, shift if kind == "lpc" else 0)
        assert all(-(1 << 31) <= v < (1 << 31) for v in res)
        write_residual(w, res, n, order, **res_opts)


def decorrelate(chans, assignment):
    if assignment == INDEPENDENT:
        return [list(c) for c in chans]
    l, r = chans
    side = [a - b for a, b in zip(l, r)]
    if assignment == LEFT_SIDE:
        return [list(l), side]
    if assignment == RIGHT_SIDE:
        return [side, list(r)]
    return [[(a + b) >> 1 for a, b in zip(l, r)], side]


def write_frame(chans, bps, sample_rate, number, variable=False, assignment=INDEPENDENT, spec=None, force_bs_trailer=False,
                rate_from_streaminfo=False, depth_from_streaminfo=False) -> bytes:
    """One frame of chans [channels][block] (the true PCM); spec: dict of write_subframe options, or a function channel -> dict."""
    n, nch = len(chans[0]), len(chans)
    w = BitWriter()
    w.put(0x3ffe, 14)
    w.put(0, 1)
    w.put(int(variable), 1)
    bc, bt, bv = block_size_code(n, force_bs_trailer)
    rc, rt, rv = rate_code(sample_rate, rate_from_streaminfo)
    w.put(bc, 4)
    w.put(rc, 4)
    w.put(nch - 1 if assignment == INDEPENDENT else 7 + assignment, 4)
    w.put(0 if depth_from_streaminfo else DEPTH_CODES.get(bps, 0), 3)
    w.put(0, 1)
    for b in utf8_number(number):
        w.put(b, 8)
    w.put(bv, bt)
    w.put(rv, rt)
    head = w.bytes()
    w.put(crc8(head), 8)
    subs = decorrelate(chans, assignment)
    for c, s in enumerate(subs):
        side = (assignment == LEFT_SIDE and c == 1) or (assignment == RIGHT_SIDE and c == 0) or (assignment == MID_SIDE and c == 1)
        opts = dict(spec(c) if callable(spec) else (spec or {}))
        write_subframe(w, s, bps + int(side), **opts)
    w.align()
    body = w.bytes()
    return body + crc16(body).to_bytes(2, "big")


def pcm_md5(chans, bps) -> bytes:
    nb = (bps + 7) // 8
    h = hashlib.md5()
    h.update(b"".join((v & ((1 << (8 * nb)) - 1)).to_bytes(nb, "little") for frame in zip(*chans) for v in frame))
    return h.digest()


def streaminfo(min_block, max_block, sample_rate, channels, bps, total, md5: bytes) -> bytes:
    w = BitWriter()
    w.put(min_block, 16); w.put(max_block, 16); w.put(0, 24); w.put(0, 24)
    w.put(sample_rate, 20); w.put(channels - 1, 3); w.put(bps - 1, 5); w.put(total, 36)
    return w.bytes() + md5


def metadata_block(kind: int, body: bytes, last: bool) -> bytes:
    return bytes([(0x80 if last else 0) | kind]) + len(body).to_bytes(3, "big") + body


def encode(chans, bps=16, sample_rate=16000, blocks=(4096,), variable=False, assignment=INDEPENDENT, spec=None, extra_metadata=(),
           total=None, id3=b"", **frame_opts) -> bytes:
    """chans [channels][n] integers -> a whole stream.  blocks: the block sizes in turn, the last one repeated (and cut at the end of
    the samples); spec: write_subframe options, or a function (frame, channel) -> options; assignment: one value or a function of the
    frame; extra_metadata: [(type, body)] after STREAMINFO."""
    n = len(chans[0])
    frames, at, k, sizes = [], 0, 0, []
    while at < n:
        size = min(blocks[min(k, len(blocks) - 1)], n - at)
        part = [c[at:at + size] for c in chans]
        asg = assignment(k) if callable(assignment) else assignment
        sp = (lambda c, k=k: spec(k, c)) if callable(spec) else spec
        frames.append(write_frame(part, bps, sample_rate, at if variable else k, variable, asg, sp, **frame_opts))
        sizes.append(size)
        at += size
        k += 1
    body_sizes = sizes[:-1] if len(sizes) > 1 else sizes
    info = streaminfo(max(min(body_sizes), 16) if variable else blocks[0], max(sizes + [blocks[0]]), sample_rate, len(chans), bps,
                      n if total is None else total, pcm_md5(chans, bps))
    meta = [(0, info)] + list(extra_metadata)
    out = id3 + b"fLaC"
    for i, (kind, body) in enumerate(meta):
        out += metadata_block(kind, body, i == len(meta) - 1)
    return out + b"".join(frames)
