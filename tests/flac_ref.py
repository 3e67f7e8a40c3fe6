"""An independent FLAC decoder for tests: pure Python, exact integers, written from the format's description (RFC 9639) and sharing
no code with csrc/flac_host.hip or tests/flac_writer.py beyond the two CRC polynomials.  The stream is held as a string of '0' / '1'
characters, so a field is a slice and a unary run is a str.find.  -> (facts, [channels][n] Python ints)."""
RATES = {1: 88200, 2: 176400, 3: 192000, 4: 8000, 5: 16000, 6: 22050, 7: 24000, 8: 32000, 9: 44100, 10: 48000, 11: 96000}
DEPTHS = {1: 8, 2: 12, 4: 16, 5: 20, 6: 24}


class Reader:
    def __init__(self, data: bytes, at: int):
        self.s = bin(int.from_bytes(b"\x01" + data, "big"))[3:]
        self.p = at * 8

    def u(self, n):
        if n == 0:
            return 0
        if self.p + n > len(self.s):
            raise EOFError
        v = int(self.s[self.p:self.p + n], 2)
        self.p += n
        return v

    def i(self, n):
        v = self.u(n)
        return v - (1 << n) if n and v >> (n - 1) else v

    def unary(self):
        q = self.s.find("1", self.p)
        if q < 0:
            raise EOFError
        n = q - self.p
        self.p = q + 1
        return n


def _crc(data, width, poly):
    c, top, mask = 0, 1 << (width - 1), (1 << width) - 1
    for b in data:
        c ^= b << (width - 8)
        for _ in range(8):
            c = ((c << 1) ^ poly) & mask if c & top else (c << 1) & mask
    return c


def _residual(r, n, order):
    method, po = r.u(2), r.u(4)
    assert method < 2
    pbits = 5 if method else 4
    out = []
    for part in range(1 << po):
        cnt = (n >> po) - (order if part == 0 else 0)
        k = r.u(pbits)
        if k == (1 << pbits) - 1:
            nb = r.u(5)
            out += [r.i(nb) for _ in range(cnt)]
        else:
            for _ in range(cnt):
                q = r.unary()
                v = (q << k) | r.u(k)
                out.append(-((v + 1) >> 1) if v & 1 else v >> 1)
    assert len(out) == n - order
    return out


def _subframe(r, n, bps):
    assert r.u(1) == 0
    t = r.u(6)
    wasted = r.unary() + 1 if r.u(1) else 0
    bps -= wasted
    if t == 0:
        s = [r.i(bps)] * n
    elif t == 1:
        s = [r.i(bps) for _ in range(n)]
    elif 8 <= t <= 12:
        order = t - 8
        s = [r.i(bps) for _ in range(order)]
        taps = [[], [1], [2, -1], [3, -3, 1], [4, -6, 4, -1]][order]
        for e in _residual(r, n, order):
            s.append(e + sum(c * s[-1 - j] for j, c in enumerate(taps)))
    elif t >= 32:
        order = t - 31
        s = [r.i(bps) for _ in range(order)]
        prec = r.u(4) + 1
        shift = r.i(5)
        assert prec < 16 and shift >= 0
        taps = [r.i(prec) for _ in range(order)]
        for e in _residual(r, n, order):
            s.append(e + (sum(c * s[-1 - j] for j, c in enumerate(taps)) >> shift))
    else:
        raise ValueError("reserved subframe type %d" % t)
    return [v << wasted for v in s] if wasted else s


def decode(data: bytes, max_frames=None):
    at = 0
    if data[:3] == b"ID3":
        at = 10 + ((data[6] << 21) | (data[7] << 14) | (data[8] << 7) | data[9])
    assert data[at:at + 4] == b"fLaC"
    at += 4
    facts, first = {}, True
    while True:
        last, kind, ln = data[at] >> 7, data[at] & 127, int.from_bytes(data[at + 1:at + 4], "big")
        body = data[at + 4:at + 4 + ln]
        if first:
            assert kind == 0
            v = int.from_bytes(body[:18], "big")
            facts = {"min_block": v >> 128, "max_block": (v >> 112) & 0xffff, "sample_rate": (v >> 44) & 0xfffff,
                     "channels": ((v >> 41) & 7) + 1, "bits_per_sample": ((v >> 36) & 31) + 1, "total_samples": v & ((1 << 36) - 1),
                     "md5": body[18:34].hex()}
            first = False
        at += 4 + ln
        if last:
            break
    nch, depth = facts["channels"], facts["bits_per_sample"]
    chans = [[] for _ in range(nch)]
    r = Reader(data, at)
    frames, blocks, ends = 0, [], []
    while r.p < len(r.s) and (max_frames is None or frames < max_frames):
        start = r.p // 8
        try:
            assert r.u(15) == 0x7ffc
            r.u(1)
            bc, rc, cc, dc = r.u(4), r.u(4), r.u(4), r.u(3)
            assert r.u(1) == 0
            x = r.u(8)
            extra = 0
            while x & (0x80 >> extra):
                extra += 1
            for _ in range(max(extra - 1, 0)):
                assert r.u(8) >> 6 == 2
            if bc == 1:
                n = 192
            elif 2 <= bc <= 5:
                n = 576 << (bc - 2)
            elif bc == 6:
                n = r.u(8) + 1
            elif bc == 7:
                n = r.u(16) + 1
            else:
                n = 256 << (bc - 8)
            rate = {12: lambda: r.u(8) * 1000, 13: lambda: r.u(16), 14: lambda: r.u(16) * 10}.get(rc, lambda: RATES.get(rc, facts["sample_rate"]))()
            assert rate == facts["sample_rate"] and (dc == 0 or DEPTHS[dc] == depth)
            want = _crc(data[start:r.p // 8], 8, 0x07)
            assert r.u(8) == want, "CRC-8"
            assert (cc + 1 if cc < 8 else 2) == nch
            subs = []
            for c in range(nch):
                side = (cc == 8 and c == 1) or (cc == 9 and c == 0) or (cc == 10 and c == 1)
                subs.append(_subframe(r, n, depth + int(side)))
            r.p = (r.p + 7) & ~7
            end = r.p // 8
            assert r.u(16) == _crc(data[start:end], 16, 0x8005), "CRC-16"
        except EOFError:
            break
        if cc == 8:
            subs[1] = [a - b for a, b in zip(subs[0], subs[1])]
        elif cc == 9:
            subs[0] = [a + b for a, b in zip(subs[0], subs[1])]
        elif cc == 10:
            mid = [(m << 1) | (s & 1) for m, s in zip(subs[0], subs[1])]
            subs = [[(m + s) >> 1 for m, s in zip(mid, subs[1])], [(m - s) >> 1 for m, s in zip(mid, subs[1])]]
        for c in range(nch):
            chans[c] += subs[c]
        frames += 1
        blocks.append(n)
        ends.append(r.p // 8)
    facts.update(frames=frames, samples=len(chans[0]), blocks=blocks, frame_ends=ends)
    return facts, chans
