"""Test-side float64 restatement of the Layer III synthesis (ISO/IEC 11172-3 §2.4.3.4, Annex B), written from the standard's
definitions and not from csrc/mp3.hip's factorisation: requantisation by the formula, the standard's short-block reorder, MS
stereo, alias-reduction butterflies, the IMDCT as its defining cosine sum, overlap-add, frequency inversion, and the polyphase
synthesis with the 1024-sample V FIFO, N[i][k] = cos((16 + i)(2k + 1) pi / 64), U / W and the window D.  It consumes what
ss_mp3_unpack returns.  Also: the constant tables parsed out of csrc/mp3_tables.hpp, and a side-info reader that gives every
granule-channel's part2_3_length (for the exact bit-accounting checks)."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TABLES_HPP = os.path.join(ROOT, "streamspeech_amd", "csrc", "mp3_tables.hpp")


def table(name: str) -> np.ndarray:
    """An array of csrc/mp3_tables.hpp as it is compiled (flat, in source order)."""
    src = open(TABLES_HPP).read()
    m = re.search(r"\b%s(\[[^\]]*\])+\s*=\s*\{(.*?)\};" % re.escape(name), src, re.S)
    assert m, name
    body = re.sub(r"//[^\n]*", "", m.group(2))
    return np.array([float(v) for v in re.findall(r"-?\d+(?:\.\d+)?(?:e[-+]?\d+)?", body)])


def window_d() -> np.ndarray:
    """D[512] (Table B.3) from the compiled half-window: D[i] = base[min(i, 512 - i)] / 65536 * (-1)^floor(i / 64)."""
    base = table("kWinBase")
    i = np.arange(512)
    return base[np.minimum(i, 512 - i)] / 65536.0 * np.where((i // 64) % 2 == 1, -1.0, 1.0)


SFB_LONG = table("kSfbLong").reshape(9, 23).astype(int)
SFB_SHORT = table("kSfbShort").reshape(9, 14).astype(int)
PRETAB = table("kPretab").astype(int)
ALIAS_C = table("kAliasC")


# ---- side info -------------------------------------------------------------------------------------------------------------------
class _Bits:
    def __init__(self, b: bytes):
        self.v, self.n = int.from_bytes(b, "big"), len(b) * 8

    def get(self, k):
        self.n -= k
        return (self.v >> self.n) & ((1 << k) - 1)


def frames(data: bytes):
    """Frames of a clean stream (no garbage): [(offset, header dict)], after an ID3v2 tag; a Xing / Info first frame is dropped."""
    pos = 0
    if data[:3] == b"ID3":
        sz = (data[6] << 21) | (data[7] << 14) | (data[8] << 7) | data[9]
        pos = 10 + sz + (10 if data[5] & 0x10 else 0)
    end = len(data)
    if end >= 128 and data[end - 128:end - 125] == b"TAG":
        end -= 128
    out = []
    while pos + 4 <= end:
        h = int.from_bytes(data[pos:pos + 4], "big")
        assert h >> 21 == 0x7FF, "lost sync at %d" % pos
        ver, prot, bri, sri, pad, mode = (h >> 19) & 3, (h >> 16) & 1, (h >> 12) & 15, (h >> 10) & 3, (h >> 9) & 1, (h >> 6) & 3
        sr_index = {3: 0, 2: 3, 0: 6}[ver] + sri
        sr = [44100, 48000, 32000, 22050, 24000, 16000, 11025, 12000, 8000][sr_index]
        br = ([0, 32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320] if ver == 3 else
              [0, 8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160])[bri]
        flen = (144000 if ver == 3 else 72000) * br // sr + pad
        if pos + flen > end:
            break
        nch = 1 if mode == 3 else 2
        side = (17 if nch == 1 else 32) if ver == 3 else (9 if nch == 1 else 17)
        hd = dict(ver=ver, prot=prot, nch=nch, side=side, len=flen, sr_index=sr_index)
        x = data[pos + 4 + (0 if prot else 2) + side:][:4]
        if not (not out and x in (b"Xing", b"Info")):
            out.append((pos, hd))
        pos += flen
    return out


def part2_3_lengths(data: bytes):
    """part2_3_length of every granule-channel, in record order."""
    res = []
    for pos, h in frames(data):
        b = _Bits(data[pos + 4 + (0 if h["prot"] else 2):][:h["side"]])
        m1 = h["ver"] == 3
        b.get(9 if m1 else 8)
        b.get((5 if h["nch"] == 1 else 3) if m1 else (1 if h["nch"] == 1 else 2))
        if m1:
            b.get(4 * h["nch"])
        for _ in range(2 if m1 else 1):
            for _ in range(h["nch"]):
                res.append(b.get(12))
                b.get(9 + 8 + (4 if m1 else 9))
                ws = b.get(1)
                b.get(22 if ws else 22)
                b.get(3 if m1 else 2)
    return res


# ---- synthesis -------------------------------------------------------------------------------------------------------------------
def _requantise(q, r):
    sr = int(r["sr_index"])
    xr = np.zeros(576)
    a = np.abs(q.astype(np.float64)) ** (4.0 / 3.0) * np.sign(q)
    mult = 1.0 if r["scalefac_scale"] else 0.5
    gain = 2.0 ** (0.25 * (int(r["global_gain"]) - 210))
    bt, mixed = int(r["block_type"]), int(r["mixed"])
    long_end = 576 if bt != 2 else (36 if mixed else 0)
    for b in range(22):
        lo, hi = SFB_LONG[sr][b], min(SFB_LONG[sr][b + 1], long_end)
        if lo >= hi:
            break
        sf = int(r["sf_l"][b]) + (PRETAB[b] if r["preflag"] else 0)
        xr[lo:hi] = a[lo:hi] * gain * 2.0 ** (-mult * sf)
    if bt == 2:
        # bitstream order: band, window, line; the standard's reorder puts line f of window w at 3 f + w
        for b in range(3 if mixed else 0, 13):
            lo, hi = SFB_SHORT[sr][b], SFB_SHORT[sr][b + 1]
            width = hi - lo
            for w in range(3):
                g = gain * 2.0 ** (-2.0 * int(r["subblock_gain"][w])) * 2.0 ** (-mult * int(r["sf_s"][b][w]))
                src = 3 * lo + w * width + np.arange(width)
                xr[3 * (lo + np.arange(width)) + w] = a[src] * g
    return xr


def _windows():
    i = np.arange(36)
    w = np.zeros((4, 36))
    w[0] = np.sin(np.pi / 36 * (i + 0.5))
    w[1, :18] = w[0, :18]; w[1, 18:24] = 1.0; w[1, 24:30] = np.sin(np.pi / 12 * (i[24:30] - 18 + 0.5))
    w[3, 6:12] = np.sin(np.pi / 12 * (i[6:12] - 6 + 0.5)); w[3, 12:18] = 1.0; w[3, 18:] = w[0, 18:]
    w[2, :12] = np.sin(np.pi / 12 * (i[:12] + 0.5))
    return w


def _imdct(X, n):
    """x[i] = sum_k X[k] cos(pi / (2n) (2i + 1 + n / 2)(2k + 1)), i < n, k < n / 2."""
    i, k = np.arange(n)[:, None], np.arange(n // 2)[None, :]
    return np.cos(np.pi / (2 * n) * (2 * i + 1 + n / 2) * (2 * k + 1)) @ X


def synthesize(info: dict, q: np.ndarray, rec: np.ndarray, mono: bool = True) -> np.ndarray:
    """float64 PCM of one file: [n] (channel mean) with mono, else [channels, n]; the gapless trim of `info` applied."""
    nch, G = info["channels"], info["granules"]
    W = _windows()
    D = window_d()
    cs = 1.0 / np.sqrt(1.0 + ALIAS_C ** 2)
    ca = ALIAS_C / np.sqrt(1.0 + ALIAS_C ** 2)
    N = np.cos((16 + np.arange(64)[:, None]) * (2 * np.arange(32)[None, :] + 1) * np.pi / 64)
    pcm = np.zeros((nch, G * 576))
    prev = np.zeros((nch, 32, 18))
    V = np.zeros((nch, 1024))
    for g in range(G):
        xr = [_requantise(q[g * nch + c], rec[g * nch + c]) for c in range(nch)]
        if nch == 2 and rec[g * nch]["ms"]:
            m, s = xr[0].copy(), xr[1].copy()
            xr = [(m + s) / np.sqrt(2.0), (m - s) / np.sqrt(2.0)]
        for c in range(nch):
            r = rec[g * nch + c]
            bt, mixed = int(r["block_type"]), int(r["mixed"])
            x = xr[c]
            nb = 31 if bt != 2 else (1 if mixed else 0)
            for sb in range(1, nb + 1):
                for i in range(8):
                    bu, bd = x[18 * sb - 1 - i], x[18 * sb + i]
                    x[18 * sb - 1 - i] = bu * cs[i] - bd * ca[i]
                    x[18 * sb + i] = bd * cs[i] + bu * ca[i]
            S = np.zeros((18, 32))                   # [time slot][subband]
            for sb in range(32):
                X = x[18 * sb:18 * sb + 18]
                if bt != 2 or (mixed and sb < 2):
                    y = _imdct(X, 36) * W[0 if bt == 2 else bt]
                else:
                    y = np.zeros(36)
                    for w in range(3):
                        y[6 + 6 * w:18 + 6 * w] += _imdct(X[w::3], 12) * W[2, :12]
                o = y[:18] + prev[c, sb]
                prev[c, sb] = y[18:]
                if sb % 2 == 1:
                    o[1::2] = -o[1::2]
                S[:, sb] = o
            for t in range(18):
                V[c, 64:] = V[c, :-64].copy()
                V[c, :64] = N @ S[t]
                U = np.zeros(512)
                for i in range(8):
                    U[i * 64:i * 64 + 32] = V[c, i * 128:i * 128 + 32]
                    U[i * 64 + 32:i * 64 + 64] = V[c, i * 128 + 96:i * 128 + 128]
                pcm[c, g * 576 + t * 32:g * 576 + t * 32 + 32] = (U * D).reshape(16, 32).sum(0)
    out = pcm[:, info["skip"]:info["skip"] + info["samples"]]
    return out.mean(0) if mono else out
