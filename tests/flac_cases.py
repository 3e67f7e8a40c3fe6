"""The grid of synthetic FLAC streams shared by tests/test_flac_cpu.py and tests/test_flac_gpu.py: name -> (stream bytes, the PCM it
encodes as [channels][n] Python ints, bits per sample, sample rate).  Every stream is written by tests/flac_writer.py from seeded
integers; sizes are the smallest that still reach each path (a block below, at and above the device stage's 64-sample chunk, the
32-sample ring, several chunks, a last block of one sample)."""
import random

import flac_writer as W

_CACHE = {}


def _noise(seed, n, bps, scale=0.5, step=1):
    rnd = random.Random(seed)
    top = int(((1 << (bps - 1)) - 1) * scale) // step
    return [rnd.randint(-top, top) * step for _ in range(n)]


def _smooth(seed, n, bps, step=1):
    """A random walk that stays in range: small residuals under the fixed predictors."""
    rnd, top = random.Random(seed), ((1 << (bps - 1)) - 1) // step
    v, out = 0, []
    for _ in range(n):
        v = max(-top, min(top, v + rnd.randint(-(top // 16 + 1), top // 16 + 1)))
        out.append(v * step)
    return out


def _coefs(seed, order, precision, shift):
    rnd = random.Random(seed)
    if shift == 0:
        return [rnd.choice((-1, 0, 1)) for _ in range(order - 1)] + [1]
    top = (1 << (precision - 1)) - 1
    return [rnd.randint(-top, top) for _ in range(order)]


def _sizes(n, blocks):
    out, k = [], 0
    while n > 0:
        out.append(min(blocks[min(k, len(blocks) - 1)], n))
        n -= out[-1]
        k += 1
    return out


def _fit(spec, sizes):
    """A spec function whose predictor orders never exceed the frame they land in (a last block of one sample is verbatim)."""
    def f(k, c):
        o = dict(spec(k, c))
        if o.get("order", 0) > sizes[k] or (sizes[k] >> o.get("partition_order", 0)) << o.get("partition_order", 0) != sizes[k] \
                or (sizes[k] >> o.get("partition_order", 0)) < o.get("order", 0):
            return {"kind": "verbatim"}
        return o
    return f


def _add(out, name, chans, bps, sr=16000, blocks=(4096,), spec=None, **kw):
    sizes = _sizes(len(chans[0]), blocks)
    sp = _fit(spec, sizes) if callable(spec) else spec
    out[name] = (W.encode(chans, bps, sr, blocks, spec=sp, **kw), [list(c) for c in chans], bps, sr)


def lpc(order, shift, precision=12, seed=0, **kw):
    return dict(kind="lpc", order=order, coefs=_coefs(seed + order, order, precision, shift), precision=precision, shift=shift,
                method=1, **kw)


def catalogue():
    if _CACHE:
        return _CACHE
    out = {}
    # block sizes: below / at / above a 64-sample chunk of the device stage, many chunks, and a last block of ONE sample
    for b in (16, 17, 192, 4096, 4608):
        n = 2 * b + 1 if b < 4096 else b + 1
        _add(out, f"block{b}", [_smooth(b, n, 16)], 16, blocks=(b,), spec=lambda k, c: lpc(8, 10))
    # subframe types: constant, verbatim, fixed 0-4, one per frame
    kinds = [dict(kind="constant"), dict(kind="verbatim")] + [dict(kind="fixed", order=o, partition_order=o % 3) for o in range(5)]
    x = [-1234] * 192 + _smooth(1, 192 * 6, 16)
    _add(out, "types", [x], 16, blocks=(192,), spec=lambda k, c: kinds[k])
    # lpc orders x shifts x depths; 200 samples: a 192-block and a block of 8 (orders above 8 fall back to verbatim there)
    for bps in (8, 16, 24):
        for order in (1, 8, 12, 32):
            for shift in (0, 14):
                prec = 15 if shift else 2
                _add(out, f"lpc_o{order}_s{shift}_b{bps}", [_noise(order * 100 + shift + bps, 200, bps, 0.9 if shift else 0.02)], bps,
                     blocks=(192,), spec=lambda k, c, o=order, s=shift, p=prec: lpc(o, s, p))
    # wasted bits: 3 in every subframe (mono), and in one channel only of each stereo decorrelation
    _add(out, "wasted3_mono", [_smooth(5, 300, 16, step=8)], 16, blocks=(192,), spec=lambda k, c: lpc(8, 10, wasted=3))
    for bps in (16, 24):
        l, r = _smooth(6 + bps, 300, bps, step=16), _smooth(7 + bps, 300, bps, step=16)
        for asg, tag in ((W.INDEPENDENT, "lr"), (W.LEFT_SIDE, "ls"), (W.RIGHT_SIDE, "rs"), (W.MID_SIDE, "ms")):
            _add(out, f"stereo_{tag}_b{bps}", [_noise(asg + bps, 300, bps, 1.0), _noise(asg + bps + 50, 300, bps, 1.0)], bps, blocks=(192,),
                 assignment=asg, spec=lambda k, c: [dict(kind="verbatim"), dict(kind="fixed", order=2, method=1)][(k + c) % 2])
            _add(out, f"stereo_{tag}_b{bps}_wasted", [l, r], bps, blocks=(192,), assignment=asg,
                 spec=lambda k, c: lpc(4, 9, wasted=3 if c == 0 else 0))
    # the extremes of a side channel: 25-bit values
    top = (1 << 23) - 1
    _add(out, "side_extremes", [[top, -top - 1, top, 0] * 8, [-top - 1, top, top, -1] * 8], 24, blocks=(32,),
         assignment=lambda k: (W.LEFT_SIDE, W.RIGHT_SIDE, W.MID_SIDE)[k % 3], spec=dict(kind="verbatim"))
    # a frame-by-frame change of the decorrelation, odd sums under mid/side
    _add(out, "stereo_switching", [_noise(60, 500, 16, 1.0), _noise(61, 500, 16, 1.0)], 16, blocks=(100,),
         assignment=lambda k: k % 4, spec=lambda k, c: dict(kind="fixed", order=1, method=1))
    _add(out, "three_channels", [_smooth(70 + c, 300, 16) for c in range(3)], 16, blocks=(192,),
         spec=lambda k, c: [lpc(12, 11), dict(kind="fixed", order=3), dict(kind="verbatim")][c])
    _add(out, "eight_channels", [_smooth(80 + c, 100, 12) for c in range(8)], 12, sr=8000, blocks=(64,),
         spec=lambda k, c: dict(kind="fixed", order=c % 5))
    # variable blocking: sample numbers in the headers, every frame another size
    _add(out, "variable", [_smooth(90, 16 + 17 + 192 + 1000 + 4096 + 1, 16)], 16, blocks=(16, 17, 192, 1000, 4096), variable=True,
         spec=lambda k, c: lpc(8, 10))
    # 24 bits, order 32, precision 15, near full scale, every product of a sum with the same sign: |sum| ~ 2^42
    rnd = random.Random(99)
    x = [(8388607 - rnd.randint(0, 999)) if i % 2 == 0 else -(8388608 - rnd.randint(0, 999)) for i in range(192 + 64)]
    c32 = [(16383 - rnd.randint(0, 99)) * (1 if j % 2 == 0 else -1) for j in range(32)]
    _add(out, "wide_accumulator", [x], 24, blocks=(192,),
         spec=lambda k, c: dict(kind="lpc", order=32, coefs=c32, precision=15, shift=14, method=1))
    # residual coding: both methods, every partition order a block of 256 allows, escapes (0 bits included), fixed parameters
    x = [0] * 64 + _smooth(11, 192, 16)
    for method in (0, 1):
        for po in range(9):
            _add(out, f"rice_m{method}_po{po}", [x], 16, blocks=(256,),
                 spec=lambda k, c, m=method, p=po: dict(kind="fixed", order=0 if p == 8 else 1, partition_order=p, method=m,
                                                        escape=(0, 1 << p >> 1) if p else ()))
    _add(out, "escape_all", [_noise(12, 256, 16, 1.0)], 16, blocks=(256,),
         spec=dict(kind="fixed", order=2, partition_order=3, escape="all"))
    _add(out, "escape_zero_bits", [[7] * 256], 16, blocks=(256,), spec=dict(kind="fixed", order=1, partition_order=2, escape="all"))
    _add(out, "rice_k0", [[(-1) ** i * (i % 3) for i in range(256)]], 16, blocks=(256,), spec=dict(kind="fixed", order=0, rice=0))
    # header codes: sample rates by table / kHz / Hz / tens of Hz / STREAMINFO, block-size trailers, depths, long frame numbers
    for sr in (8000, 22050, 44100, 96000, 12000, 12345, 88210, 192000):
        _add(out, f"rate{sr}", [_smooth(sr, 40, 16)], 16, sr=sr, blocks=(32,), spec=dict(kind="fixed", order=1))
    _add(out, "rate_from_streaminfo", [_smooth(13, 40, 20)], 20, sr=11025, blocks=(32,), spec=dict(kind="fixed", order=1),
         rate_from_streaminfo=True, depth_from_streaminfo=True)
    _add(out, "depth10", [_smooth(14, 40, 10)], 10, blocks=(32,), spec=dict(kind="fixed", order=1))
    _add(out, "trailer8", [_smooth(15, 300, 16)], 16, blocks=(256,), spec=dict(kind="fixed", order=2), force_bs_trailer=True)
    _add(out, "trailer16", [_smooth(16, 1100, 16)], 16, blocks=(1000,), spec=dict(kind="fixed", order=2))
    _add(out, "frame_numbers", [[3] * (16 * 2100)], 16, blocks=(16,), spec=dict(kind="constant"))
    _add(out, "sample_numbers", [[-3] * (4096 * 20)], 16, blocks=(4096,), variable=True, spec=dict(kind="constant"))
    _add(out, "metadata", [_smooth(17, 100, 16)], 16, blocks=(64,), spec=dict(kind="fixed", order=1),
         extra_metadata=[(4, b"\x00" * 40), (1, bytes(100)), (3, bytes(18))], id3=b"ID3\x04\x00\x00\x00\x00\x00\x14" + bytes(20))
    _CACHE.update(out)
    return _CACHE
