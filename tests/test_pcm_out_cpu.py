"""Speech out at the caller's sample rate and PCM format, host side: the G.711 compressors and the other encodings
(ss_pcm_encode_host), the streaming output resampler's host twin (ss_pcm_emit_host, ss_pcm_emit_count) against the whole-utterance
result, and the pools' host logic with a stub engine whose pcm_emit runs the host twin.  Comparisons of bytes are exact.  No GPU."""
import argparse
import ctypes as C
import math
import os
import re

import numpy as np
import pytest
import torch

from streamspeech_amd import lib as L
from streamspeech_amd import pcm
from streamspeech_amd.frontend import design_filter
from streamspeech_amd.pcm import PcmFormat, PcmOut, PcmSegment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ss_pcm_emit", "ss_pcm_emit_host", "ss_pcm_emit_count", "ss_pcm_encode_host")
RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)
FMTS = ("s16le", "f32le", "ulaw", "alaw")


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_header_and_bindings():
    lib = L.load()
    with open(os.path.join(ROOT, "include", "streamspeech_hip.h"), encoding="utf-8") as f:
        header = f.read()
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\b(int|int64_t)\s+%s\s*\(" % name, header), f"{name} has no prototype in the header"
        assert name in L.SIGNATURES
    assert lib.ss_abi_version() == 2 and "#define SS_ABI_VERSION 2" in header
    assert C.sizeof(L.SSPcmEmitSeg) == 88 and "/* 88 bytes */" in header
    assert pcm.OUT_RATES == RATES


# ---- the encodings --------------------------------------------------------------------------------------------------------------
def _s16_values():
    """Every 16-bit value the pack can give, as the floats that pack to them: -32767 .. 32767 (the pack clips at -1.0, so -32768 is
    not an output of it and no float reaches the compressors with it)."""
    v = np.arange(-32767, 32768, dtype=np.int32)
    x = (v.astype(np.float64) / 32767.0).astype(np.float32)
    assert (pcm.pack_s16_host(x) == v).all()
    return v.astype("<i2"), x


def _codes(x, fmt):
    return np.frombuffer(pcm.encode_host(x, fmt), np.uint8)


def test_g711_compressors_equal_audioop():
    audioop = pytest.importorskip("audioop")
    v, x = _s16_values()
    for fmt, ref in (("ulaw", audioop.lin2ulaw), ("alaw", audioop.lin2alaw)):
        want = np.frombuffer(ref(v.tobytes(), 2), np.uint8)
        got = _codes(x, fmt)
        assert (got == want).all(), (fmt, int((got != want).sum()))
    # the expansion tables the decoders were pinned to are audioop's too: the round trip below speaks about the same pair
    codes = bytes(range(256))
    for fmt, ref in (("ulaw", audioop.ulaw2lin), ("alaw", audioop.alaw2lin)):
        assert (np.frombuffer(ref(codes, 2), "<i2").astype(np.float32) / 32768 == pcm.decode_host(codes, PcmFormat(fmt))).all()


def test_g711_round_trip_and_monotone():
    v, x = _s16_values()
    for fmt in ("ulaw", "alaw"):
        codes = np.arange(256, dtype=np.uint8)
        lin = np.round(pcm.decode_host(codes.tobytes(), PcmFormat(fmt)).astype(np.float64) * 32768).astype(np.int64)
        assert np.abs(lin).max() <= 32767
        back = _codes((lin / 32767.0).astype(np.float32), fmt)          # the floats that pack to exactly the decoded values
        assert (pcm.pack_s16_host((lin / 32767.0).astype(np.float32)) == lin).all()
        for c in range(256):
            if fmt == "ulaw" and c == 0x7F:                               # negative zero re-encodes as positive zero
                assert back[c] == 0xFF
            else:
                assert back[c] == c, (fmt, c)
        # monotone within a sign: the decoded level of the code never decreases with the input
        got = _codes(x, fmt)
        level = lin[got]
        assert (np.diff(level[v >= 0]) >= 0).all() and (np.diff(level[v < 0]) >= 0).all(), fmt
        assert (level[v >= 0] >= 0).all() and (level[v < 0] <= 0).all()
        # the code's level is never further from the input than the segment's step (a coarse bound: truncation, not nearest)
        assert (np.abs(level - v) <= np.maximum(np.abs(v.astype(np.int64)) // 16 + 16, 16)).all(), fmt


def test_encodings_of_special_values():
    x = np.array([np.nan, np.inf, -np.inf, 7.5, -7.5, 1.0, -1.0, 0.0, -0.0], np.float32)
    zero, top, bot = np.zeros(1, np.float32), np.ones(1, np.float32), -np.ones(1, np.float32)
    for fmt in ("s16le", "ulaw", "alaw"):
        sb = 2 if fmt == "s16le" else 1
        got = pcm.encode_host(x, fmt)
        z, t, b = pcm.encode_host(zero, fmt), pcm.encode_host(top, fmt), pcm.encode_host(bot, fmt)
        assert got == z + t + b + t + b + t + b + z + z, fmt
        assert len(got) == sb * x.size
    assert pcm.encode_host(top, "s16le") == np.array([32767], "<i2").tobytes()
    assert pcm.encode_host(bot, "s16le") == np.array([-32767], "<i2").tobytes()
    assert pcm.encode_host(zero, "ulaw") == b"\xff" and pcm.encode_host(zero, "alaw") == b"\xd5"
    assert pcm.encode_host(top, "ulaw") == b"\x80" and pcm.encode_host(bot, "ulaw") == b"\x00"
    assert pcm.encode_host(top, "alaw") == b"\xaa" and pcm.encode_host(bot, "alaw") == b"\x2a"
    # f32le: the bits, unclipped, NaN payloads and -0.0 included
    y = np.array([7.5, -0.0, 1e-42], np.float32)
    y = np.concatenate([y, np.array([0x7FC12345, 0xFFA00001], np.uint32).view(np.float32)])
    assert pcm.encode_host(y, "f32le") == y.tobytes()
    rng = np.random.default_rng(5)
    r = rng.uniform(-1.2, 1.2, 10000).astype(np.float32)
    assert pcm.encode_host(r, "s16le") == pcm.pack_s16_host(r).tobytes()
    lib = L.load()
    assert lib.ss_pcm_encode_host(None, 0, 0, None) == 0
    assert lib.ss_pcm_encode_host(None, 4, 0, None) == L.SS_ERR_ARG
    assert lib.ss_pcm_encode_host(r.ctypes.data, 4, 4, r.ctypes.data) == L.SS_ERR_ARG
    assert lib.ss_pcm_encode_host(r.ctypes.data, -1, 0, r.ctypes.data) == L.SS_ERR_ARG


# ---- the streaming resampler's host twin ------------------------------------------------------------------------------------------
def _k_model(n, up, down, half, finished):
    """The issue's K(N), restated."""
    if up == down:
        return n
    if finished:
        return -(-n * up // down)
    return 0 if n * up - 1 - half < 0 else (n * up - 1 - half) // down + 1


def test_emit_count_is_the_definition():
    lib = L.load()
    for R in RATES:
        up, down, half = PcmOut("s16le", R).ratio
        assert (up, down) == (R // math.gcd(R, 16000), 16000 // math.gcd(R, 16000)) and half == (0 if R == 16000 else 10 * max(up, down))
        for n in list(range(0, 200)) + [1000, 4801, 123457]:
            for fin in (False, True):
                assert pcm.emit_count(n, up, down, half, fin) == _k_model(n, up, down, half, fin), (R, n, fin)
        assert PcmOut("s16le", R).history == (0 if R == 16000 else (2 * half) // up)
    assert [PcmOut("ulaw", r).history for r in (8000, 11025, 48000)] == [40, 29, 20]
    assert lib.ss_pcm_emit_count(-1, 1, 2, 20, 0) == -1 and lib.ss_pcm_emit_count(5, 0, 2, 20, 0) == -1
    assert lib.ss_pcm_emit_count(5, 1, 0, 20, 0) == -1 and lib.ss_pcm_emit_count(5, 1, 2, -1, 0) == -1


class _HostEngine:
    """What PcmOutState / PcmEmitter need of an engine, on the host: taps as CPU tensors, pcm_emit = ss_pcm_emit_host."""
    device = "cpu"

    def __init__(self):
        self.emits = []

    def pcm_taps(self, up, down):
        return torch.from_numpy(design_filter(up, down).astype(np.float32))

    def pcm_emit(self, segs, out):
        self.emits.append([tuple(s) for s in segs])
        pcm.emit_host(segs, out)


def _whole(y, out):
    """encode(resample(y)) by the host twin over the whole y in one finished call -> (bytes, float32 samples before encoding)."""
    st = pcm.PcmOutState(out, _HostEngine())
    got = pcm.PcmEmitter(_HostEngine()).emit([(st, torch.from_numpy(y), True)])[0]
    stf = pcm.PcmOutState(PcmOut("f32le", out.sample_rate), _HostEngine())
    z = np.frombuffer(pcm.PcmEmitter(_HostEngine()).emit([(stf, torch.from_numpy(y), True)])[0], np.float32)
    return got, z


@pytest.mark.parametrize("rate", RATES)
def test_streaming_equals_whole_utterance(rate):
    from oracle.resample import resample_poly_ref
    from streamspeech_amd import synth
    rng = np.random.default_rng(rate)
    for fi, fmt in enumerate(FMTS):
        out = PcmOut(fmt, rate)
        up, down, half = out.ratio
        n = int(rng.integers(2500, 4000))
        y = synth.synth_pcm(70 + fi, n).astype(np.float32)
        y[::97] *= 1.5                                                     # some samples clip
        whole, z = _whole(y, out)
        assert len(z) == -(-n * up // down) and whole == pcm.encode_host(z, fmt)
        # the reference: the NumPy oracle the existing ss_resample test uses, at its tolerance
        want = resample_poly_ref(y, rate, 16000) if up != down else y
        assert want.shape == z.shape and np.abs(z - want).max() < 2e-6, (rate, np.abs(z - want).max())
        # random cuts: empty chunks, 1-sample chunks, a cut at 0; the finishing call adds nothing in half of the cases
        cuts = sorted(set(rng.integers(0, n + 1, 14).tolist()) | {0, 1, 2, n})
        cuts = [0] + cuts + [cuts[3]]                                      # a cut at 0 and a repeated cut: empty chunks
        cuts = sorted(cuts)
        eng = _HostEngine()
        st, em = pcm.PcmOutState(out, eng), pcm.PcmEmitter(eng)
        got, prev, n_seen = [], 0, 0
        late_finish = bool(fi % 2)
        for i, c in enumerate(cuts):
            last = i == len(cuts) - 1
            k_before = st.k
            b = em.emit([(st, torch.from_numpy(y[prev:c]), last and not late_finish)])[0]
            n_seen, prev = c, c
            assert st.n == n_seen
            fin = last and not late_finish
            assert st.k == _k_model(n_seen, up, down, half, fin) and len(b) == (st.k - k_before) * out.sample_bytes
            got.append(b)
            if st.carry is not None:
                assert st.carry.numel() == (2 * half) // up
                keep = min(st.carry.numel(), n_seen)
                assert (st.carry[:keep].numpy() == y[n_seen - keep:n_seen]).all()   # the last samples of y, and never more than the bound
        if late_finish:
            k_before = st.k
            got.append(em.emit([(st, None, True)])[0])
            assert st.k == -(-n * up // down) and len(got[-1]) == (st.k - k_before) * out.sample_bytes
            if up != down:
                assert len(got[-1]) > 0
        assert b"".join(got) == whole, (rate, fmt)
        calls = em.calls
        assert em.emit([(st, None, True)]) == [b""] and em.calls == calls   # flushed once: nothing more until reset
        st.reset()
        assert (st.n, st.k, st.flushed) == (0, 0, False)
        assert em.emit([(st, torch.from_numpy(y), True)])[0] == whole


def test_many_segments_in_one_host_call_and_untouched_gaps():
    rng = np.random.default_rng(3)
    eng = _HostEngine()
    em = pcm.PcmEmitter(eng)
    states, ys = [], []
    for i in range(12):
        out = PcmOut(FMTS[i % 4], RATES[(i * 3) % 8])
        states.append(pcm.PcmOutState(out, eng))
        ys.append(rng.uniform(-1, 1, 900 + 37 * i).astype(np.float32))
    a = em.emit([(st, torch.from_numpy(y[:400 + i]), False) for i, (st, y) in enumerate(zip(states, ys))])
    b = em.emit([(st, torch.from_numpy(y[400 + i:]), i % 2 == 0) for i, (st, y) in enumerate(zip(states, ys))])
    c = em.emit([(st, None, True) for st in states])
    assert em.calls == 3 and len(eng.emits) == 3 and all(len(e) == 12 for e in eng.emits)
    for i, (st, y) in enumerate(zip(states, ys)):
        assert a[i] + b[i] + c[i] == _whole(y, st.out)[0], i
        assert (c[i] == b"") == (i % 2 == 0 or st.up == st.down)
    for e in eng.emits:                                                    # every output range starts on a 16-byte boundary
        assert all(s[6] % 16 == 0 for s in e)


def _seg(**kw):
    d = dict(carry=0, tail=0, taps=0, n_before=0, k0=0, k1=0, out_offset=0, carry_len=0, n_new=0, up=1, down=2, half=20, fmt=1,
             finished=0)
    d.update(kw)
    return tuple(d[k] for k in ("carry", "tail", "taps", "n_before", "k0", "k1", "out_offset", "carry_len", "n_new", "up", "down",
                                "half", "fmt", "finished"))


def test_emit_host_refusals_codes_and_order():
    lib = L.load()
    taps = design_filter(1, 2).astype(np.float32)
    carry, tail = np.full(40, 9.0, np.float32), np.ones(100, np.float32)
    out = np.full(256, 0xAB, np.uint8)
    ok = dict(carry=carry.ctypes.data, tail=tail.ctypes.data, taps=taps.ctypes.data, n_new=100, k1=40)

    def call(segs, out_bytes=256, n=None, o=out):
        tab = pcm._emit_table(segs)
        return lib.ss_pcm_emit_host(tab, len(segs) if n is None else n, o.ctypes.data if o is not None else None, out_bytes)

    assert pcm.emit_count(100, 1, 2, 20, False) == 40 and pcm.emit_count(100, 1, 2, 20, True) == 50
    assert call([], n=0) == 0 and call([], n=-1) == L.SS_ERR_ARG
    assert lib.ss_pcm_emit_host(None, 1, out.ctypes.data, 256) == L.SS_ERR_ARG
    bad = [dict(fmt=4), dict(fmt=-1), dict(up=0), dict(down=0), dict(down=-2), dict(half=0), dict(half=8192),
           dict(n_new=-1), dict(n_before=-1), dict(n_before=2 ** 31 - 50), dict(carry_len=1), dict(n_before=10, carry_len=9),
           dict(k1=41), dict(k0=41, k1=40), dict(k0=-1), dict(finished=1, k1=51), dict(out_offset=8), dict(out_offset=-16),
           dict(tail=0), dict(taps=0), dict(carry=0), dict(n_before=50, carry_len=40, k0=14, k1=20)]
    for b in bad:
        d = dict(ok)
        d.update(b)
        assert call([_seg(**d)]) == L.SS_ERR_ARG, b
    assert call([_seg(**ok)], o=None) == L.SS_ERR_ARG                     # NULL output with samples to write
    # capacity: only after every argument check of every segment
    assert call([_seg(**ok)], out_bytes=79) == L.SS_ERR_CAPACITY
    assert call([_seg(**ok), _seg(**dict(ok, out_offset=256 - 64))], out_bytes=256) == L.SS_ERR_CAPACITY
    assert call([_seg(**ok), _seg(**dict(ok, fmt=9))], out_bytes=79) == L.SS_ERR_ARG
    assert (out == 0xAB).all() and (carry == 9.0).all()                   # no refusal wrote a byte
    assert call([_seg(**ok)], out_bytes=80) == 0
    assert (out[80:] == 0xAB).all() and (carry == 1.0).all()
    # up == down: no taps, no carry, the samples as they are
    assert call([_seg(tail=tail.ctypes.data, n_new=100, k1=100, up=3, down=3, half=0, fmt=2)], out_bytes=100) == 0
    assert bytes(out[:100]) == pcm.encode_host(tail, "ulaw")
    assert call([_seg(tail=tail.ctypes.data, n_new=100, k1=100, up=1, down=1, half=0, carry_len=1)]) == L.SS_ERR_ARG


# ---- PcmOut and the pools' host logic -----------------------------------------------------------------------------------------------
def test_pcm_out_is_frozen_hashable_and_validates():
    a = PcmOut("ulaw", sample_rate=8000)
    assert a == PcmOut("ulaw", 8000) and hash(a) == hash(PcmOut("ulaw", 8000)) and a != PcmOut("alaw", 8000)
    assert PcmOut("s16le").sample_rate == 16000 and PcmOut("s16le").ratio == (1, 1, 0)
    with pytest.raises(Exception):
        a.fmt = "alaw"
    for r in RATES + (12000, 96000, 4000, 100):
        PcmOut("f32le", r)
    for bad in (("s24le", 16000), ("ulaw", 0), ("ulaw", -8000), ("ulaw", 8000.5), ("ulaw", 7), ("ulaw", 16001), ("ulaw", "8000")):
        with pytest.raises(ValueError):
            PcmOut(*bad)
    with pytest.raises(ValueError):
        PcmFormat("s24le")


class _Cfg:
    max_target_positions, eos, pad, dec_dim, ctc_upsample = 1024, 2, 1, 8, 25


class _StubPool:
    def reset(self, slot):
        pass

    def set_tail(self, slot, n):
        pass


class _StubEngine(_HostEngine):
    """Enough of HipModel for the pools' host side: the PCM calls run the library's HOST entry points and count themselves; any other
    device entry point fails the test."""
    cfg = _Cfg()

    def __init__(self):
        super().__init__()
        self.packs = []

    def stream_pool(self, max_sessions, max_rows):
        return _StubPool()

    def pcm_pack_s16(self, src, out):
        self.packs.append(int(src.numel()))
        out[:src.numel()] = torch.from_numpy(pcm.pack_s16_host(src.numpy()))

    def __getattr__(self, k):
        raise AttributeError(f"device work in a host-only test: {k}")


def _args(segment_ms=320, sr=16000):
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    p = argparse.ArgumentParser()
    StreamSpeechS2STAgent.add_args(p)
    a = p.parse_args(["--model-path", "synthetic:0", "--data-bin", "/nonexistent", "--vocoder", "synthetic:0", "--dur-prediction",
                      "--sample-rate", str(sr)])
    a.source_segment_size, a.device = segment_ms, "cpu"
    return a


class _Voc:
    class cfg:
        @staticmethod
        def receptive_field_frames():
            return 20


def _dicts():
    from streamspeech_amd.modules import Dictionary
    syms = [("" if i % 3 == 0 else "▁") + f"t{i}" for i in range(40)]
    return {"tgt": Dictionary.units(1000), "target_unigram": Dictionary(syms), "source_unigram": Dictionary(syms),
            "ctc_target_unigram": Dictionary(syms)}


def _pool(n=6):
    from streamspeech_amd.speech_pool import SpeechSessionPool
    eng = _StubEngine()
    return eng, SpeechSessionPool(eng, n, 64, vocoder=_Voc())


def test_open_accepts_and_refuses():
    eng, pool = _pool()
    for kind in ("asr", "s2tt"):
        with pytest.raises(ValueError):
            pool.open(kind, _args(), dicts=_dicts(), pcm_out=PcmOut("ulaw", 8000))
    for bad in ("ulaw", "f32le", "alaw", "s16le@8000", ("ulaw", 8000), 8000, PcmFormat("ulaw")):
        with pytest.raises(ValueError):
            pool.open("s2st", _args(), dicts=_dicts(), pcm_out=bad)
    with pytest.raises(ValueError):
        pool.open("s2st", _args(), dicts=_dicts(), pcm_out=PcmOut("ulaw", 16001))       # refused where it is made
    assert pool.sessions == {} and pool._next == 0
    sid = pool.open("s2st", _args(), dicts=_dicts(), pcm_in=PcmFormat("ulaw"), pcm_out=PcmOut("ulaw", sample_rate=8000))
    s = pool.sessions[sid]
    assert s.pcm_out == PcmOut("ulaw", 8000) and s.pcm_state is not None and s.pcm_state.carry.numel() == 40
    assert s.pcm_state.taps.numel() == 41 and (s.pcm_state.n, s.pcm_state.k) == (0, 0)
    s16 = pool.sessions[pool.open("s2st", _args(), dicts=_dicts(), pcm_out="s16le")]
    assert s16.pcm_out == "s16le" and s16.pcm_state is None
    same = pool.sessions[pool.open("s2st", _args(), dicts=_dicts(), pcm_out=PcmOut("f32le"))]
    assert same.pcm_state.carry is None and same.pcm_state.taps is None     # 16 kHz out: no filter, no state
    assert pool.sessions[pool.open("s2st", _args(), dicts=_dicts())].pcm_out is None
    assert eng.emits == [] and eng.packs == []


def test_one_emit_call_beside_one_pack_call_and_the_flush_happens_once():
    eng, pool = _pool()
    outs = [PcmOut("ulaw", 8000), PcmOut("s16le", 48000), PcmOut("f32le", 44100), PcmOut("alaw", 16000)]
    own = [pool.sessions[pool.open("s2st", _args(), dicts=_dicts(), pcm_out=o)] for o in outs]
    s16 = pool.sessions[pool.open("s2st", _args(), dicts=_dicts(), pcm_out="s16le")]
    rng = np.random.default_rng(8)
    buf = torch.from_numpy(rng.uniform(-1, 1, 20000).astype(np.float32))
    ys = [buf[0:1500], buf[1500:4100], buf[4100:4101], buf[5000:7000]]
    actions = {}
    # step 1: every PcmOut session writes (tails where they lie in one buffer), the "s16le" session packs beside them
    assert pool._emit_out(list(zip(own, ys)), [], actions) == (1, sum(len(actions[s.sid][1]) for s in own))
    assert pool._pack_out([(s16, buf[8000:9000])], actions) == 1000
    assert len(eng.emits) == 1 and len(eng.emits[0]) == 4 and eng.packs == [1000]
    for s, y in zip(own, ys):
        assert eng.emits[0][own.index(s)][1] == y.data_ptr()               # no gather: the tail's own pointer
        kind, content, finished, done = actions[s.sid]
        assert kind == "speech" and isinstance(content, bytes) and not finished and not done
        st = s.pcm_state
        assert st.n == y.numel() and st.k == pcm.emit_count(st.n, st.up, st.down, st.half) and len(content) == st.k * s.pcm_out.sample_bytes
    assert actions[s16.sid][1] == pcm.pack_s16_host(buf[8000:9000].numpy()).tobytes()
    seg = pool._segment(own[0], actions[own[0].sid])
    assert isinstance(seg, PcmSegment) and (seg.fmt, seg.sample_rate, seg.finished) == ("ulaw", 8000, False)
    assert seg.content == actions[own[0].sid][1]
    first = {s.sid: actions[s.sid][1] for s in own}
    # step 2: two finish without new speech (_finish_empty), one makes its final write, one writes on; still ONE call
    for s in own[:2]:
        assert pool._finish_empty(s) == ("speech", b"", True, False)
    assert pool._flush == own[:2] and len(eng.emits) == 1
    own[2].states.source_finished = True
    more = [buf[10000:10700], buf[12000:12001]]
    assert pool._emit_out(list(zip(own[2:], more)), pool._flush, actions)[0] == 1
    assert len(eng.emits) == 2 and len(eng.emits[1]) == 4
    for s, y in zip(own[:2], ys[:2]):
        assert actions[s.sid][2:] == (True, False) and s.pcm_state.flushed
        assert first[s.sid] + actions[s.sid][1] == _whole(y.numpy(), s.pcm_out)[0] and len(actions[s.sid][1]) > 0
    assert actions[own[2].sid][2:] == (False, True)
    assert first[own[2].sid] + actions[own[2].sid][1] == _whole(torch.cat((ys[2], more[0])).numpy(), own[2].pcm_out)[0]
    assert not own[3].pcm_state.flushed and own[3].pcm_state.n == 2001
    # a later finishing call emits nothing, and makes no call, until reset
    pool._flush = []
    assert pool._finish_empty(own[0]) == ("speech", b"", True, False)
    assert pool._emit_out([], pool._flush, actions) == (0, 0) and len(eng.emits) == 2 and actions[own[0].sid][1] == b""
    # the final write's segment runs the agent's reset(): the state starts over
    seg = pool._segment(own[2], actions[own[2].sid])
    assert (seg.fmt, seg.sample_rate, seg.finished) == ("f32le", 44100, False)
    assert (own[2].pcm_state.n, own[2].pcm_state.k, own[2].pcm_state.flushed) == (0, 0, False)
    # reset(sid) and close(sid)
    pool.reset(own[0].sid)
    assert (own[0].pcm_state.n, own[0].pcm_state.k, own[0].pcm_state.flushed) == (0, 0, False)
    pool._flush = []
    again = {}
    assert pool._emit_out([(own[0], ys[0])], [], again)[0] == 1 and again[own[0].sid][1] == first[own[0].sid]
    sid = own[1].sid
    pool.close(sid)
    assert own[1].pcm_state is None and sid not in pool.sessions
    early = pool._segment(own[3], ("write", "", True))
    assert isinstance(early, PcmSegment) and early.content == b"" and early.finished and (early.fmt, early.sample_rate) == ("alaw", 16000)


def test_a_pool_without_pcm_out_sessions_calls_nothing_new():
    eng, pool = _pool()
    s16 = pool.sessions[pool.open("s2st", _args(), dicts=_dicts(), pcm_out="s16le")]
    lst = pool.sessions[pool.open("s2st", _args(), dicts=_dicts())]
    actions = {}
    assert pool._pack_out([(s16, torch.ones(10))], actions) == 10
    assert pool._finish_empty(s16) == ("speech", b"", True, False) and pool._finish_empty(lst) == ("speech", [], True, False)
    assert pool._flush == [] and pool._emitter is None and eng.emits == []
    out = pool.step()                                                       # an empty step: the counters exist and are zero
    assert out == {} and pool.last_step["pcm_emit_calls"] == 0 and pool.last_step["pcm_emit_bytes_out"] == 0
    assert pool.last_step["pcm_pack_calls"] == 0
