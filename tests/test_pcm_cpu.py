"""Binary PCM in and out of the session pools, host side (csrc/pcm.hip's host entry points, streamspeech_amd/pcm.py, the pools' host
logic with a stub engine, the offline flag).  Every comparison is exact: the conversions are integers times powers of two, bit copies,
or one correctly rounded operation.  No GPU."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from streamspeech_amd import lib as L
from streamspeech_amd import pcm, synth
from streamspeech_amd.pcm import PcmArena, PcmFormat, PcmSegment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("ss_pcm_scatter", "ss_pcm_pack_s16", "ss_pcm_decode_host", "ss_pcm_pack_s16_host")


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_header_and_bindings():
    lib = L.load()
    with open(os.path.join(ROOT, "include", "streamspeech_hip.h"), encoding="utf-8") as f:
        header = f.read()
    for name in NEW:
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} has no prototype in the header"
        assert name in L.SIGNATURES
    assert lib.ss_abi_version() == 2 and "#define SS_ABI_VERSION 2" in header
    assert C.sizeof(L.SSPcmSeg) == 32
    assert (pcm.SS_PCM_F32LE, pcm.SS_PCM_S16LE, pcm.SS_PCM_ULAW, pcm.SS_PCM_ALAW) == (0, 1, 2, 3)
    assert re.search(r"SS_PCM_F32LE = 0, SS_PCM_S16LE = 1, SS_PCM_ULAW = 2, SS_PCM_ALAW = 3", header)


# ---- ss_pcm_decode_host ---------------------------------------------------------------------------------------------------------
def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def test_decode_s16_all_values_and_stereo_mean():
    s = np.arange(-32768, 32768, dtype=np.int64).astype("<i2")
    got = pcm.decode_host(s, PcmFormat("s16le"))
    want = s.astype(np.float32) / 32768
    assert np.array_equal(_bits(got), _bits(want))
    # the list route: the Python float of s / 32768, rounded to float32
    assert np.array_equal(_bits(got[::97]), _bits(np.asarray([int(v) / 32768 for v in s[::97]], dtype=np.float32)))
    rng = np.random.default_rng(7)
    st = rng.integers(-32768, 32768, size=(50000, 2)).astype("<i2")
    st[:4] = [[-32768, -32768], [32767, 32767], [-32768, 32767], [1, 0]]
    got = pcm.decode_host(st.tobytes(), PcmFormat("s16le", 2))
    want = (st.reshape(-1).astype(np.float32) / 32768.0).reshape(-1, 2).mean(axis=1)        # frontend.read_wav's channel mean
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(want))


def _ulaw(c):
    u = ~c & 0xFF
    t = (((u & 15) << 3) + 0x84) << ((u & 0x70) >> 4)
    return 0x84 - t if u & 0x80 else t - 0x84


def _alaw(c):
    a = c ^ 0x55
    s = (a & 0x70) >> 4
    t = (a & 15) << 4
    t = t + 8 if s == 0 else (t + 0x108) << (s - 1)
    return t if a & 0x80 else -t


def test_decode_g711_all_codes():
    codes = np.arange(256, dtype=np.uint8)
    for name, f in (("ulaw", _ulaw), ("alaw", _alaw)):
        want = np.array([f(int(c)) for c in codes], np.int64)
        got = pcm.decode_host(codes, PcmFormat(name))
        assert np.array_equal(got * 32768, want.astype(np.float32)), name         # exact: |value| < 2^15
        assert np.array_equal(_bits(got), _bits(want.astype(np.float32) / 32768))
        # stereo: the channel mean of the two expansions, as s16le
        pairs = np.stack([codes, codes[::-1]], 1).copy()
        got2 = pcm.decode_host(pairs, PcmFormat(name, 2))
        want2 = (want + want[::-1]).astype(np.float32) / 65536
        assert np.array_equal(_bits(got2), _bits(want2)), name
    u = pcm.decode_host(np.array([0x00, 0x80, 0xFF, 0x7F], np.uint8), PcmFormat("ulaw")) * 32768
    assert u.tolist() == [-32124.0, 32124.0, 0.0, 0.0]
    a = pcm.decode_host(np.array([0x2A, 0xAA, 0xD5, 0x55], np.uint8), PcmFormat("alaw")) * 32768
    assert a.tolist() == [-32256.0, 32256.0, 8.0, -8.0]
    try:
        import audioop
    except ImportError:
        return
    raw = bytes(range(256))
    for name, fn in (("ulaw", audioop.ulaw2lin), ("alaw", audioop.alaw2lin)):
        want = np.frombuffer(fn(raw, 2), "<i2").astype(np.float32) / 32768
        assert np.array_equal(_bits(pcm.decode_host(raw, PcmFormat(name))), _bits(want)), name


def test_decode_f32_keeps_bits():
    bits = np.array([0x80000000, 0x00000001, 0x807FFFFF, 0x7FC12345, 0xFFA00001, 0x7F800000, 0x3F800000, 0x00000000], np.uint32)
    x = bits.view(np.float32)
    got = pcm.decode_host(x, PcmFormat("f32le"))
    assert np.array_equal(got.view(np.uint32), bits)
    rng = np.random.default_rng(3)
    st = rng.standard_normal((4096, 2)).astype(np.float32)
    got = pcm.decode_host(st, PcmFormat("f32le", 2))
    assert np.array_equal(_bits(got), _bits((st[:, 0] + st[:, 1]) * np.float32(0.5)))
    assert pcm.decode_host(b"", PcmFormat("f32le")).size == 0


def test_decode_host_refusals():
    lib = L.load()
    buf = (C.c_float * 4)()
    for fmt, ch, n in ((4, 1, 1), (-1, 1, 1), (1, 0, 1), (1, 3, 1), (1, 1, -1)):
        assert lib.ss_pcm_decode_host(C.addressof(buf), fmt, ch, n, C.addressof(buf)) == L.SS_ERR_ARG
    assert lib.ss_pcm_decode_host(None, 1, 1, 0, None) == 0
    assert lib.ss_pcm_pack_s16_host(None, -1, None) == L.SS_ERR_ARG and lib.ss_pcm_pack_s16_host(None, 0, None) == 0
    assert lib.ss_pcm_pack_s16(None, None, -1, None) == L.SS_ERR_ARG and lib.ss_pcm_pack_s16(None, None, 0, None) == 0


# ---- ss_pcm_pack_s16_host -------------------------------------------------------------------------------------------------------
def _write_wav_array(x):
    """frontend.write_wav's samples, as it computes them."""
    x = np.clip(np.asarray(x, np.float32), -1.0, 1.0)
    return np.round(x * 32767.0).astype("<i2")


def pack_inputs(n=1_000_000, seed=11):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 0.6).astype(np.float32)
    k = np.arange(-32767, 32767, dtype=np.float64)
    special = np.concatenate([[1.0, -1.0, 1.5, -1.5, 1.0000001, -3e38, 3e38, 0.0, -0.0, 1e-40, -1e-40, np.inf, -np.inf],
                              (k + 0.5) / 32767]).astype(np.float32)
    m = min(n, special.size)
    x[:m] = special[:m]
    return x


def test_pack_s16_host_is_write_wav():
    x = pack_inputs()
    got = pcm.pack_s16_host(x)
    assert got.dtype == np.int16 and np.array_equal(got, _write_wav_array(x))
    assert pcm.pack_s16_host(np.array([np.inf, -np.inf, np.nan, -np.nan, 1.0, -1.0], np.float32)).tolist() == [32767, -32767, 0, 0, 32767, -32767]
    assert pcm.pack_s16_host(np.array([0.5 / 32767, 1.5 / 32767, 2.5 / 32767, -0.5 / 32767], np.float32)).tolist() == \
        np.round(np.array([0.5 / 32767, 1.5 / 32767, 2.5 / 32767, -0.5 / 32767], np.float32) * 32767.0).astype(np.int16).tolist()


# ---- ss_pcm_scatter refusals ----------------------------------------------------------------------------------------------------
def _scatter(segs, stage_bytes=4096, caps=(1000, 1000), n_segs=None, n_dst=None):
    """The call with pointers that are never dereferenced: every refusal comes before any HIP call."""
    lib = L.load()
    tab = (L.SSPcmSeg * max(len(segs), 1))(*[L.SSPcmSeg(*s) for s in segs])
    dst = (C.c_void_p * len(caps))(*[0x1000 * (i + 1) for i in range(len(caps))])
    cap = (C.c_int64 * len(caps))(*caps)
    return lib.ss_pcm_scatter(None, C.c_void_p(0x10000), stage_bytes, tab, len(segs) if n_segs is None else n_segs, dst, cap,
                              len(caps) if n_dst is None else n_dst)


def test_scatter_refusals_codes_and_order():
    ok = (0, 0, 100, 1, 1, 0)                    # src_offset, dst_offset, frames, fmt, channels, dst
    ARG, CAP = L.SS_ERR_ARG, L.SS_ERR_CAPACITY
    assert _scatter([ok], n_segs=-1) == ARG
    assert _scatter([], n_segs=0) == 0 and _scatter([(0, 0, 0, 9, 9, 9)], n_segs=0) == 0      # nothing to do: SS_OK, nothing read
    for bad in ((0, 0, 100, 4, 1, 0), (0, 0, 100, -1, 1, 0),          # fmt outside the enum
                (0, 0, 100, 1, 0, 0), (0, 0, 100, 1, 3, 0),           # channels
                (0, 0, -1, 1, 1, 0),                                  # frames
                (-16, 0, 100, 1, 1, 0), (8, 0, 100, 1, 1, 0), (17, 0, 100, 1, 1, 0),   # src_offset
                (0, 0, 100, 1, 1, 2), (0, 0, 100, 1, 1, -1),          # dst
                (0, -1, 100, 1, 1, 0)):                               # dst_offset
        assert _scatter([bad]) == ARG, bad
        assert _scatter([ok, bad]) == ARG, bad
    # capacities: the source range against stage_bytes, the destination range against h_dst_cap[dst]
    assert _scatter([(0, 0, 100, 1, 1, 0)], stage_bytes=199) == CAP and _scatter([(16, 0, 100, 1, 2, 0)], stage_bytes=415) == CAP
    assert _scatter([(4096 + 16, 0, 0, 1, 1, 0)]) == CAP
    assert _scatter([(0, 901, 100, 1, 1, 0)]) == CAP and _scatter([(0, 0, 1001, 2, 1, 1)]) == CAP
    assert _scatter([(0, 2 ** 62, 2 ** 31 - 1, 2, 1, 1)], stage_bytes=2 ** 40) == CAP           # no overflow in the range arithmetic
    # the order: an argument error anywhere in the table wins over a capacity error; the source is checked before the destination
    assert _scatter([(0, 0, 5000, 1, 1, 0), (0, 0, 100, 7, 1, 0)]) == ARG
    assert _scatter([(0, 0, 5000, 1, 1, 0)], stage_bytes=10, caps=(10, 10)) == CAP
    # within one segment the first of the header's list wins: fmt, channels, frames, src_offset, dst, dst_offset -- all ARG, so the
    # pairwise order shows only against CAPACITY, above
    assert _scatter([(3, -5, -1, 9, 9, 9)]) == ARG


# ---- PcmFormat / PcmArena -------------------------------------------------------------------------------------------------------
def test_format_and_partial_frames():
    assert PcmFormat("s16le").bytes_per_frame == 2 and PcmFormat("s16le", 2).bytes_per_frame == 4
    assert PcmFormat("f32le", 2).bytes_per_frame == 8 and PcmFormat("ulaw").bytes_per_frame == 1 and PcmFormat("alaw", 2).bytes_per_frame == 2
    with pytest.raises(ValueError):
        PcmFormat("s24le")
    with pytest.raises(ValueError):
        PcmFormat("s16le", 3)
    assert PcmFormat("s16le", 2).frames(4000) == 1000
    for fmt, n in ((PcmFormat("s16le"), 3), (PcmFormat("s16le", 2), 6), (PcmFormat("f32le"), 7), (PcmFormat("ulaw", 2), 5)):
        with pytest.raises(ValueError):
            pcm.as_bytes(bytes(n), fmt)


def test_arena_alignment_growth_and_buffer_types():
    ar = PcmArena("cpu", capacity=64)
    rng = np.random.default_rng(5)
    f16, f32, u8 = PcmFormat("s16le"), PcmFormat("f32le"), PcmFormat("ulaw")
    a = rng.integers(-30000, 30000, 7).astype("<i2")
    chunks = [(a.tobytes(), f16), (bytearray(a.tobytes()), f16), (memoryview(a.tobytes()), f16), (a, f16), (torch.from_numpy(a.copy()), f16),
              (rng.standard_normal(1000).astype(np.float32), f32), (torch.randn(33), f32), (np.arange(256, dtype=np.uint8), u8),
              (memoryview(a), f16), (b"", f16)]
    offs = [ar.add(d, f) for d, f in chunks]
    assert all(o % 16 == 0 for o in offs) and offs == sorted(offs) and ar.capacity >= ar.used > 64       # it grew, more than once
    for (d, f), o in zip(chunks, offs):          # every earlier chunk survived the growth
        want = bytes(pcm.as_bytes(d, f))
        assert bytes(ar.view(o, len(want))) == want
    dev, n = ar.upload()
    assert n == ar.used and ar.uploads == 1 and bytes(dev[:n].numpy()[offs[5]:offs[5] + 4000]) == bytes(pcm.as_bytes(chunks[5][0], f32))
    ar.clear()
    assert ar.used == 0 and ar.add(b"\x01\x02", f16) == 0
    # refused buffers: a wrong dtype, a non-contiguous array, something that is no buffer
    for bad, f in ((a.astype(np.int32), f16), (np.zeros(8, np.float64), f32), (np.zeros((8, 2), "<i2")[:, 0], f16),
                   (torch.zeros(8, dtype=torch.int32), f16), ([0.0, 1.0], f32), (np.zeros(8, np.int8), u8)):
        with pytest.raises(ValueError):
            ar.add(bad, f)
    assert ar.used == 2


# ---- pool host logic with a stub engine -----------------------------------------------------------------------------------------
class _Cfg:
    max_target_positions, eos, pad, dec_dim, ctc_upsample = 1024, 2, 1, 8, 25


class _StubPool:
    def reset(self, slot):
        pass

    def set_tail(self, slot, n):
        pass


class _StubEngine:
    """Enough of HipModel for the pools' host side.  The two PCM calls run the library's HOST conversions and count themselves; any
    other device entry point fails the test."""
    cfg = _Cfg()
    device = "cpu"

    def __init__(self):
        self.scatters, self.packs = [], []

    def stream_pool(self, max_sessions, max_rows):
        return _StubPool()

    def pcm_scatter(self, stage, stage_bytes, segs, dsts):
        self.scatters.append(list(segs))
        raw = stage.numpy()
        for src, at, frames, code, ch, d in segs:
            fmt = PcmFormat({v: k for k, v in pcm.FORMATS.items()}[code], ch)
            dsts[d][at:at + frames] = torch.from_numpy(pcm.decode_host(raw[src:src + frames * fmt.bytes_per_frame].tobytes(), fmt))

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


def _s16(seed, n):
    return np.round(synth.synth_pcm(seed, n) * 32767.0).astype("<i2")


def test_open_pcm_arguments():
    from streamspeech_amd.speech_pool import SpeechSessionPool
    pool = SpeechSessionPool(_StubEngine(), 4, 64, vocoder=_Voc())
    for kind in ("asr", "s2tt"):
        with pytest.raises(ValueError):
            pool.open(kind, _args(), dicts=_dicts(), pcm_out="s16le")
    with pytest.raises(ValueError):
        pool.open("s2st", _args(), dicts=_dicts(), pcm_out="ulaw")
    with pytest.raises(ValueError):
        pool.open("asr", _args(), dicts=_dicts(), pcm_in="s16le")
    assert pool.sessions == {}
    sid = pool.open("s2st", _args(), dicts=_dicts(), pcm_in=PcmFormat("s16le"), pcm_out="s16le")
    assert pool.sessions[sid].pcm_in == PcmFormat("s16le") and pool.sessions[sid].pcm_out == "s16le"
    assert pool.sessions[pool.open("asr", _args(), dicts=_dicts())].pcm_in is None


def test_admission_equals_the_list_route():
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.text_pool import TextSessionPool
    msgs = []
    for route in ("list", "pcm"):
        pool = TextSessionPool(_StubEngine(), 1, 16)
        fmt = PcmFormat("s16le") if route == "pcm" else None
        a, b = pool.open("asr", _args(), dicts=_dicts(), pcm_in=fmt), pool.open("s2tt", _args(), dicts=_dicts(), pcm_in=fmt)

        def push(sid, n):
            x = _s16(sid, n)
            if route == "pcm":
                pool.push_pcm(sid, x.tobytes())
            else:
                pool.push(sid, SpeechSegment(content=(x.astype(np.float64) / 32768).tolist(), sample_rate=16000, finished=False))
        got = []
        with pytest.raises(ValueError) as e:     # 16000 samples: 25 encoder rows pass max_rows 16
            push(a, 16000)
        got.append(str(e.value))
        assert not pool.sessions[a].pending and pool.sessions[a].n_source() == 0
        push(a, 5120)                            # takes the pool's one slot
        assert pool.sessions[a].pending and pool.sessions[a].n_source() == 5120
        with pytest.raises(ValueError) as e:     # already pushed in this step
            push(a, 160)
        got.append(str(e.value))
        with pytest.raises(ValueError) as e:     # no free slot
            push(b, 5120)
        got.append(str(e.value))
        assert not pool.sessions[b].pending and pool.sessions[b].n_source() == 0
        push(b, 300)                             # no frame yet: needs no slot
        assert pool.sessions[b].pending and pool.sessions[b].n_source() == 300
        msgs.append(got)
    assert msgs[0] == msgs[1] and len(msgs[0]) == 3


def test_mixing_refusals_change_nothing():
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.text_pool import TextSessionPool
    pool = TextSessionPool(_StubEngine(), 4, 64)
    p, q = pool.open("asr", _args(), dicts=_dicts(), pcm_in=PcmFormat("s16le")), pool.open("asr", _args(), dicts=_dicts())
    seg = SpeechSegment(content=[0.0] * 300, sample_rate=16000, finished=True)
    with pytest.raises(ValueError):
        pool.push(p, seg)
    with pytest.raises(ValueError):
        pool.step({q: seg, p: seg})              # the whole call is refused: the list-fed session does not move either
    with pytest.raises(ValueError):
        pool.push_pcm(q, bytes(600), finished=True)
    with pytest.raises(ValueError):
        pool.push_pcm(p, bytes(601))             # a partial frame
    for s in pool.sessions.values():
        assert not s.pending and s.n_source() == 0 and len(s.states.source) == 0 and not s.states.source_finished
        assert s.pcm_chunk is None
    assert pool._arena is None or pool._arena.used == 0


def test_one_upload_and_one_scatter_per_step():
    from streamspeech_amd.simuleval_shim import EmptySegment, SpeechSegment
    from streamspeech_amd.text_pool import TextSessionPool
    eng = _StubEngine()
    pool = TextSessionPool(eng, 8, 64)
    fmts = [PcmFormat("s16le"), PcmFormat("s16le", 2), PcmFormat("ulaw"), PcmFormat("f32le"), PcmFormat("alaw", 2)]
    sids = [pool.open("asr", _args(), dicts=_dicts(), pcm_in=f) for f in fmts]
    lst = pool.open("asr", _args(), dicts=_dicts())
    want = {sid: np.zeros(0, np.float32) for sid in sids}
    rng = np.random.default_rng(2)
    for step, frames in enumerate((100, 37, 120)):                 # 257 samples in all: no fbank frame yet, so no launch is due
        for sid, f in zip(sids, fmts):
            raw = rng.integers(0, 256, frames * f.bytes_per_frame, dtype=np.uint8)
            if f.fmt == "f32le":
                raw = rng.standard_normal(frames * f.channels).astype(np.float32).view(np.uint8)
            want[sid] = np.concatenate([want[sid], pcm.decode_host(raw.tobytes(), f)])
            pool.push_pcm(sid, raw.tobytes())
        pool.push(lst, SpeechSegment(content=[0.0] * frames, sample_rate=16000, finished=False))
        out = pool.step()
        assert set(out) == set(sids) | {lst} and all(isinstance(v, EmptySegment) for v in out.values())
        assert len(eng.scatters) == step + 1 and len(eng.scatters[-1]) == len(sids) and pool._arena.uploads == step + 1
        ls = pool.last_step
        assert (ls["pcm_uploads"], ls["pcm_scatter_calls"], ls["pcm_pack_calls"], ls["pcm_bytes_out"]) == (1, 1, 0, 0)
        assert ls["pcm_bytes_in"] >= sum(frames * f.bytes_per_frame for f in fmts)
        assert all(seg[0] % 16 == 0 for seg in eng.scatters[-1])
        for sid in sids:
            s = pool.sessions[sid]
            assert s.n_source() == s.fe.n_pcm == want[sid].size and s.pcm_chunk is None
            assert np.array_equal(s.fe._dev[:s.fe.n_pcm].numpy().view(np.uint32), want[sid].view(np.uint32))
    pool.push(lst, SpeechSegment(content=[0.0] * 10, sample_rate=16000, finished=False))
    pool.step()                                                    # a step without PCM: no upload, no scatter
    assert len(eng.scatters) == 3 and pool._arena.uploads == 3
    assert (pool.last_step["pcm_uploads"], pool.last_step["pcm_scatter_calls"], pool.last_step["pcm_bytes_in"]) == (0, 0, 0)
    pool.reset(sids[0])
    assert pool.sessions[sids[0]].n_source() == 0


def test_history_grows_by_doubling_and_keeps_samples():
    from streamspeech_amd.frontend import OnlineFeatureExtractor
    eng = _StubEngine()
    fe = OnlineFeatureExtractor(_args(), eng)
    fe.clear_cache()
    x = _s16(4, 200000)
    n = 0
    for k in (1234, 60000, 5000, 100000, 33766):
        dst, at = fe.pcm_reserve(k)
        assert at == n and dst.numel() >= n + k
        dst[at:at + k] = torch.from_numpy(x[n:n + k].astype(np.float32) / 32768)
        fe.pcm_commit(k)
        n += k
    assert fe.n_pcm == 200000 and np.array_equal(fe._dev[:n].numpy(), x.astype(np.float32) / 32768)
    assert fe.stage_pcm() == fe.frames_of(200000) == (1248, 199920)
    assert fe.frames_of(399) is None and fe.frames_of(400) == (1, 400)


def test_pcm_out_writers_share_one_pack_call():
    from streamspeech_amd.speech_pool import SpeechSessionPool
    eng = _StubEngine()
    pool = SpeechSessionPool(eng, 4, 64, vocoder=_Voc())
    sess = [pool.sessions[pool.open("s2st", _args(), dicts=_dicts(), pcm_in=PcmFormat("s16le"), pcm_out="s16le")] for _ in range(3)]
    buf = torch.from_numpy(pack_inputs(5000, seed=9))
    tails = [buf[0:1603], buf[1603:1603], buf[1603:4100]]          # views that follow each other, one of them empty
    actions = {}
    assert pool._pack_out(list(zip(sess, tails)), actions) == 4100 and eng.packs == [4100]
    for s, t in zip(sess, tails):
        kind, content, finished, done = actions[s.sid]
        assert kind == "speech" and isinstance(content, bytes) and not finished
        assert content == _write_wav_array(t.numpy()).tobytes()
    tails = [buf[10:99], buf[2000:2777], buf[3000:3001]]           # scattered views: gathered, still one pack call
    assert pool._pack_out(list(zip(sess, tails)), actions) == 867 and eng.packs == [4100, 867]
    for s, t in zip(sess, tails):
        assert actions[s.sid][1] == _write_wav_array(t.numpy()).tobytes()
    seg = pool._segment(sess[0], actions[sess[0].sid])
    assert isinstance(seg, PcmSegment) and seg.fmt == "s16le" and seg.sample_rate == 16000 and seg.content == actions[sess[0].sid][1]
    assert pool._finish_empty(sess[1]) == ("speech", b"", True, False)
    early = pool._segment(sess[2], ("write", "", True))
    assert isinstance(early, PcmSegment) and early.content == b"" and early.finished


# ---- offline parser -------------------------------------------------------------------------------------------------------------
def test_offline_parser_flag():
    from streamspeech_amd.offline import build_parser
    base = ["--path", "synthetic:0", "--vocoder", "synthetic:0", "--results-path", "out"]
    assert build_parser().parse_args(base).pcm16_io is False
    assert build_parser().parse_args(base + ["--pcm16-io"]).pcm16_io is True


def test_raw_wav_reader_and_pcm16_writer(tmp_path):
    from streamspeech_amd import frontend
    x = _s16(8, 4321)
    p = tmp_path / "a.wav"
    frontend.write_wav(str(p), x.astype(np.float32) / 32767.0, 48000)
    raw, nch, sr, n = frontend.read_wav_raw16(str(p))
    assert (nch, sr, n) == (1, 48000, 4321)
    want, _ = frontend.read_wav(str(p))
    assert np.array_equal(_bits(pcm.decode_host(raw, PcmFormat("s16le"))), _bits(want))
    q = tmp_path / "b.wav"
    frontend.write_wav_pcm16(str(q), pcm.pack_s16_host(want), 48000)
    frontend.write_wav(str(p), want, 48000)
    assert p.read_bytes() == q.read_bytes()
