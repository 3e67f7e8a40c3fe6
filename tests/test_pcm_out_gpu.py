"""Speech out at the caller's sample rate and PCM format, on the GPU: the emit kernels against the library's own host twin
(ss_pcm_emit_host: the same inline functions), the streamed output against the existing resampling kernel over the whole signal, the
speech pool with PcmOut sessions against its list-fed twin, and the standalone encoder.  Every comparison of bytes is exact."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ref_fixtures as RF

pytestmark = pytest.mark.gpu

RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)
FMTS = ("s16le", "f32le", "ulaw", "alaw")
CANARY_F = np.float32(-777.25)
CANARY_B = 0xAB


@pytest.fixture(scope="module")
def model(hip_model):
    return hip_model


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _host_taps(up, down):
    from streamspeech_amd.frontend import design_filter
    return np.ascontiguousarray(design_filter(up, down).astype(np.float32))


def _mixed_segments(model, rng, n_seg=48):
    """n_seg sessions mid-stream, every rate and format, with the cases that matter: nothing received before, a history shorter than
    the carry, long tails (several tiles), empty tails, finishing with and without new samples, tail pointers off the 16-byte grid.
    -> per segment a dict with the host arrays and the device tensors."""
    from streamspeech_amd import pcm
    pad = 3                                                                 # canary floats behind every carry
    pool = torch.full((600000,), float(CANARY_F), dtype=torch.float32, device=model.device)   # the tails lie in ONE buffer
    cursor, segs = 1, []                                                    # float index 1: 4 bytes off the 16-byte grid
    for i in range(n_seg):
        out = pcm.PcmOut(FMTS[(i + i // 8) % 4], RATES[i % 8])
        up, down, half = out.ratio
        hist = out.history
        n_before = (0, 7, hist, 5000 + 13 * i, 123457)[i % 5] if hist else (0, 5, 4000)[i % 3]
        kind = i % 6
        n_new = (0 if kind in (1, 4) else (1, 2, 37, 900, 6000, 23000)[(i // 2) % 6])
        if i in (5, 9, 14, 23):
            n_new = 30000 + i                                               # several tiles also where a tile is 10240 or 14336 outputs
        finished = kind in (3, 4)
        y = rng.uniform(-1.15, 1.15, min(n_before, hist) + n_new).astype(np.float32)
        carry_len = min(n_before, hist)
        carry_h = np.full(hist + pad, CANARY_F, np.float32)
        carry_h[:carry_len] = y[:carry_len]
        tail_h = np.ascontiguousarray(y[carry_len:])
        cursor += int(rng.integers(0, 4))                                   # 0 .. 3 floats: every misalignment occurs
        tail_d = pool[cursor:cursor + n_new]
        tail_d.copy_(torch.from_numpy(tail_h))
        cursor += n_new
        k0 = pcm.emit_count(n_before, up, down, half, False)
        k1 = pcm.emit_count(n_before + n_new, up, down, half, finished)
        segs.append(dict(out=out, up=up, down=down, half=half, hist=hist, n_before=n_before, n_new=n_new, finished=finished,
                         carry_len=carry_len, carry_h=carry_h, carry_d=torch.from_numpy(carry_h.copy()).to(model.device),
                         tail_h=tail_h, tail_d=tail_d, k0=k0, k1=k1,
                         taps_h=_host_taps(up, down) if up != down else None,
                         taps_d=model.pcm_taps(up, down) if up != down else None))
    return segs


def _tuples(segs, side):
    """The segment tuples of pcm.emit / pcm.emit_host with the pointers of one side ("h" or "d"), 16..48 canary bytes between the
    output ranges.  -> (tuples, total bytes)."""
    out, cursor = [], 16
    for j, s in enumerate(segs):
        off = (cursor + 15) & ~15
        cursor = off + (s["k1"] - s["k0"]) * s["out"].sample_bytes + 16 * (j % 3)
        ptr = (lambda a: a.ctypes.data if a is not None and a.size else 0) if side == "h" else \
              (lambda t: t.data_ptr() if t is not None and t.numel() else 0)
        out.append((ptr(s["carry_" + side]), ptr(s["tail_" + side]), ptr(s["taps_" + side]), s["n_before"], s["k0"], s["k1"], off,
                    s["carry_len"], s["n_new"], s["up"], s["down"], s["half"], s["out"].code, int(s["finished"])))
    return out, cursor + 16


def test_emit_kernel_equals_host_twin(model):
    """One ss_pcm_emit call over 48 segments against ss_pcm_emit_host on copies: the whole output buffer (the canary bytes between
    the segments' ranges included) and every carry buffer (the canary floats behind it included) are equal byte for byte."""
    from streamspeech_amd import pcm
    rng = np.random.default_rng(77)
    segs = _mixed_segments(model, rng)
    assert len(segs) >= 40 and {s["out"].sample_rate for s in segs} == set(RATES) and {s["out"].fmt for s in segs} == set(FMTS)
    assert any(s["n_new"] == 0 and s["finished"] and s["k1"] > s["k0"] for s in segs)      # a flush with nothing new
    assert any(s["n_new"] == 0 and not s["finished"] for s in segs) and any(s["k1"] == s["k0"] for s in segs)
    assert any(s["tail_d"].data_ptr() % 16 for s in segs if s["n_new"])
    assert any((s["k1"] - s["k0"]) > 3 * 14336 for s in segs)
    th, total = _tuples(segs, "h")
    td, total_d = _tuples(segs, "d")
    assert total == total_d
    want = torch.full((total,), CANARY_B, dtype=torch.uint8)
    pcm.emit_host(th, want)
    got = torch.full((total,), CANARY_B, dtype=torch.uint8, device=model.device)
    model.pcm_emit(td, got)
    torch.cuda.synchronize()
    got = got.cpu().numpy()
    want = want.numpy()
    for j, (s, t) in enumerate(zip(segs, th)):
        a, b = t[6], t[6] + (s["k1"] - s["k0"]) * s["out"].sample_bytes
        assert (got[a:b] == want[a:b]).all(), (j, s["out"], s["n_before"], s["n_new"], int((got[a:b] != want[a:b]).sum()))
    assert (got == want).all()                                             # and the gaps: nothing but the ranges was written
    covered = np.zeros(total, bool)
    for s, t in zip(segs, th):
        covered[t[6]:t[6] + (s["k1"] - s["k0"]) * s["out"].sample_bytes] = True
    assert (got[~covered] == CANARY_B).all() and covered.sum() > 100000
    for j, s in enumerate(segs):
        cd = s["carry_d"].cpu().numpy()
        assert (cd.view(np.uint32) == s["carry_h"].view(np.uint32)).all(), j
        keep = min(s["hist"], s["n_before"] + s["n_new"])
        if s["n_new"] >= keep:                                              # the last samples of y, here all of them from the tail
            assert (cd[:keep] == s["tail_h"][s["n_new"] - keep:]).all()
        assert (cd[s["hist"]:] == CANARY_F).all()


def test_emit_refusals_write_nothing(model):
    from streamspeech_amd import lib as L
    from streamspeech_amd import pcm
    lib = model.lib
    taps = model.pcm_taps(1, 2)
    carry = torch.full((40,), 9.0, dtype=torch.float32, device=model.device)
    tail = torch.ones((100,), dtype=torch.float32, device=model.device)
    out = torch.full((256,), CANARY_B, dtype=torch.uint8, device=model.device)
    keys = ("carry", "tail", "taps", "n_before", "k0", "k1", "out_offset", "carry_len", "n_new", "up", "down", "half", "fmt", "finished")
    ok = dict(carry=carry.data_ptr(), tail=tail.data_ptr(), taps=taps.data_ptr(), n_before=0, k0=0, k1=40, out_offset=0, carry_len=0,
              n_new=100, up=1, down=2, half=20, fmt=1, finished=0)

    def call(ds, out_bytes=256, n=None, o=out):
        tab = pcm._emit_table([tuple(d[k] for k in keys) for d in ds])
        return lib.ss_pcm_emit(_stream(), tab, len(ds) if n is None else n, C.c_void_p(o.data_ptr() if o is not None else 0), out_bytes)

    assert call([], n=0) == 0 and call([], n=-1) == L.SS_ERR_ARG
    for bad in (dict(fmt=4), dict(up=0), dict(down=-1), dict(half=0), dict(k0=3, k1=2), dict(k1=41), dict(finished=1, k1=51),
                dict(out_offset=4), dict(tail=0), dict(taps=0), dict(carry=0), dict(carry_len=2), dict(n_new=-1)):
        assert call([ok, dict(ok, **bad)]) == L.SS_ERR_ARG, bad
    assert call([ok], o=None) == L.SS_ERR_ARG
    assert call([ok], out_bytes=79) == L.SS_ERR_CAPACITY
    assert call([ok, dict(ok, out_offset=192)]) == L.SS_ERR_CAPACITY
    assert call([dict(ok, out_offset=192), dict(ok, fmt=7)]) == L.SS_ERR_ARG               # arguments of all segments first
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == CANARY_B).all() and (carry.cpu().numpy() == 9.0).all()
    assert call([ok], out_bytes=80) == 0
    torch.cuda.synchronize()
    o = out.cpu().numpy()
    want = torch.full((256,), CANARY_B, dtype=torch.uint8)
    hc, ht, hh = np.zeros(40, np.float32), np.ones(100, np.float32), _host_taps(1, 2)
    pcm.emit_host([tuple(dict(ok, carry=hc.ctypes.data, tail=ht.ctypes.data, taps=hh.ctypes.data)[k] for k in keys)], want)
    assert (o == want.numpy()).all() and (o[80:] == CANARY_B).all() and (carry.cpu().numpy() == 1.0).all()


@pytest.mark.parametrize("rate", RATES)
def test_chunked_stream_equals_the_resample_kernel(model, rate):
    """PcmStreamEncoder fed in chunks == encode(model.resample(y, 16000, rate)): the existing device kernel over the whole signal."""
    from streamspeech_amd import pcm, synth
    rng = np.random.default_rng(rate + 1)
    n = 40000 + int(rng.integers(0, 999))
    y = synth.synth_pcm(40 + rate % 7, n).astype(np.float32)
    y[::101] *= 1.4
    yd = torch.from_numpy(y).to(model.device)
    z = model.resample(yd, 16000, rate).cpu().numpy()
    assert z.size == -(-n * rate // 16000)
    for fmt in FMTS:
        enc = pcm.PcmStreamEncoder(model, pcm.PcmOut(fmt, rate))
        cuts = sorted(set(rng.integers(0, n + 1, 9).tolist()) | {0, 1, n})
        got, prev = [], 0
        for c in [0] + cuts:
            got.append(enc.push(yd[prev:c], finished=False))
            prev = c
        got.append(enc.push(yd[:0], finished=True))
        assert b"".join(got) == pcm.encode_host(z, fmt), (rate, fmt)


def test_standalone_encoder_chunks_equal_one_shot(model):
    from streamspeech_amd import pcm
    rng = np.random.default_rng(12)
    y = rng.uniform(-1, 1, 30011).astype(np.float32)
    for out in (pcm.PcmOut("ulaw", 8000), pcm.PcmOut("s16le", 44100), pcm.PcmOut("alaw", 16000)):
        enc = pcm.PcmStreamEncoder(model, out)
        whole = enc.push(y, finished=True)                                  # host arrays are accepted and uploaded
        assert len(whole) == -(-y.size * out.sample_rate // 16000) * out.sample_bytes
        with pytest.raises(ValueError):
            enc.push(y[:10])
        enc.reset()
        parts = [enc.push(torch.from_numpy(y[a:b]).to(model.device), finished=(b == y.size))
                 for a, b in ((0, 1), (1, 1), (1, 4000), (4000, 4001), (4001, 30011))]
        assert b"".join(parts) == whole and all(isinstance(p, bytes) for p in parts)


# ---- the speech pool ----------------------------------------------------------------------------------------------------------------
def _s16(seed, n):
    from streamspeech_amd import synth
    return np.round(synth.synth_pcm(seed, n) * 32767.0).astype("<i2")


def _sessions():
    """The eight sessions of test_pcm_gpu.test_speech_pool_pcm_in_and_out_equal_list_sessions: same seeds, sizes and overrides."""
    rng = np.random.default_rng(31)
    sess = []
    for i in range(8):
        ms, sr = (320, 640, 960)[i % 3], (48000 if i == 5 else 16000)
        over = {"lagging_k1": (0, 1)[i % 2], "stride_n": (1, 2)[(i // 2) % 2]}
        sess.append((ms, sr, over, _s16(900 + i, int(sr * (1.5 + 3.5 * rng.random())))))
    return sess


def test_speech_pool_pcm_out_sessions_equal_list_sessions(model, hip_vocoder, synth_weights):
    """8 S2ST sessions answering at four-plus rates in all four formats against the same sessions list-fed in a second pool: READ /
    WRITE sequences, flags and units are equal; the bytes of every step are the encoding of samples K_before .. K_after of
    model.resample over the list side's accumulated floats, the final step flushing to ceil(N up / down); every step with such a
    writer makes exactly one emit call."""
    from streamspeech_amd import pcm
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.speech_pool import SpeechSessionPool
    d = RF.dictionaries(synth_weights[0])
    sess = _sessions()
    outs = [pcm.PcmOut(FMTS[i % 4], r) for i, r in enumerate((8000, 48000, 44100, 11025, 16000, 24000, 22050, 32000))]
    pl, pp = SpeechSessionPool(model, 8, 512, vocoder=hip_vocoder), SpeechSessionPool(model, 8, 512, vocoder=hip_vocoder)
    sl = [pl.open("s2st", RF.agent_args(StreamSpeechS2STAgent, ms, sr, over), dicts=d) for ms, sr, over, _ in sess]
    sp = [pp.open("s2st", RF.agent_args(StreamSpeechS2STAgent, ms, sr, over), dicts=d, pcm_in=pcm.PcmFormat("s16le"), pcm_out=o)
          for (ms, sr, over, _), o in zip(sess, outs)]
    pos = [0] * len(sess)
    acc = [np.zeros(0, np.float32) for _ in sess]                          # the list side's 16-kHz output of the utterance so far
    K = [0] * len(sess)
    n_writes = emits = flushed = 0
    while any(p < len(s[3]) for p, s in zip(pos, sess)):
        segs, live, fins = {}, [], {}
        for i, (ms, sr, over, s) in enumerate(sess):
            if pos[i] >= len(s):
                continue
            n = sr * ms // 1000
            chunk = s[pos[i]:pos[i] + n]
            pos[i] += len(chunk)
            fins[i] = pos[i] >= len(s)
            segs[sl[i]] = SpeechSegment(content=(chunk.astype(np.float64) / 32768).tolist(), sample_rate=sr, finished=fins[i])
            pp.push_pcm(sp[i], chunk.tobytes(), finished=fins[i])
            live.append(i)
        want, got = pl.step(segs), pp.step()
        wrote, expect_call = 0, False
        for i in live:
            w, g = want[sl[i]], got[sp[i]]
            assert (w.is_empty, bool(w.finished)) == (g.is_empty, bool(g.finished)), i
            assert not (fins[i] and w.is_empty), i                         # a finished source is always answered: the flush below runs
            if w.is_empty:
                continue
            o = outs[i]
            up, down, half = o.ratio
            assert isinstance(g, pcm.PcmSegment) and (g.fmt, g.sample_rate) == (o.fmt, o.sample_rate) and isinstance(g.content, bytes)
            acc[i] = np.concatenate([acc[i], np.asarray(w.content, np.float32)])
            k1 = pcm.emit_count(len(acc[i]), up, down, half, fins[i])
            z = model.resample(torch.from_numpy(acc[i]).to(model.device), 16000, o.sample_rate).cpu().numpy() if len(acc[i]) else acc[i]
            assert g.content == pcm.encode_host(z[K[i]:k1], o.fmt), (i, o, K[i], k1)
            if fins[i]:
                assert k1 == -(-len(acc[i]) * up // down) == z.size
                flushed += 1
            expect_call = expect_call or bool(w.content) or k1 > K[i]
            K[i] = k1
            wrote += len(g.content)
            n_writes += bool(w.content)
            assert pl.sessions[sl[i]].unit == pp.sessions[sp[i]].unit, i
        ls = pp.last_step
        assert ls["pcm_emit_calls"] == (1 if expect_call else 0) and ls["pcm_emit_bytes_out"] == wrote
        assert ls["pcm_pack_calls"] == 0 and ls["pcm_bytes_out"] == 0
        assert pl.last_step["pcm_emit_calls"] == 0 and pl.last_step["pcm_pack_calls"] == 0
        emits += ls["pcm_emit_calls"]
    assert n_writes > len(sess) and emits > 3 and flushed == len(sess)
    assert all(k > 0 for k in K)                                            # nobody answered silence only
    for i in range(len(sess)):                                              # the utterances ended: the states started over
        st = pp.sessions[sp[i]].pcm_state
        assert (st.n, st.k) == (0, 0) or st.flushed


def test_mixing_leaves_the_other_routes_alone(model, hip_vocoder, synth_weights):
    """A pool mixing PcmOut, "s16le" and list sessions answers its non-PcmOut sessions with exactly the bytes / lists of a pool
    that has no PcmOut session (there the same sessions answer lists)."""
    from streamspeech_amd import pcm
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.speech_pool import SpeechSessionPool
    d = RF.dictionaries(synth_weights[0])
    sess = _sessions()[:6]
    routes = [pcm.PcmOut("ulaw", 8000), "s16le", None, pcm.PcmOut("f32le", 48000), "s16le", None]
    pa, pb = SpeechSessionPool(model, 6, 512, vocoder=hip_vocoder), SpeechSessionPool(model, 6, 512, vocoder=hip_vocoder)
    sa = [pa.open("s2st", RF.agent_args(StreamSpeechS2STAgent, ms, sr, over), dicts=d, pcm_out=r) for (ms, sr, over, _), r in zip(sess, routes)]
    sb = [pb.open("s2st", RF.agent_args(StreamSpeechS2STAgent, ms, sr, over), dicts=d, pcm_out=(r if isinstance(r, str) else None))
          for (ms, sr, over, _), r in zip(sess, routes)]
    pos = [0] * len(sess)
    compared = both = 0
    while any(p < len(s[3]) for p, s in zip(pos, sess)):
        ga, gb, live = {}, {}, []
        for i, (ms, sr, over, s) in enumerate(sess):
            if pos[i] >= len(s):
                continue
            chunk = s[pos[i]:pos[i] + sr * ms // 1000]
            pos[i] += len(chunk)
            for g, ids in ((ga, sa), (gb, sb)):
                g[ids[i]] = SpeechSegment(content=(chunk.astype(np.float64) / 32768).tolist(), sample_rate=sr, finished=pos[i] >= len(s))
            live.append(i)
        a, b = pa.step(ga), pb.step(gb)
        for i in live:
            x, y = a[sa[i]], b[sb[i]]
            assert (x.is_empty, bool(x.finished)) == (y.is_empty, bool(y.finished)), i
            if isinstance(routes[i], pcm.PcmOut) or x.is_empty:
                continue
            assert type(x) is type(y) and x.content == y.content, i
            compared += bool(x.content)
        la, lb = pa.last_step, pb.last_step
        assert lb["pcm_emit_calls"] == 0 and (la["pcm_pack_calls"], la["pcm_bytes_out"]) == (lb["pcm_pack_calls"], lb["pcm_bytes_out"])
        both += la["pcm_emit_calls"] and la["pcm_pack_calls"]
    assert compared > 4 and both > 0                                       # steps in which the emit call and the pack call both ran
