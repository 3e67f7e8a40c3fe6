"""Binary PCM in and out of the session pools, on the GPU: the scatter and pack kernels against the library's own host conversions
(csrc/pcm.hpp, one inline function per conversion), the PCM-fed feature extractor, text pool and speech pool against their list-fed
twins, and the offline driver with and without --pcm16-io.  Every comparison is bitwise or exact equality."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from tests import ref_fixtures as RF

pytestmark = pytest.mark.gpu

CANARY = np.float32(-777.25)


@pytest.fixture(scope="module")
def model(hip_model):
    return hip_model


def _s16(seed, n):
    """Seeded synthetic audio, quantised to int16 ONCE: the list side gets s / 32768, the PCM side the int16 bytes."""
    from streamspeech_amd import synth
    return np.round(synth.synth_pcm(seed, n) * 32767.0).astype("<i2")


def _raw(rng, fmt, frames):
    """Random frames in `fmt` as bytes (f32le: finite floats and a few special bit patterns)."""
    if fmt.fmt == "f32le":
        x = rng.standard_normal(frames * fmt.channels).astype(np.float32)
        if fmt.channels == 1 and x.size > 6:
            x.view(np.uint32)[:5] = [0x80000000, 0x00000001, 0x7FC12345, 0xFFA00001, 0x807FFFFF]
        return x.tobytes()
    return rng.integers(0, 256, frames * fmt.bytes_per_frame, dtype=np.uint8).tobytes()


# ---- the kernels against the host conversions ---------------------------------------------------------------------------------------
def test_scatter_kernel_equals_host_decode(model):
    """64 segments in one call: four formats x mono / stereo, lengths 0, 1, 7, 8, 9, 4095, 4096, 100 003, destination offsets of every
    residue modulo 4 (odd ones included), several segments per destination.  The samples equal ss_pcm_decode_host bit for bit and the
    canaries on both sides of every destination range are untouched."""
    from streamspeech_amd import pcm
    rng = np.random.default_rng(17)
    fmts = [pcm.PcmFormat(f, ch) for f in ("f32le", "s16le", "ulaw", "alaw") for ch in (1, 2)]
    lengths = [0, 1, 7, 8, 9, 4095, 4096, 100003]
    arena = pcm.PcmArena(model.device, capacity=1 << 12)             # grows many times while the chunks are added
    n_dst, pad = 8, 37
    cursor = [pad + d for d in range(n_dst)]                         # next free sample of each destination; starts of every residue
    segs, want = [], []
    for i in range(64):
        fmt, frames = fmts[i % 8], lengths[(i // 8 + i) % 8]         # every (format, length) pair once
        raw = _raw(rng, fmt, frames)
        d = (i * 5) % n_dst
        at = cursor[d]
        cursor[d] = at + frames + pad + (i % 4)                      # a gap of canaries, and the next offset's residue moves on
        segs.append((arena.add(raw, fmt), at, frames, fmt.code, fmt.channels, d))
        want.append((d, at, pcm.decode_host(raw, fmt)))
    assert {(s[3], s[4], s[2]) for s in segs} == {(f.code, f.channels, n) for f in fmts for n in lengths}
    assert {s[1] % 4 for s in segs} == {0, 1, 2, 3}
    dsts = [torch.full((cursor[d] + pad,), float(CANARY), dtype=torch.float32, device=model.device) for d in range(n_dst)]
    stage, nbytes = arena.upload()
    model.pcm_scatter(stage, nbytes, segs, dsts)
    torch.cuda.synchronize()
    host = [d.cpu().numpy() for d in dsts]
    covered = [np.zeros(h.size, bool) for h in host]
    for d, at, w in want:
        got = host[d][at:at + w.size]
        assert np.array_equal(got.view(np.uint32), w.view(np.uint32)), (d, at, w.size)
        covered[d][at:at + w.size] = True
    for h, c in zip(host, covered):
        assert np.all(h[~c] == CANARY) and (~c).sum() >= 2 * pad
    # refused for the whole call, nothing written: a destination range one sample past its buffer
    from streamspeech_amd import lib as L
    bad = list(segs) + [(0, dsts[0].numel() - 3, 4, 1, 1, 0)]
    with pytest.raises(L.StreamSpeechHipError) as e:
        model.pcm_scatter(stage, nbytes, bad, dsts)
    assert e.value.code == L.SS_ERR_CAPACITY


def test_pack_kernel_equals_host_pack(model):
    from streamspeech_amd import pcm
    from tests.test_pcm_cpu import pack_inputs
    x = pack_inputs(1_000_003)
    want = pcm.pack_s16_host(x)
    dev = torch.from_numpy(x).to(model.device)
    for lo, hi in ((0, x.size), (0, 1_000_000), (1, 999_990), (3, 10), (8, 8 + 2048), (5, 6)):      # aligned and not, with tails
        out = torch.full((hi - lo + 16,), 12345, dtype=torch.int16, device=model.device)
        model.pcm_pack_s16(dev[lo:hi], out[8:8 + hi - lo])
        got = out.cpu().numpy()
        assert np.array_equal(got[8:8 + hi - lo], want[lo:hi]), (lo, hi)
        assert np.all(got[:8] == 12345) and np.all(got[8 + hi - lo:] == 12345)
    out = torch.full((64,), 12345, dtype=torch.int16, device=model.device)
    model.pcm_pack_s16(dev[3:3 + 50], out[1:51])                     # both pointers off the 16-byte grid
    got = out.cpu().numpy()
    assert np.array_equal(got[1:51], want[3:53]) and got[0] == 12345 and np.all(got[51:] == 12345)


# ---- the extractor ------------------------------------------------------------------------------------------------------------------
def _fe_args(sr):
    from streamspeech_amd.agent_text import StreamSpeechS2TTAgent
    return RF.agent_args(StreamSpeechS2TTAgent, 320, sr)


@pytest.mark.parametrize("sr", [16000, 48000])
@pytest.mark.parametrize("chunks", ["320ms", "irregular"])
def test_extractor_pcm_route_is_bitwise_the_list_route(model, sr, chunks):
    from streamspeech_amd.frontend import OnlineFeatureExtractor
    from streamspeech_amd.pcm import PcmFormat
    s = _s16(41, 3 * sr + 777)
    sizes = [sr * 320 // 1000] * 12 if chunks == "320ms" else [1234, 1, 5000, 399, 160, 1234, 20001, 7, 1234, 48000, 3333]
    a, b = OnlineFeatureExtractor(_fe_args(sr), model), OnlineFeatureExtractor(_fe_args(sr), model)
    a.clear_cache(); b.clear_cache()
    history, pos, rows = [], 0, 0
    for n in sizes:
        chunk = s[pos:pos + n]
        pos += len(chunk)
        history += (chunk.astype(np.float64) / 32768).tolist()
        want = a(history, sr)
        got = b.call_pcm(chunk.tobytes(), PcmFormat("s16le"), sr)
        assert got.shape == want.shape and torch.equal(got.view(torch.int32), want.view(torch.int32)), (sr, chunks, pos)
        assert b.n_pcm == len(history)
        rows = got.shape[0]
    assert rows > 100


def test_extractor_f32_route(model):
    from streamspeech_amd import synth
    from streamspeech_amd.frontend import OnlineFeatureExtractor
    from streamspeech_amd.pcm import PcmFormat
    x = synth.synth_pcm(5, 40000).astype(np.float32)
    a, b = OnlineFeatureExtractor(_fe_args(16000), model), OnlineFeatureExtractor(_fe_args(16000), model)
    a.clear_cache(); b.clear_cache()
    for lo, hi in ((0, 5120), (5120, 6354), (6354, 40000)):
        want = a(x[:hi].tolist(), 16000)
        got = b.call_pcm(x[lo:hi], PcmFormat("f32le"), 16000)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---- the text pool ------------------------------------------------------------------------------------------------------------------
def _text_sessions():
    """16 sessions: ASR and S2TT at 16 / 48 / 44.1 kHz s16le and 8-kHz mu-law -> (kind, sr, format name, raw bytes per sample, int16
    or mu-law samples)."""
    rng = np.random.default_rng(23)
    out = []
    for i in range(16):
        kind = ("asr", "s2tt")[i % 2]
        sr, fmt = [(16000, "s16le"), (48000, "s16le"), (44100, "s16le"), (8000, "ulaw")][(i // 2) % 4]
        secs = 1.5 + 2.5 * rng.random()
        s = _s16(500 + i, int(sr * secs))
        if fmt == "ulaw":                                     # any byte is a valid code: take the high bytes of the synthetic audio
            s = (s.view(np.uint16) >> 8).astype(np.uint8)
        out.append((kind, sr, fmt, s))
    return out


def _text_args(kind, sr, ms):
    from streamspeech_amd.agent_text import StreamSpeechASRAgent, StreamSpeechS2TTAgent
    return RF.agent_args(StreamSpeechS2TTAgent if kind == "s2tt" else StreamSpeechASRAgent, ms, sr)


def test_text_pool_pcm_sessions_equal_list_sessions(model, synth_weights):
    """The same audio through a PCM-fed pool and a list-fed pool: every step's segments and flags are equal, the fbank rows are
    bitwise equal, and every step with a push makes exactly one upload and one scatter launch."""
    from streamspeech_amd import pcm
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.text_pool import TextSessionPool
    cfg = synth_weights[0]
    d = RF.dictionaries(cfg)
    sess = _text_sessions()
    pools = {"list": TextSessionPool(model, 16, 512), "pcm": TextSessionPool(model, 16, 512)}
    sids = {"list": [], "pcm": []}
    for kind, sr, fmt, s in sess:
        sids["list"].append(pools["list"].open(kind, _text_args(kind, sr, 320), dicts=d))
        sids["pcm"].append(pools["pcm"].open(kind, _text_args(kind, sr, 320), dicts=d, pcm_in=pcm.PcmFormat(fmt)))
    pos = [0] * len(sess)
    steps = writes = 0
    while any(p < len(s[3]) for p, s in zip(pos, sess)):
        segs, pushed, fins = {}, 0, {}
        for i, (kind, sr, fmt, s) in enumerate(sess):
            if pos[i] >= len(s):
                continue
            n = sr * 320 // 1000 if i % 3 else 1234 + 100 * i          # every third session pushes irregular chunks
            chunk = s[pos[i]:pos[i] + n]
            pos[i] += len(chunk)
            fin = pos[i] >= len(s)
            fins[i] = fin
            decoded = pcm.decode_host(chunk, pcm.PcmFormat(fmt))       # the samples the PCM side stands for
            segs[sids["list"][i]] = SpeechSegment(content=decoded.astype(np.float64).tolist(), sample_rate=sr, finished=fin)
            pools["pcm"].push_pcm(sids["pcm"][i], chunk.tobytes() if i % 2 else chunk, finished=fin)
            pushed += chunk.nbytes
        want = pools["list"].step(segs)
        got = pools["pcm"].step()
        ls = pools["pcm"].last_step
        assert ls["pcm_uploads"] == ls["pcm_scatter_calls"] == 1 and ls["pcm_bytes_in"] >= pushed and ls["pcm_pack_calls"] == 0
        assert pools["list"].last_step["pcm_uploads"] == pools["list"].last_step["pcm_scatter_calls"] == 0
        for k in ("sessions", "encoded", "writers", "frontend_calls", "fbank_rows"):
            assert ls[k] == pools["list"].last_step[k], k
        for i in fins:
            w, g = want[sids["list"][i]], got[sids["pcm"][i]]
            assert type(w) is type(g) and (w.is_empty, w.content, w.finished) == (g.is_empty, g.content, g.finished), (steps, i)
            writes += bool(w.content)
            a, b = pools["list"].sessions[sids["list"][i]], pools["pcm"].sessions[sids["pcm"][i]]
            assert a.fe._n_fb == b.fe._n_fb and (a.fe._fb is None) == (b.fe._fb is None)
            if a.fe._fb is not None and a.fe._n_fb:
                k = a.fe._n_fb
                assert torch.equal(a.fe._fb[:k].view(torch.int32), b.fe._fb[:k].view(torch.int32)), (steps, i)
        steps += 1
    assert steps > 8 and writes > 0


def test_text_pool_serves_both_kinds_in_one_step(model, synth_weights):
    """A PCM-fed and a list-fed session of the same audio in ONE pool give the same answers step by step; feeding either the wrong way
    is refused and changes nothing."""
    from streamspeech_amd import pcm
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.text_pool import TextSessionPool
    d = RF.dictionaries(synth_weights[0])
    pool = TextSessionPool(model, 4, 256)
    a = pool.open("s2tt", _text_args("s2tt", 16000, 320), dicts=d)
    b = pool.open("s2tt", _text_args("s2tt", 16000, 320), dicts=d, pcm_in=pcm.PcmFormat("s16le", 2))
    s = _s16(77, 16000 * 3)
    stereo = np.stack([s, s], 1).copy()                               # the channel mean of two equal channels is the channel
    with pytest.raises(ValueError):
        pool.push_pcm(a, s[:5120].tobytes())
    with pytest.raises(ValueError):
        pool.step({b: SpeechSegment(content=[0.0] * 5120, sample_rate=16000, finished=False)})
    assert not pool.sessions[a].pending and not pool.sessions[b].pending and pool.sessions[b].n_source() == 0
    texts = []
    for pos in range(0, len(s), 5120):
        fin = pos + 5120 >= len(s)
        pool.push_pcm(b, stereo[pos:pos + 5120], finished=fin)
        out = pool.step({a: SpeechSegment(content=(s[pos:pos + 5120].astype(np.float64) / 32768).tolist(), sample_rate=16000,
                                          finished=fin)})
        assert (out[a].is_empty, out[a].content, out[a].finished) == (out[b].is_empty, out[b].content, out[b].finished)
        texts.append(out[a].content)
        assert pool.last_step["pcm_uploads"] == 1 and pool.last_step["frontend_calls"] == 1
    assert any(texts)


# ---- the speech pool ----------------------------------------------------------------------------------------------------------------
def test_speech_pool_pcm_in_and_out_equal_list_sessions(model, hip_vocoder, synth_weights):
    """8 S2ST sessions with s16le in and out against the same sessions list-fed: READ / WRITE sequences and flags are equal, the units
    are identical, and the output bytes are exactly write_wav's rounding of the list side's samples; every writing step makes one pack
    launch (and one download of exactly the bytes it answers with)."""
    from streamspeech_amd import pcm
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.speech_pool import SpeechSessionPool
    d = RF.dictionaries(synth_weights[0])
    rng = np.random.default_rng(31)
    sess = []
    for i in range(8):
        ms, sr = (320, 640, 960)[i % 3], (48000 if i == 5 else 16000)
        over = {"lagging_k1": (0, 1)[i % 2], "stride_n": (1, 2)[(i // 2) % 2]}
        sess.append((ms, sr, over, _s16(900 + i, int(sr * (1.5 + 3.5 * rng.random())))))
    pl, pp = SpeechSessionPool(model, 8, 512, vocoder=hip_vocoder), SpeechSessionPool(model, 8, 512, vocoder=hip_vocoder)
    sl = [pl.open("s2st", RF.agent_args(StreamSpeechS2STAgent, ms, sr, over), dicts=d) for ms, sr, over, _ in sess]
    sp = [pp.open("s2st", RF.agent_args(StreamSpeechS2STAgent, ms, sr, over), dicts=d, pcm_in=pcm.PcmFormat("s16le"), pcm_out="s16le")
          for ms, sr, over, _ in sess]
    pos = [0] * len(sess)
    n_writes = packs = 0
    while any(p < len(s[3]) for p, s in zip(pos, sess)):
        segs, live = {}, []
        for i, (ms, sr, over, s) in enumerate(sess):
            if pos[i] >= len(s):
                continue
            n = sr * ms // 1000
            chunk = s[pos[i]:pos[i] + n]
            pos[i] += len(chunk)
            fin = pos[i] >= len(s)
            segs[sl[i]] = SpeechSegment(content=(chunk.astype(np.float64) / 32768).tolist(), sample_rate=sr, finished=fin)
            pp.push_pcm(sp[i], chunk.tobytes(), finished=fin)
            live.append(i)
        want, got = pl.step(segs), pp.step()
        wrote = 0
        for i in live:
            w, g = want[sl[i]], got[sp[i]]
            assert (w.is_empty, bool(w.finished)) == (g.is_empty, bool(g.finished)), i
            if w.is_empty:
                continue
            assert isinstance(g, pcm.PcmSegment) and g.fmt == "s16le" and g.sample_rate == 16000 and isinstance(g.content, bytes)
            ref = np.round(np.clip(np.asarray(w.content, np.float32), -1.0, 1.0) * 32767.0).astype("<i2")      # write_wav's samples
            assert g.content == ref.tobytes(), i
            wrote += len(g.content)
            n_writes += bool(w.content)
            assert pl.sessions[sl[i]].unit == pp.sessions[sp[i]].unit, i
        ls = pp.last_step
        assert ls["pcm_uploads"] == ls["pcm_scatter_calls"] == 1
        assert ls["pcm_pack_calls"] == (1 if wrote else 0) and ls["pcm_bytes_out"] == wrote
        assert "handover_s" in ls or not ls["writers"]
        assert pl.last_step["pcm_pack_calls"] == 0 and pl.last_step["pcm_uploads"] == 0
        packs += ls["pcm_pack_calls"]
    assert n_writes > len(sess) and packs > 3


# ---- the offline driver -------------------------------------------------------------------------------------------------------------
def test_offline_pcm16_io_writes_the_same_files(tmp_path):
    """Six 16-bit WAVs (16 and 48 kHz, one of them stereo) through the driver with and without --pcm16-io: every output file is
    byte-identical."""
    import wave
    from streamspeech_amd import offline
    paths = []
    for i in range(6):
        sr = (16000, 48000)[i % 2]
        s = _s16(1200 + i, int(sr * (1.0 + 0.6 * i)))
        nch = 2 if i == 3 else 1
        if nch == 2:
            s = np.stack([s, _s16(1300, len(s))], 1).copy()
        p = tmp_path / f"u{i}.wav"
        with wave.open(str(p), "wb") as w:
            w.setnchannels(nch); w.setsampwidth(2); w.setframerate(sr)
            w.writeframes(s.tobytes())
        paths.append(str(p))
    lst = tmp_path / "wav_list.txt"
    lst.write_text("\n".join(paths) + "\n")
    base = ["--wav-list", str(lst), "--path", "synthetic:0", "--vocoder", "synthetic:0", "--device", "cuda:0", "--dur-prediction",
            "--batch-size", "4"]
    offline.main(base + ["--results-path", str(tmp_path / "plain")])
    offline.main(base + ["--results-path", str(tmp_path / "pcm"), "--pcm16-io"])
    files = []
    for root, _, names in os.walk(tmp_path / "plain"):
        files += [os.path.relpath(os.path.join(root, n), tmp_path / "plain") for n in names]
    assert len([f for f in files if f.endswith("_pred.wav")]) == 6 and len(files) >= 11
    for f in files:
        with open(tmp_path / "plain" / f, "rb") as a, open(tmp_path / "pcm" / f, "rb") as b:
            assert a.read() == b.read(), f
    assert sorted(files) == sorted(os.path.relpath(os.path.join(r, n), tmp_path / "pcm")
                                   for r, _, ns in os.walk(tmp_path / "pcm") for n in ns)
