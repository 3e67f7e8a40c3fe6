"""The incremental batched front-end for sources at any sample rate (ss_batch_fbank_frames_sr), on the GPU: the op against
fbank_cmvn(resample(.)) for seven source rates and the 16-kHz pass-through, alone and mixed in one call; the single-session extractor
against the whole-history recompute at every call, with the rows it computes counted; text and speech pools of sessions at five rates
against their single-session agents with ONE front-end call per step; and the entry point's refusals.  Every front-end equality is
bitwise: the new path forms each 16-kHz sample with the resampler's own sum and each row with the fbank kernel's own code."""
import ctypes as C
import types

import numpy as np
import pytest
import torch

from tests import ref_fixtures as RF

pytestmark = pytest.mark.gpu

RATES = (48000, 44100, 32000, 24000, 22050, 11025, 8000, 16000)
BATCH_RMS_TOL = 1e-5        # batched against single-utterance vocoder (tests/test_speech_pool_gpu.py, tests/test_batch_gpu.py)


@pytest.fixture(scope="module")
def model(hip_model):
    return hip_model


def _want(model, x, n_in, sr):
    """The two whole-history launches the new call stands in for."""
    return model.fbank_cmvn(model.resample(x[:n_in], sr, 16000), 32768.0)


def _history(model, sr, seconds, seed):
    pcm = RF.trace_pcm(seed, sr, seconds)
    return torch.from_numpy(np.ascontiguousarray(pcm)).to(model.device)


def _nan(model, n):
    return torch.full((n, 80), float("nan"), device=model.device)


# ---- the op ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr", RATES)
def test_rows_equal_resample_then_fbank(model, sr):
    """Rows first .. first + n - 1 of the new call are fbank_cmvn(resample(x[:n_in]))[first : first + n], bit for bit: from the first
    row (the left zero padding), in the middle, and up to the last row (the right zero padding), for an n_in that is no multiple of
    anything and a history buffer longer than n_in (what lies past n_in must not be read as audio)."""
    x = _history(model, sr, 2.5, 300 + sr % 97)
    for n_in in (x.numel(), int(1.3 * sr) + 77):
        want = _want(model, x, n_in, sr)
        rows = want.shape[0]
        assert model.fbank_sr_rows(n_in, sr)[0] == rows > 100
        for first, n in ((0, rows), (rows - 3, 3), (17, 40), (rows - 1, 1)):
            out = _nan(model, n)
            model.batch_fbank_frames_sr([x], [n_in], [sr], [first], [n], [out])
            assert torch.equal(out, want[first:first + n]), (sr, n_in, first, n)


def test_mixed_rates_in_one_call(model):
    """One call with all eight rates, each session with its own first / n / n_in, and a skipped session: the per-session results."""
    hist, n_in, first, cnt, outs, want = [], [], [], [], [], []
    for i, sr in enumerate(RATES):
        x = _history(model, sr, 1.5 + 0.2 * i, 400 + i)
        n = x.numel() - 311 * i
        w = _want(model, x, n, sr)
        k = (7 * i) % w.shape[0] if i % 3 else w.shape[0] - 1 - i
        c = w.shape[0] - k if i % 2 else min(5 + i, w.shape[0] - k)
        hist.append(x); n_in.append(n); first.append(k); cnt.append(c)
        outs.append(_nan(model, c)); want.append(w[k:k + c])
    cnt[3] = 0
    outs[3] = outs[3][:0]
    model.batch_fbank_frames_sr(hist, n_in, list(RATES), first, cnt, outs)
    for i in range(len(RATES)):
        if cnt[i]:
            assert torch.equal(outs[i], want[i]), RATES[i]
    # the 16-kHz session passed through: also the bits of the 16-kHz call
    i = RATES.index(16000)
    ref = _nan(model, cnt[i])
    model.batch_fbank_frames([hist[i]], [first[i]], [cnt[i]], [ref])
    assert torch.equal(outs[i], ref)


def test_refusals_before_the_launch(model):
    """A row past what n_in resamples to, B = 0 and a null history with rows asked for: SS_ERR_ARG, no output row written, and the
    next valid call is correct."""
    from streamspeech_amd import lib as L
    from streamspeech_amd.engine import _i32, _stream, resample_ratio
    sr = 48000
    x = _history(model, sr, 1.0, 5)
    n_in = x.numel()
    up, down, half = resample_ratio(sr)
    taps = model._taps(up, down)
    rows, _ = model.fbank_sr_rows(n_in, sr)
    out = _nan(model, rows + 1)

    def call(B, pcm, first, n, n_in=n_in, up=up, half=half, tp=taps.data_ptr()):
        return model.lib.ss_batch_fbank_frames_sr(model.h, _stream(), B, (C.c_void_p * 1)(pcm), _i32([n_in]), _i32([up]), _i32([down]),
                                                  (C.c_void_p * 1)(tp), _i32([half]), _i32([first]), _i32([n]), 32768.0,
                                                  (C.c_void_p * 1)(out.data_ptr()))
    assert call(1, x.data_ptr(), 0, rows + 1) == L.SS_ERR_ARG            # one row more than the history resamples to
    assert call(1, x.data_ptr(), rows, 1) == L.SS_ERR_ARG
    assert call(1, x.data_ptr(), 0, 5, n_in=1000) == L.SS_ERR_ARG         # 1000 samples at 48 kHz make no row
    assert call(0, x.data_ptr(), 0, 1) == L.SS_ERR_ARG
    assert call(65536, x.data_ptr(), 0, 1) == L.SS_ERR_ARG
    assert call(1, 0, 0, 1) == L.SS_ERR_ARG                               # no history
    assert call(1, x.data_ptr(), 0, 1, tp=0) == L.SS_ERR_ARG              # a resampling session without taps
    assert call(1, x.data_ptr(), -1, 1) == L.SS_ERR_ARG
    assert call(1, x.data_ptr(), 0, 1, up=0) == L.SS_ERR_ARG
    assert call(1, x.data_ptr(), 0, 1, half=8000) == L.SS_ERR_ARG         # taps that do not fit the workgroup's LDS
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert call(1, x.data_ptr(), 0, rows) == 0
    assert torch.equal(out[:rows], _want(model, x, n_in, sr)) and bool(torch.isnan(out[rows:]).all())
    assert call(1, 0, 0, 0) == 0                                          # a skipped session needs no buffers


# ---- the single-session extractor --------------------------------------------------------------------------------------------------
class _Spy:
    """The engine, with the three front-end calls counted."""

    def __init__(self, m):
        self._m, self.sr_calls, self.old_calls = m, [], 0

    def __getattr__(self, name):
        return getattr(self._m, name)

    def batch_fbank_frames_sr(self, hist, n_in, rates, first, counts, outs, pcm_scale=32768.0):
        self.sr_calls.append((list(n_in), list(rates), list(first), list(counts)))
        return self._m.batch_fbank_frames_sr(hist, n_in, rates, first, counts, outs, pcm_scale)

    def resample(self, *a, **k):
        self.old_calls += 1
        return self._m.resample(*a, **k)

    def fbank_cmvn(self, *a, **k):
        self.old_calls += 1
        return self._m.fbank_cmvn(*a, **k)


class _WholeHistory:
    """An engine without the new call: the extractor resamples and transforms the whole history at every call, as it always did."""

    def __init__(self, m):
        self.device, self.resample, self.fbank_cmvn = m.device, m.resample, m.fbank_cmvn


def _fe_args(sr):
    return types.SimpleNamespace(shift_size=10, window_size=25, sample_rate=sr, feature_dim=80)


def _segments(sr, kind):
    if kind == "320ms":
        return [sr * 320 // 1000] * 11
    rng = np.random.RandomState(sr % 1000)
    return [int(v) for v in rng.randint(1, sr // 2, size=12)] + [3, 1, sr // 100 - 1, 2 * sr // 100]


@pytest.mark.parametrize("sr,kind", [(48000, "320ms"), (44100, "320ms"), (44100, "irregular"), (48000, "irregular")])
def test_extractor_against_whole_history(model, sr, kind):
    """Every call returns the rows of the whole-history recompute of that call and computes at most (rows now - rows before + 1) of
    them, the 1 being the row that was not final yet; nothing goes through resample / fbank_cmvn.  A new source list and a shrunk
    history start over."""
    from streamspeech_amd.frontend import OnlineFeatureExtractor
    spy = _Spy(model)
    fe, ref = OnlineFeatureExtractor(_fe_args(sr), spy), OnlineFeatureExtractor(_fe_args(sr), _WholeHistory(model))
    fe.clear_cache(); ref.clear_cache()
    segs = _segments(sr, kind)
    pcm = RF.trace_pcm(21, sr, sum(segs) / sr + 0.01).tolist()
    src, pos, prev_rows, computed = [], 0, 0, 0
    for n in segs:
        src.extend(pcm[pos:pos + n])
        pos += n
        before = len(spy.sr_calls)
        got, want = fe(src), ref(list(src))
        assert got.shape == want.shape and torch.equal(got, want), (sr, kind, pos)
        calls = spy.sr_calls[before:]
        assert len(calls) <= 1
        n_new = sum(c[3][0] for c in calls)
        assert n_new <= got.shape[0] - prev_rows + 1, (sr, kind, pos, n_new, got.shape[0], prev_rows)
        for c in calls:
            assert c[1] == [sr] and c[2][0] + c[3][0] == got.shape[0]
        computed += n_new
        prev_rows = got.shape[0]
    assert prev_rows > 100 and computed <= prev_rows + len(segs) and spy.old_calls == 0
    # a new source list: the cache belongs to the old one
    got, want = fe(list(src[:len(src) // 2])), ref(list(src[:len(src) // 2]))
    assert torch.equal(got, want) and spy.sr_calls[-1][2] == [0] and spy.sr_calls[-1][3] == [got.shape[0]]
    # the same list, shrunk
    src2 = list(src)
    full = fe(src2).clone()
    assert torch.equal(full, ref(list(src2)))
    del src2[len(src2) // 3:]
    got, want = fe(src2), ref(list(src2))
    assert torch.equal(got, want) and spy.sr_calls[-1][2] == [0] and spy.sr_calls[-1][3] == [got.shape[0]]
    fe.clear_cache()
    assert torch.equal(fe(src2), want) and spy.sr_calls[-1][2] == [0]


# ---- the pools ---------------------------------------------------------------------------------------------------------------------
POOL_RATES = (8000, 16000, 32000, 44100, 48000)


def _plan(cls_of, kinds, seconds=(2.2, 3.4, 1.6, 2.9, 3.1, 1.2, 2.5)):
    """Sessions at the five rates (two of them twice), 320- and 640-ms segments, joining at different steps and of different
    lengths, so that they also finish at different steps."""
    plan = {}
    for i, secs in enumerate(seconds):
        sr, kind = POOL_RATES[i % len(POOL_RATES)], kinds[i % len(kinds)]
        ms = (320, 640)[i % 2]
        args = RF.agent_args(cls_of[kind], ms, sr, {"lagging_k1": i % 3, "stride_n": 1 + i % 2})
        plan[f"{kind}{i}@{sr}"] = (kind, args, RF.trace_pcm(700 + i, sr, secs), sr, ms, (0, 2, 1, 3, 0, 4, 2)[i])
    return plan


def _drive(pool, plan, cfg, each_step):
    """As the pools' own tests drive them; each_step(pool) runs after every step()."""
    from streamspeech_amd.simuleval_shim import SpeechSegment
    d = RF.dictionaries(cfg)
    sid, pos, recs, done = {}, {}, {}, set()
    for name, (kind, args, _, _, _, _) in plan.items():
        sid[name] = pool.open(kind, args, dicts=d)
        pos[name], recs[name] = 0, []
    st = 0
    while len(done) < len(plan):
        segs = {}
        for name, (kind, args, pcm, sr, ms, start) in plan.items():
            if name in done or st < start:
                continue
            step = sr * ms // 1000
            chunk = pcm[pos[name]:pos[name] + step]
            pos[name] += step
            segs[sid[name]] = (name, SpeechSegment(content=chunk.tolist(), sample_rate=sr, finished=pos[name] >= len(pcm)))
        out = pool.step({k: v[1] for k, v in segs.items()})
        each_step(pool)
        for k, (name, seg) in segs.items():
            o = out[k]
            recs[name].append((not o.is_empty, None if o.is_empty else o.content, bool(o.finished)))
            if seg.finished:
                done.add(name)
        st += 1
    return recs


def _single(agent, pcm, sr, ms):
    from streamspeech_amd.simuleval_shim import SpeechSegment
    step, pos, want = sr * ms // 1000, 0, []
    while True:
        chunk = pcm[pos:pos + step]
        pos += step
        fin = pos >= len(pcm)
        o = agent.pushpop(SpeechSegment(content=chunk.tolist(), sample_rate=sr, finished=fin))
        want.append((not o.is_empty, None if o.is_empty else o.content, bool(o.finished)))
        if fin:
            return want


class HipVocSurface:
    """CodeHiFiGANVocoderWithDur call surface over the shared fixture handle (as tests/test_speech_pool_gpu.py)."""

    def __init__(self, hv):
        self.hip = hv

    def __call__(self, x, dur_prediction=False):
        from streamspeech_amd.modules import CodeHiFiGANVocoderWithDur
        return CodeHiFiGANVocoderWithDur.__call__(self, x, dur_prediction)


class _Counted:
    """model.resample / model.fbank_cmvn counted while a pool is driven (instance attributes over the methods, removed on exit)."""

    def __init__(self, model):
        self.model, self.n = model, 0

    def __enter__(self):
        def wrap(f):
            def g(*a, **k):
                self.n += 1
                return f(*a, **k)
            return g
        self.model.resample, self.model.fbank_cmvn = wrap(self.model.resample), wrap(self.model.fbank_cmvn)
        return self

    def __exit__(self, *exc):
        del self.model.resample, self.model.fbank_cmvn


def _one_call_per_step(steps, model):
    """After every step: one front-end call iff a session had frames, and the fbank rows every live session holds are the rows of the
    whole-history recompute of its device history, bit for bit (the class's own methods: the counted wrappers stay at zero)."""
    def check(pool):
        ls = pool.last_step
        steps.append(ls)
        assert ls["frontend_calls"] == (1 if ls["encoded"] else 0), ls
        assert (ls["fbank_rows"] > 0) == (ls["encoded"] > 0), ls
        for s in pool.sessions.values():
            fe = s.fe
            if getattr(fe, "_fb", None) is None or not fe._n_dev:
                continue
            want = type(model).fbank_cmvn(model, type(model).resample(model, fe._dev[:fe._n_dev], s.sr, 16000), 32768.0)
            assert torch.equal(fe._fb[:want.shape[0]], want), (s.sid, s.sr)
    return check


def test_text_pool_of_mixed_rates(model, synth_weights):
    """ASR and S2TT sessions at 8 / 16 / 32 / 44.1 / 48 kHz in one pool: every step() output is the matching single agent's pushpop,
    every step with frames makes ONE front-end call, and the pool never resamples or transforms a whole history."""
    from streamspeech_amd.agent_text import StreamSpeechASRAgent, StreamSpeechS2TTAgent
    from streamspeech_amd.modules import StreamSpeechModel
    from streamspeech_amd.text_pool import TextSessionPool
    cfg = synth_weights[0]
    cls_of = {"s2tt": StreamSpeechS2TTAgent, "asr": StreamSpeechASRAgent}
    plan = _plan(cls_of, ("s2tt", "asr", "s2tt"))
    steps = []
    with _Counted(model) as counted:
        got = _drive(TextSessionPool(model, 8, 256), plan, cfg, _one_call_per_step(steps, model))
        assert counted.n == 0
    assert sum(1 for ls in steps if ls["encoded"] > 1) > 5                  # steps that batched several rates
    try:
        for name, (kind, args, pcm, sr, ms, _) in plan.items():
            agent = RF.set_dicts(cls_of[kind](args, model=StreamSpeechModel.from_engine(model)), cfg)
            assert got[name] == _single(agent, pcm, sr, ms), name
    finally:
        model.encoder_stream_set_tail(0)
    assert any(c for rec in got.values() for w, c, _ in rec if w)           # text was written


def test_speech_pool_of_mixed_rates(model, hip_vocoder, synth_weights):
    """S2ST sessions at the five rates with S2TT sessions beside them: READ / WRITE sequence, finished flags and per-write sample
    counts are the single S2ST agent's, the text sessions' records are their agents', one front-end call per step, and the fbank rows
    of every session are the whole-history recompute's bits after every step.  The speech samples alone are not compared bitwise:
    the pool synthesises the writers of a step in ONE ragged vocoder call, whose sums are ordered otherwise than the single-utterance
    vocoder's (measured here: worst RMS 1.8e-7), so they keep the bar that comparison has in tests/test_speech_pool_gpu.py.  That
    is the pool's write side; nothing of it depends on the front-end once the fbank rows are equal."""
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.agent_text import StreamSpeechS2TTAgent
    from streamspeech_amd.modules import StreamSpeechModel
    from streamspeech_amd.speech_pool import SpeechSessionPool
    cfg = synth_weights[0]
    cls_of = {"s2st": StreamSpeechS2STAgent, "s2tt": StreamSpeechS2TTAgent}
    plan = _plan(cls_of, ("s2st", "s2st", "s2tt", "s2st"))
    steps = []
    with _Counted(model) as counted:
        got = _drive(SpeechSessionPool(model, 8, 256, vocoder=hip_vocoder), plan, cfg, _one_call_per_step(steps, model))
        assert counted.n == 0
    n_writes, worst = 0, 0.0
    try:
        for name, (kind, args, pcm, sr, ms, _) in plan.items():
            if kind == "s2tt":
                agent = RF.set_dicts(cls_of[kind](args, model=StreamSpeechModel.from_engine(model)), cfg)
                assert got[name] == _single(agent, pcm, sr, ms), name
                continue
            agent = RF.set_dicts(StreamSpeechS2STAgent(args, model=StreamSpeechModel.from_engine(model),
                                                       vocoder=HipVocSurface(hip_vocoder)), cfg)
            want, g = _single(agent, pcm, sr, ms), got[name]
            assert [(w, f) for w, _, f in g] == [(w, f) for w, _, f in want], name
            assert [len(c or []) for _, c, _ in g] == [len(c or []) for _, c, _ in want], name
            for (_, a, _), (_, b, _) in zip(g, want):
                if a:
                    n_writes += 1
                    rms = float(np.sqrt(np.mean((np.asarray(a, np.float32) - np.asarray(b, np.float32)) ** 2)))
                    worst = max(worst, rms)
                    assert rms < BATCH_RMS_TOL, (name, rms)
    finally:
        model.encoder_stream_set_tail(0)
    print(f"speech writes {n_writes}, worst RMS against the single agents {worst:.3g}")
    assert n_writes >= 3


def test_pool_of_16k_sessions_calls_the_16k_entry_point(model, synth_weights):
    """A pool whose sessions are all at 16 kHz makes the batch_fbank_frames call it always made: the sessions' device histories, the
    first row that is not cached, the count up to the session's frames, and the views of the row buffers those rows go to."""
    from streamspeech_amd.agent_text import StreamSpeechASRAgent, StreamSpeechS2TTAgent
    from streamspeech_amd.text_pool import TextSessionPool, fbank_frames_after
    cfg = synth_weights[0]
    cls_of = {"s2tt": StreamSpeechS2TTAgent, "asr": StreamSpeechASRAgent}
    plan = {}
    for i in range(4):
        kind = ("s2tt", "asr")[i % 2]
        plan[f"{kind}{i}"] = (kind, RF.agent_args(cls_of[kind], 320, 16000), RF.trace_pcm(40 + i, 16000, 1.5 + 0.4 * i), 16000, 320, i % 2)
    pool = TextSessionPool(model, 4, 128)
    seen = []

    def spy16(hist, first, cnt, outs, *a, **k):
        assert not a and not k and len(hist) == len(first) == len(cnt) == len(outs)
        by_dev = {s.fe._dev.data_ptr(): s for s in pool.sessions.values() if getattr(s.fe, "_dev", None) is not None}
        for h, f, c, o in zip(hist, first, cnt, outs):
            s = by_dev[h.data_ptr()]
            assert h is s.fe._dev and f + c == fbank_frames_after(16000, len(s.states.source)), (f, c)
            assert o.data_ptr() == s.fe._fb.data_ptr() + 4 * 80 * f and tuple(o.shape) == (c, 80)
        seen.append((len(hist), sum(cnt)))
        return type(model).batch_fbank_frames(model, hist, first, cnt, outs)

    def no_sr(*a, **k):
        raise AssertionError("a 16-kHz pool called batch_fbank_frames_sr")
    model.batch_fbank_frames, model.batch_fbank_frames_sr = spy16, no_sr
    try:
        def check(pool):
            ls = pool.last_step
            assert ls["frontend_calls"] == (1 if ls["encoded"] else 0)
            if ls["encoded"]:
                assert seen[-1] == (ls["encoded"], ls["fbank_rows"])
        _drive(pool, plan, cfg, check)
    finally:
        del model.batch_fbank_frames, model.batch_fbank_frames_sr
    assert len(seen) >= 5
