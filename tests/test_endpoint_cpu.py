"""Endpointing of live PCM streams, host side: the ABI, the scan's host twin (ss_vad_scan_host) against the float64 restatement of
tests/vad_ref.py, its invariance under chunking, its refusals, Endpoint's validation, and the pools' host logic with a stub engine
whose vad_scan runs the host twin.  No GPU."""
import argparse
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from streamspeech_amd import endpoint as EP
from streamspeech_amd import lib as L
from streamspeech_amd import pcm
from streamspeech_amd.endpoint import Endpoint
from streamspeech_amd.pcm import PcmFormat
from streamspeech_amd.simuleval_shim import EmptySegment

from tests import vad_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = {"silence": Endpoint(max_utterance_ms=10000), "forced": Endpoint(max_utterance_ms=700)}


# ---- ABI ------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_header_and_bindings():
    lib = L.load()
    with open(os.path.join(ROOT, "include", "streamspeech_hip.h"), encoding="utf-8") as f:
        header = f.read()
    for name in ("ss_vad_scan", "ss_vad_scan_host"):
        assert hasattr(lib, name), f"{name} is not exported"
        assert re.search(r"\bint\s+%s\s*\(" % name, header), f"{name} has no prototype in the header"
        assert name in L.SIGNATURES
    assert lib.ss_abi_version() == 2 and "#define SS_ABI_VERSION 2" in header
    for struct, size, name in ((L.SSVadSeg, 96, "ss_vad_seg"), (L.SSVadState, 40, "ss_vad_state"), (L.SSVadResult, 40, "ss_vad_result")):
        assert C.sizeof(struct) == size
        assert re.search(r"}\s*%s;\s*/\* %d bytes \*/" % (name, size), header), name
    assert (EP.STATE_BYTES, EP.RESULT_BYTES) == (40, 40)


# ---- the host twin against the float64 reference ----------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(EPS))
@pytest.mark.parametrize("sr", R.RATES)
def test_host_twin_equals_the_float64_reference(sr, which):
    ep = EPS[which]
    p, thr = ep.params(sr), R.ref_thresholds(ep)
    assert (p.H, p.W) == (sr // 100, int(25 * sr / 1000)) and p.W <= 1200
    x = R.make_stream(sr, 1000 + sr)
    total = p.frames_present(x.size)
    # the reference alone first: no decision of these inputs lies within 3 dB of its threshold
    P64 = R.ref_powers(x, p.H, p.W, 0, 0, total)
    margins, st64, want, nxt = [], R.fresh_state(), [], 0
    while nxt < total:
        r = R.ref_scan(P64[nxt:], p, thr, st64, nxt, margins)
        want.append(r)
        nxt = r["consumed"]
    assert len(margins) == total - 1 and min(margins) > 3.0, min(margins)
    # the DC offset is not speech, the short burst starts nothing, the pause inside an utterance does not end it
    kinds = R.merge([(r["events"], r["start_frame"], r["cut_sample"]) for r in want])
    if which == "silence":
        assert [k for k, _ in kinds] == ["start", "end", "start", "end"]
        assert kinds[0][1] == 58 and kinds[1][1] == (219 + 1 + p.post_roll) * p.H + p.W - p.H      # frames 58 .. 219 see the bursts
    else:
        assert [k for k, _ in kinds].count("forced") >= 2 and kinds[0] == ("start", 58)
    # the host twin, call for call
    state, nxt = np.zeros(EP.STATE_BYTES, np.uint8), 0
    for w in want:
        n = total - nxt
        pw = np.full(n + 2, -1.0, np.float32)
        got = R.host_scan(x, p, state, 0, nxt, n, pw[1:n + 1])
        assert got == w, (got, w)
        k = got["consumed"] - nxt
        assert pw[0] == -1.0 and (pw[k + 1:] == -1.0).all()                  # frames behind the stop are not written
        rel = np.abs(pw[1:k + 1].astype(np.float64) - P64[nxt:nxt + k]) / P64[nxt:nxt + k]
        assert rel.max() < 2e-4, rel.max()
        nxt = got["consumed"]
    sd = R.state_dict(state)
    assert {k: sd[k] for k in sd if k != "floor"} == {k: st64[k] for k in st64 if k != "floor"}
    assert abs(sd["floor"] - st64["floor"]) <= 2e-4 * st64["floor"]


@pytest.mark.parametrize("which", sorted(EPS))
def test_host_twin_is_invariant_under_chunking(which):
    for sr in (8000, 11025):
        p = EPS[which].params(sr)
        x = R.make_stream(sr, 77 + sr)
        total = p.frames_present(x.size)
        runs = []
        for chunk in (1, 7, 64, 65, total):
            state = np.zeros(EP.STATE_BYTES, np.uint8)
            ev = R.scan_all(lambda first, n: R.host_scan(x, p, state, 0, first, n), total, chunk)
            runs.append((R.merge(ev), state.tobytes()))
        assert len(runs[0][0]) >= 4
        for r in runs[1:]:
            assert r == runs[0]
        # a history that begins later in the stream gives the same answers: only the frames' own samples are read
        state, cut = np.zeros(EP.STATE_BYTES, np.uint8), 61 * p.H
        a = R.host_scan(x, p, state, 0, 0, 61)
        b = R.host_scan(x[cut:], p, state, cut, 61, total - 61)
        state2 = np.zeros(EP.STATE_BYTES, np.uint8)
        assert R.host_scan(x, p, state2, 0, 0, total) == dict(b, start_frame=max(a["start_frame"], b["start_frame"]),
                                                                   events=a["events"] | b["events"])
        assert state.tobytes() == state2.tobytes()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def _good(x, state, p, first=0, n=10, hist_first=0):
    return L.SSVadSeg(*p.seg(x.ctypes.data, state.ctypes.data, 0, hist_first, x.size, first, n), 0)


def test_refusals_in_order_and_nothing_is_touched():
    lib = L.load()
    p = Endpoint(max_utterance_ms=10000).params(8000)
    x = R.make_stream(8000, 3)[:8000]
    state = np.zeros(EP.STATE_BYTES, np.uint8)
    R.host_scan(x, p, state, 0, 0, 70)                                       # mid-utterance: a state worth keeping
    assert R.state_dict(state)["mode"] == EP.SPEECH
    x0, s0 = x.copy(), state.copy()
    res = (L.SSVadResult * 2)()
    sentinel = bytes(res)

    def rc(segs, n=None, results=res):
        tab = (L.SSVadSeg * max(len(segs), 1))(*segs)
        return lib.ss_vad_scan_host(tab, len(segs) if n is None else n, results)

    def bad(**kw):
        g = _good(x, state, p, 70, 10)
        for k, v in kw.items():
            setattr(g, k, v)
        return g
    ok = _good(x, state, p, 70, 10)
    assert rc([ok], n=-1) == L.SS_ERR_ARG
    assert rc([bad(H=0)], n=0) == 0 and lib.ss_vad_scan_host(None, 0, None) == 0       # n_segs == 0: SS_OK before anything is read
    assert lib.ss_vad_scan_host(None, 1, res) == L.SS_ERR_ARG and rc([ok], results=None) == L.SS_ERR_ARG
    full = p.frames_present(x.size)
    cases = [dict(state=None), dict(reserved=1), dict(H=0), dict(W=0), dict(H=p.W + 1), dict(W=(1 << 20) + 1),
             dict(min_speech=0), dict(end_silence=0), dict(post_roll=-1), dict(post_roll=p.end_silence + 1), dict(max_frames=0),
             dict(p_abs=-1.0), dict(p_abs=float("nan")), dict(p_min=-1.0), dict(snr=0.0), dict(rise=float("nan")),
             dict(n_frames=-1), dict(n_hist=-1), dict(first_frame=-1), dict(hist_first=-1), dict(first_frame=1 << 40),
             dict(hist_first=70 * p.H + 1),                                  # the first frame begins before the history
             dict(n_frames=full - 70 + 1),                                   # the last frame ends behind it
             dict(n_hist=79 * p.H + p.W - 1), dict(hist=None)]
    for kw in cases:
        assert rc([bad(**kw)]) == L.SS_ERR_ARG, kw
        assert rc([ok, bad(**kw)]) == L.SS_ERR_ARG, kw                        # for the whole call: the good segment is not run
    # order: the first bad field of the first bad segment decides, and every refusal is SS_ERR_ARG, so the order shows in what
    # is NOT evaluated: a NULL history is only looked at behind the range check, which needs frames to scan
    assert rc([bad(hist=None, n_frames=0)]) == 0
    assert bytes(res)[40:] == sentinel[40:]
    assert (x == x0).all() and (state == s0).all()
    assert rc([bad(n_frames=full - 70)]) == 0 and not (state == s0).all()     # the exact fit is accepted


# ---- Endpoint ---------------------------------------------------------------------------------------------------------------------
def test_endpoint_validation_and_conversion():
    for kw in (dict(threshold_db=1.0), dict(threshold_db=-120.0), dict(threshold_db=float("nan")), dict(threshold_db="-50"),
               dict(snr_db=-1.0), dict(floor_rise_db_per_s=-0.1), dict(min_speech_ms=0), dict(end_silence_ms=0), dict(pre_roll_ms=-1),
               dict(post_roll_ms=-1), dict(post_roll_ms=700), dict(max_utterance_ms=0), dict(max_utterance_ms=float("inf")),
               dict(min_speech_ms=True)):
        with pytest.raises(ValueError):
            Endpoint(**kw)
    ep = Endpoint()
    assert (ep.threshold_db, ep.snr_db, ep.floor_rise_db_per_s, ep.min_speech_ms, ep.end_silence_ms, ep.pre_roll_ms, ep.post_roll_ms,
            ep.max_utterance_ms) == (-50.0, 9.0, 2.0, 100, 600, 200, 200, None)
    with pytest.raises(Exception):
        ep.snr_db = 3.0                                                        # frozen
    with pytest.raises(ValueError):
        ep.params(16000)                                                       # no limit given and no pool to take it from
    p = ep.params(11025, fit_samples=110250)
    assert (p.H, p.W, p.min_speech, p.end_silence, p.post_roll, p.pre_roll_samples) == (110, 275, 10, 60, 20, 2205)
    assert p.max_utterance_samples == 110250 and p.max_frames == (110250 - 165 - 2205) // 110
    assert p.p_abs == float(np.float32(1e-5)) and p.p_min == float(np.float32(1e-10))
    assert p.snr == float(np.float32(10 ** 0.9)) and p.rise == float(np.float32(10 ** 0.002))
    with pytest.raises(ValueError):
        Endpoint(max_utterance_ms=20000).params(16000, fit_samples=160000)     # more than the pool holds
    with pytest.raises(ValueError):
        Endpoint(max_utterance_ms=250).params(16000)                           # no room behind the pre-roll


# ---- the pools' host logic with a stub engine -------------------------------------------------------------------------------------
class _Cfg:
    max_target_positions, eos, pad, dec_dim, ctc_upsample = 1024, 2, 1, 8, 25


def _enc_len(T):
    t1 = (T + 2 * 2 - 5) // 2 + 1
    return (t1 + 2 * 2 - 5) // 2 + 1


class _StubPool:
    """The encoder step and the CTC heads: one token per 8 encoder rows, read off the fbank rows (which the stub engine makes of the
    history's own samples), so the text depends on every sample an utterance commits and on where it lies in the history."""

    def __init__(self):
        self.held = set()

    def reset(self, slot):
        pass

    def set_tail(self, slot, n):
        pass

    def forward(self, slots, fbanks, attn, conv):
        assert len(set(slots)) == len(slots)
        self.T2 = [_enc_len(f.shape[0]) for f in fbanks]
        self.toks = [[int(abs(float(f[min(32 * k, f.shape[0] - 1), 0])) * 1e3) % 40 for k in range(t // 8)] for f, t in zip(fbanks, self.T2)]
        out = torch.zeros((sum(self.T2), 8))
        off = np.concatenate([[0], np.cumsum(self.T2)]).tolist()
        return out, [out[a:b] for a, b in zip(off, off[1:])], None, None

    def ctc_both(self):
        res = [(tk, list(range(len(tk)))) for tk in self.toks]
        return res, res


class _StubEngine:
    """Enough of HipModel for the pools' host side: the scatter and the endpoint scan run the library's HOST entry points and count
    themselves, the fbank rows are zeros; any other device entry point fails the test."""
    cfg = _Cfg()
    device = "cpu"

    def __init__(self):
        self.scans, self.scatters = [], 0

    def stream_pool(self, max_sessions, max_rows):
        return _StubPool()

    def pcm_scatter(self, stage, stage_bytes, segs, dsts):
        self.scatters += 1
        raw = stage.numpy()
        for src, at, frames, code, ch, d in segs:
            fmt = PcmFormat({v: k for k, v in pcm.FORMATS.items()}[code], ch)
            dsts[d][at:at + frames] = torch.from_numpy(pcm.decode_host(raw[src:src + frames * fmt.bytes_per_frame].tobytes(), fmt))

    def vad_scan(self, segs, results):
        self.scans.append([tuple(s) for s in segs])
        for i, r in enumerate(EP.scan_host(segs)):
            results[EP.RESULT_BYTES * i:EP.RESULT_BYTES * (i + 1)] = torch.frombuffer(bytearray(bytes(r)), dtype=torch.uint8)

    def batch_fbank_frames(self, hist, first, cnt, outs, pcm_scale=32768.0):
        for h, f, n, o in zip(hist, first, cnt, outs):
            for r in range(n):
                o[r] = h[(f + r) * 160:(f + r) * 160 + 400].sum()

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


def _dicts():
    from streamspeech_amd.modules import Dictionary
    syms = [("" if i % 3 == 0 else "▁") + f"t{i}" for i in range(40)]
    return {"tgt": Dictionary.units(1000), "target_unigram": Dictionary(syms), "source_unigram": Dictionary(syms),
            "ctc_target_unigram": Dictionary(syms)}


def _s16(x):
    return np.round(x.astype(np.float64) * 32767.0).astype("<i2")


def _pool(n=4, rows=512):
    from streamspeech_amd.text_pool import TextSessionPool
    eng = _StubEngine()
    return eng, TextSessionPool(eng, n, rows)


CHUNK = 5120                                                                   # 320 ms at 16 kHz


def _fins(log, sid):
    """Steps that were an utterance's final call for the session (the text agents' final write itself does not say finished: their
    reset() runs before the segment is built)."""
    return sum(1 for st in log if st["endpoint_commits"].get(sid, (0, 0, False))[2])


def _drive(pool, streams, chunk=CHUNK, finish=False, log=None):
    """Feed every stream in chunks, one step per chunk, then step on while anyone is pending.  -> {sid: [segments]}."""
    outs = {sid: [] for sid in streams}
    n = max(len(x) for x in streams.values())
    for at in range(0, n, chunk):
        for sid, x in streams.items():
            if at < len(x):
                pool.push_pcm(sid, x[at:at + chunk].tobytes(), finished=finish and at + chunk >= len(x))
        for sid, seg in pool.step().items():
            outs[sid].append(seg)
        if log is not None:
            log.append(dict(pool.last_step))
    while any(s.pending for s in pool.sessions.values()):
        for sid, seg in pool.step().items():
            outs[sid].append(seg)
        if log is not None:
            log.append(dict(pool.last_step))
    return outs


def test_open_refusals_and_state():
    eng, pool = _pool()
    ep = Endpoint()
    with pytest.raises(ValueError, match="pcm_in"):
        pool.open("asr", _args(), dicts=_dicts(), endpoint=ep)
    with pytest.raises(ValueError, match="mp3_in"):
        pool.open("asr", _args(), dicts=_dicts(), mp3_in=True, endpoint=ep)
    for bad in ("default", True, {"threshold_db": -50}, Endpoint):
        with pytest.raises(ValueError, match="Endpoint"):
            pool.open("asr", _args(), dicts=_dicts(), pcm_in=PcmFormat("s16le"), endpoint=bad)
    with pytest.raises(ValueError, match="max_rows"):
        pool.open("asr", _args(), dicts=_dicts(), pcm_in=PcmFormat("s16le"), endpoint=Endpoint(max_utterance_ms=60000))
    assert pool.sessions == {} and pool._next == 0
    sid = pool.open("asr", _args(), dicts=_dicts(), pcm_in=PcmFormat("s16le"), endpoint=ep)
    e = pool.sessions[sid].ep
    # None: the longest utterance whose encoder rows fit max_rows, one sample more does not
    fit = e.p.max_utterance_samples
    from streamspeech_amd.text_pool import fbank_frames_after
    assert _enc_len(fbank_frames_after(16000, fit)) <= 512 < _enc_len(fbank_frames_after(16000, fit + 160))
    assert pool.backlog(sid) == 0 and pool.utterances(sid) == []
    plain = pool.open("asr", _args(), dicts=_dicts(), pcm_in=PcmFormat("s16le"))
    for f in (pool.backlog, pool.utterances):
        with pytest.raises(ValueError):
            f(plain)
    assert pool.sessions[plain].ep is None


def test_idle_sessions_hold_no_slot_and_more_sessions_than_slots():
    eng, pool = _pool(n=2)
    ep = Endpoint()
    sids = [pool.open("asr", _args(), dicts=_dicts(), pcm_in=PcmFormat("s16le"), endpoint=ep) for _ in range(4)]
    early, late = ((300, 1100),), ((2400, 3200),)
    streams = {sid: _s16(R.make_stream(16000, 40 + sid, early if i < 2 else late, 4600)) for i, sid in enumerate(sids)}
    seen, log = [], []
    n = len(streams[sids[0]])
    outs = {sid: [] for sid in sids}
    for at in range(0, n, CHUNK):
        for sid in sids:
            pool.push_pcm(sid, streams[sid][at:at + CHUNK].tobytes())
        res = pool.step()
        log.append(dict(pool.last_step))
        for sid in sids:
            outs[sid].append(res[sid])
            s = pool.sessions[sid]
            assert (s.slot is not None) == (s.ep.in_utt and not s.ep.final) or not s.ep.in_utt
            if not s.ep.in_utt and res[sid].is_empty:
                assert s.slot is None and s.fe.n_pcm == 0
        seen.append(sum(1 for s in pool.sessions.values() if s.slot is not None))
        assert seen[-1] + len(pool.free) == 2
    assert max(seen) == 2 and seen[0] == 0 and seen[-1] == 0
    for sid in sids:
        u = pool.utterances(sid)
        assert len(u) == 1 and u[0]["kind"] == "silence", u
        texts = [o for o in outs[sid] if not o.is_empty]
        assert texts and _fins(log, sid) == 1
        assert all(isinstance(o, EmptySegment) and not o.finished for o in outs[sid] if o.is_empty)
        # idle: the history is bounded by what a START may still reach back to, and a second of slack
        s = pool.sessions[sid]
        assert s.ep.held <= s.ep.p.idle_keep + 16000 + CHUNK + s.ep.p.idle_keep
    assert sum(st["endpoint_starts"] for st in log) == 4 == sum(st["endpoint_ends"] for st in log)
    assert all(st["vad_scan_calls"] == 1 and st["pcm_scatter_calls"] == 1 for st in log) and len(eng.scans) == len(log)
    assert all(len(sc) == 4 for sc in eng.scans)                               # ONE call for all four sessions of a step
    # frames handed to the scan: every frame once, and those behind a stop again in the next step
    assert sum(st["vad_frames"] for st in log) >= sum(pool.sessions[sid].ep.next_frame for sid in sids) == 4 * 458


def test_a_speaker_without_a_free_slot_waits():
    eng, pool = _pool(n=1)
    ep = Endpoint()
    a, b = (pool.open("asr", _args(), dicts=_dicts(), pcm_in=PcmFormat("s16le"), endpoint=ep) for _ in range(2))
    streams = {a: _s16(R.make_stream(16000, 5, ((300, 1100),), 3000)), b: _s16(R.make_stream(16000, 6, ((300, 1100),), 3000))}
    log = []
    outs = _drive(pool, streams, log=log)
    ua, ub = pool.utterances(a), pool.utterances(b)
    assert len(ua) == 1 and len(ub) == 1 and ua[0]["kind"] == ub[0]["kind"] == "silence"
    assert ua[0]["start"] == ub[0]["start"] == 28 * 160 - 3200                 # the same onset: b's utterance waited for a's slot
    assert _fins(log, a) == _fins(log, b) == 1 and len(pool.free) == 1 and any(not o.is_empty for o in outs[b])


def test_backlog_continues_without_a_push_and_the_only_size_refusal():
    eng, pool = _pool()
    sid = pool.open("asr", _args(), dicts=_dicts(), pcm_in=PcmFormat("s16le"), endpoint=Endpoint())
    x = _s16(R.make_stream(16000, 9))
    e = pool.sessions[sid].ep
    with pytest.raises(ValueError, match="longest utterance"):
        pool.push_pcm(sid, np.zeros(e.p.max_utterance_samples + 1, "<i2").tobytes())
    assert not pool.sessions[sid].pending and pool.backlog(sid) == 0
    pool.push_pcm(sid, x.tobytes())                                            # 4.6 s at once: two utterances
    assert pool.backlog(sid) == len(x)
    with pytest.raises(ValueError, match="already pushed"):
        pool.push_pcm(sid, x[:160].tobytes())
    first = pool.step()[sid]
    u = pool.utterances(sid)
    assert len(u) == 1 and not first.is_empty and pool.last_step["endpoint_starts"] == pool.last_step["endpoint_ends"] == 1
    assert pool.sessions[sid].pending and 0 < pool.backlog(sid) < len(x)       # the scan stopped at the cut
    assert pool.last_step["endpoint_commits"][sid] == (u[0]["start"], u[0]["end"] - u[0]["start"], True)
    b0, answers, log = pool.backlog(sid), [], []
    while pool.sessions[sid].pending:
        answers.append(pool.step()[sid])                                       # no push
        log.append(dict(pool.last_step))
        assert pool.last_step["pcm_scatter_calls"] == 0
    assert pool.backlog(sid) < b0 and pool.backlog(sid) < e.p.W + e.p.H
    u = pool.utterances(sid)
    assert [v["kind"] for v in u] == ["silence", "silence"] and u[0]["end"] <= u[1]["start"]
    assert _fins(log, sid) == 1 and any(not o.is_empty for o in answers)
    # the ranges are the reference's: the scan's events with pre-roll and cut as the issue defines them
    p = e.p
    assert u[0] == {"start": 58 * p.H - p.pre_roll_samples, "end": (219 + 1 + p.post_roll) * p.H + p.W - p.H, "kind": "silence"}
    pool.reset(sid)
    assert pool.utterances(sid) == [] and pool.backlog(sid) == 0 and e.next_frame == 0 and not e.dev_state.any()


def test_forced_cut_keeps_every_utterance_inside_the_limit():
    eng, pool = _pool(rows=24)                                                 # 24 encoder rows: about a second
    sid = pool.open("asr", _args(), dicts=_dicts(), pcm_in=PcmFormat("s16le"), endpoint=Endpoint())
    e = pool.sessions[sid].ep
    x = _s16(R.make_stream(16000, 12, ((300, 3300),), 4600))                   # three seconds of speech
    log = []
    outs = _drive(pool, {sid: x}, log=log)
    u = pool.utterances(sid)
    assert [v["kind"] for v in u][:-1] == ["forced"] * (len(u) - 1) and len(u) >= 3 and u[-1]["kind"] == "silence"
    for v, w in zip(u, u[1:]):
        assert v["end"] == w["start"]                                          # the next utterance begins at the cut
    assert all(0 < v["end"] - v["start"] <= e.p.max_utterance_samples for v in u)
    assert _fins(log, sid) == len(u)
    # what a step committed is contiguous inside an utterance and ends at its cut
    at = None
    for st in log:
        if sid in st["endpoint_commits"]:
            a, n, fin = st["endpoint_commits"][sid]
            assert at is None or a == at
            at = None if fin else a + n
            if fin:
                assert a + n in [v["end"] for v in u]


def test_stream_end_in_both_modes():
    eng, pool = _pool()
    ep = Endpoint()
    a = pool.open("asr", _args(), dicts=_dicts(), pcm_in=PcmFormat("s16le"), endpoint=ep)
    b = pool.open("asr", _args(), dicts=_dicts(), pcm_in=PcmFormat("s16le"), endpoint=ep)
    xa = _s16(R.make_stream(16000, 21, ((300, 1100),), 2560))                  # ends in silence behind an utterance
    xb = _s16(R.make_stream(16000, 22, ((300, 2560),), 2560))                  # ends mid-speech
    log = []
    outs = _drive(pool, {a: xa, b: xb}, finish=True, log=log)
    assert pool.utterances(a)[-1]["kind"] == "silence" and isinstance(outs[a][-1], EmptySegment) and outs[a][-1].finished
    assert _fins(log, a) == 1 and sum(1 for o in outs[a] if o.finished) == 1   # the utterance's end, then the stream's
    ub = pool.utterances(b)
    assert ub[-1] == {"start": ub[-1]["start"], "end": len(xb), "kind": "stream_end"}
    assert not outs[b][-1].is_empty and log[-1]["endpoint_commits"][b][2] and _fins(log, b) == len(ub)
    for sid in (a, b):
        assert not pool.sessions[sid].pending and pool.sessions[sid].slot is None
        with pytest.raises(ValueError, match="ended"):
            pool.push_pcm(sid, xa[:160].tobytes())
        pool.reset(sid)
        pool.push_pcm(sid, xa[:160].tobytes())
    assert len(pool.free) == 4


def test_equivalence_with_a_plain_session_and_non_interference():
    """The stub's answers depend on nothing but the samples an utterance has committed, so this pins the host logic: an endpointed
    session answers what a plain pcm_in session answers when it is fed the committed slices; and a plain session sharing its steps
    answers what it answers alone."""
    eng, pool = _pool()
    sid = pool.open("asr", _args(), dicts=_dicts(), pcm_in=PcmFormat("s16le"), endpoint=Endpoint())
    other = pool.open("asr", _args(), dicts=_dicts(), pcm_in=PcmFormat("s16le"))
    x, y = _s16(R.make_stream(16000, 31)), _s16(R.make_stream(16000, 32))[:5 * CHUNK]
    got, plain_got, commits = [], [], []
    for i, at in enumerate(range(0, len(x), CHUNK)):
        pool.push_pcm(sid, x[at:at + CHUNK].tobytes())
        if i < 5:
            pool.push_pcm(other, y[at:at + CHUNK].tobytes(), finished=i == 4)
        res = pool.step()
        got.append(res[sid])
        commits.append(pool.last_step["endpoint_commits"].get(sid))
        if i < 5:
            plain_got.append(res[other])
    assert pool.last_step["vad_scan_calls"] == 1
    eng2, ref = _pool()
    r1, r2 = (ref.open("asr", _args(), dicts=_dicts(), pcm_in=PcmFormat("s16le")) for _ in range(2))
    for i in range(5):
        ref.push_pcm(r2, y[i * CHUNK:(i + 1) * CHUNK].tobytes(), finished=i == 4)
        assert ref.step()[r2] == plain_got[i]
        assert ref.last_step["vad_scan_calls"] == 0 and ref.last_step["vad_frames"] == 0 and eng2.scans == []
    assert any(c is not None for c in commits) and any(c is None for c in commits)
    for seg, c in zip(got, commits):
        if c is None:
            assert isinstance(seg, EmptySegment) and not seg.finished
            continue
        a, n, fin = c
        ref.push_pcm(r1, x[a:a + n].tobytes(), finished=fin)
        assert ref.step()[r1] == seg
        if fin:
            ref.reset(r1)


# ---- the benchmark tool's host side -----------------------------------------------------------------------------------------------
def test_bench_tool_merges_runs(tmp_path):
    import importlib.util
    import json
    spec = importlib.util.spec_from_file_location("pooled_endpoint_bench", os.path.join(ROOT, "tools", "pooled_endpoint_bench.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)

    def run(path, t_ep, t_cut):
        runs = [{"sessions": 1, "side": "endpointed", "speaking_steps": tool._summary(t_ep, [x / 10 for x in t_ep]),
                 "silent_steps": tool._summary([1e-4], [9e-5]), "_t": t_ep, "_fe": [x / 10 for x in t_ep], "_ti": [1e-4], "_fi": [9e-5]},
                {"sessions": 1, "side": "caller-cut", "speaking_steps": tool._summary(t_cut, [x / 20 for x in t_cut]), "_t": t_cut,
                 "_fe": [x / 20 for x in t_cut]}]
        tool.write(str(path), {"workload": "w", "device": "d", "passes": 1, "runs": runs})
    run(tmp_path / "a.json", [0.003, 0.004, 0.005], [0.002, 0.003, 0.004])
    run(tmp_path / "b.json", [0.006, 0.007], [0.005, 0.006])
    tool.merge([str(tmp_path / "a.json"), str(tmp_path / "b.json")], str(tmp_path / "m.json"))
    with open(tmp_path / "m.json") as f:
        m = json.load(f)
    ep, cut = m["runs"]
    assert m["passes"] == 2 and m["merged_runs"] == 2 and ep["speaking_steps"]["steps"] == 5 == cut["speaking_steps"]["steps"]
    assert ep["speaking_steps"]["step_ms_median"] == 5.0 and cut["speaking_steps"]["step_ms_median"] == 4.0
    assert ep["extra_ms_per_speaking_step_median"] == 1.0 and ep["silent_steps"]["steps"] == 2
    assert ep["speaking_steps"]["frontend_share"] == 0.1
