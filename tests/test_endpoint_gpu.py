"""Endpointing of live PCM streams, on the GPU: the scan kernel against the library's own host twin (ss_vad_scan_host: the same inline
functions) bit for bit, its invariance under chunking, and the pools end to end -- an endpointed session answers, step for step and
byte for byte, what a plain pcm_in session answers when a caller who knew the utterance ranges feeds it the samples each step
committed."""
import os
import re

import numpy as np
import pytest
import torch

from tests import ref_fixtures as RF
from tests import vad_ref as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LDS_BATCH = 256                                  # csrc/vad.hip kBatch (checked below): frames a workgroup takes through LDS at a time
CANARY = np.float32(-777.25)


@pytest.fixture(scope="module")
def model(hip_model):
    return hip_model


def _endpoints():
    from streamspeech_amd.endpoint import Endpoint
    return Endpoint(max_utterance_ms=10000), Endpoint(max_utterance_ms=700)


def _segments(dev):
    """~70 segments of one call: four rates, frame counts around the wave count and the LDS batch, histories that begin at odd
    offsets of their buffers and of the frame grid, fresh and mid-utterance states (the host twin scanned up to the first frame)."""
    from streamspeech_amd import endpoint as EP
    with open(os.path.join(ROOT, "streamspeech_amd", "csrc", "vad.hip"), encoding="utf-8") as f:
        assert re.search(r"constexpr int kBatch = %d;" % LDS_BATCH, f.read())
    counts = (0, 1, 2, 63, 64, 65, LDS_BATCH + 1)
    segs = []
    for ri, sr in enumerate(R.RATES):
        x = R.make_stream(sr, 500 + sr)
        for ei, ep in enumerate(_endpoints()):
            p = ep.params(sr)
            total = p.frames_present(x.size)
            for ci, n in enumerate(counts):
                for first in ((0, 61, 150), (29, 70, 200), (67, 107, 190))[(ci + ei) % 3][:1 if ei else 2]:
                    n_eff = min(n, total - first)
                    state = np.zeros(EP.STATE_BYTES, np.uint8)
                    nxt = 0
                    while nxt < first:                                      # the state a stream has at `first`: stops included
                        nxt = R.host_scan(x, p, state, 0, nxt, first - nxt)["consumed"]
                    lead = (len(segs) * 7 + 3) % 11                        # samples of history before the first frame
                    h0 = first * p.H - lead if first else 0
                    hist = x[h0:(first + max(n_eff, 1) - 1) * p.H + p.W + (len(segs) % 5)].copy()
                    segs.append(dict(p=p, hist=hist, h0=h0, first=first, n=n_eff, state=state))
    assert 60 <= len(segs) <= 90
    assert any(R.state_dict(s["state"])["mode"] == EP.SPEECH for s in segs) and any(s["first"] == 0 and s["n"] > 0 for s in segs)
    return segs


def _device_call(model, segs, dev):
    """All segments in ONE ss_vad_scan: histories packed at odd offsets of one buffer, powers between canaries.
    -> (results bytes [n, 40], states bytes [n, 40], powers buffer as uint32, [(offset, n)])."""
    from streamspeech_amd import endpoint as EP
    off, at = [], 1
    for s in segs:
        off.append(at)
        at += s["hist"].size + 1 + (len(off) % 2)
    hist = np.zeros(at, np.float32)
    for s, o in zip(segs, off):
        hist[o:o + s["hist"].size] = s["hist"]
    poff, pat = [], 3
    for s in segs:
        poff.append(pat)
        pat += s["n"] + 3
    d_hist = torch.from_numpy(hist).to(dev)
    d_pw = torch.full((pat,), float(CANARY), dtype=torch.float32, device=dev)
    d_state = torch.from_numpy(np.stack([s["state"] for s in segs])).to(dev)
    d_res = torch.zeros((len(segs) * EP.RESULT_BYTES,), dtype=torch.uint8, device=dev)
    tup = [s["p"].seg(d_hist.data_ptr() + 4 * o, d_state.data_ptr() + EP.STATE_BYTES * i, d_pw.data_ptr() + 4 * po, s["h0"],
                      s["hist"].size, s["first"], s["n"]) for i, (s, o, po) in enumerate(zip(segs, off, poff))]
    model.vad_scan(tup, d_res)
    torch.cuda.synchronize()
    return (d_res.cpu().numpy().reshape(len(segs), -1), d_state.cpu().numpy(), d_pw.cpu().numpy().view(np.uint32), poff)


def test_scan_kernel_equals_host_twin(model):
    from streamspeech_amd import endpoint as EP
    segs = _segments(model.device)
    res, states, pw, poff = _device_call(model, segs, model.device)
    want_pw = np.full(pw.size, CANARY, np.float32)
    events = 0
    for i, (s, po) in enumerate(zip(segs, poff)):
        st = s["state"].copy()
        h_pw = want_pw[po:po + s["n"]] if s["n"] else None
        r = EP.scan_host([s["p"].seg(s["hist"].ctypes.data, st.ctypes.data, h_pw.ctypes.data if s["n"] else 0, s["h0"], s["hist"].size,
                                     s["first"], s["n"])])[0]
        assert bytes(r) == res[i].tobytes(), (i, R.result_dict(r))
        assert st.tobytes() == states[i].tobytes(), i
        events += bool(r.events)
    # powers bitwise, canaries on both sides of every range (and the frames behind a stop) untouched
    assert (pw == want_pw.view(np.uint32)).all(), int((pw != want_pw.view(np.uint32)).sum())
    assert events >= 10 and (want_pw != CANARY).sum() > 3000


def test_device_scan_is_invariant_under_chunking(model):
    from streamspeech_amd import endpoint as EP
    dev = model.device
    eps = _endpoints()
    jobs = [(sr, ep) for sr in R.RATES for ep in eps]
    xs = {sr: R.make_stream(sr, 900 + sr) for sr in R.RATES}
    d_x = {sr: torch.from_numpy(xs[sr]).to(dev) for sr in R.RATES}
    want = []
    for sr, ep in jobs:
        p = ep.params(sr)
        state = np.zeros(EP.STATE_BYTES, np.uint8)
        total = p.frames_present(xs[sr].size)
        ev = R.scan_all(lambda first, n: R.host_scan(xs[sr], p, state, 0, first, n), total, total)
        want.append((R.merge(ev), state.tobytes()))
    for chunk in (1, 7, 1 << 20):
        d_state = torch.zeros((len(jobs), EP.STATE_BYTES), dtype=torch.uint8, device=dev)
        d_res = torch.zeros((len(jobs) * EP.RESULT_BYTES,), dtype=torch.uint8, device=dev)
        nxt, evs = [0] * len(jobs), [[] for _ in jobs]
        ps = [ep.params(sr) for sr, ep in jobs]
        totals = [p.frames_present(xs[sr].size) for p, (sr, _) in zip(ps, jobs)]
        while any(a < t for a, t in zip(nxt, totals)):
            tup = [p.seg(d_x[sr].data_ptr(), d_state.data_ptr() + EP.STATE_BYTES * i, 0, 0, xs[sr].size, nxt[i], min(chunk, totals[i] - nxt[i]))
                   for i, (p, (sr, _)) in enumerate(zip(ps, jobs))]
            model.vad_scan(tup, d_res)                                      # every stream of the round in one launch
            for i, r in enumerate(EP.read_results(d_res.cpu().numpy(), len(jobs))):
                if r.events:
                    evs[i].append((r.events, r.start_frame, r.cut_sample))
                assert nxt[i] <= r.consumed <= totals[i]
                nxt[i] = int(r.consumed)
        states = d_state.cpu().numpy()
        for i in range(len(jobs)):
            assert (R.merge(evs[i]), states[i].tobytes()) == want[i], (chunk, jobs[i][0])


# ---- the pools, end to end ----------------------------------------------------------------------------------------------------------
BURSTS = ((300, 1100), (1400, 1900), (2800, 3400))       # a pause shorter than end_silence, then a longer one: two utterances
TOTAL_MS, CHUNK_MS = 4480, 320


def _encode(x, fmt):
    from streamspeech_amd import pcm
    return pcm.encode_host(x, fmt)


def _plan(synth_weights):
    """name -> (kind, args, pcm_in, pcm_out, stream bytes, bytes per sample, samples per chunk, endpointed)."""
    from streamspeech_amd import pcm
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.agent_text import StreamSpeechASRAgent, StreamSpeechS2TTAgent
    plan = {}
    for name, kind, cls, sr, fmt, out, ep in (
            ("asr", "asr", StreamSpeechASRAgent, 16000, "s16le", None, True),
            ("s2tt", "s2tt", StreamSpeechS2TTAgent, 16000, "s16le", None, True),
            ("s2st", "s2st", StreamSpeechS2STAgent, 16000, "s16le", "s16le", True),
            ("phone", "s2st", StreamSpeechS2STAgent, 8000, "ulaw", pcm.PcmOut("ulaw", 8000), True),
            ("plain", "s2st", StreamSpeechS2STAgent, 16000, "s16le", "s16le", False)):
        x = R.make_stream(sr, 70 + len(plan), BURSTS, TOTAL_MS, dc=0.0 if fmt == "ulaw" else 0.02)
        if not ep:
            x = x[:sr * 2]
        plan[name] = (kind, RF.agent_args(cls, CHUNK_MS, sr), pcm.PcmFormat(fmt), out, _encode(x, fmt), 2 if fmt == "s16le" else 1,
                      sr * CHUNK_MS // 1000, ep)
    return plan


def _run_endpointed(pool, plan, d, endpoint):
    """Feed every stream in 320-ms chunks, step on while anyone is pending.  -> per step ({name: segment}, {name: commit or None},
    last_step)."""
    sid = {n: pool.open(k, a, dicts=d, pcm_in=fi, pcm_out=fo, endpoint=endpoint if ep else None)
           for n, (k, a, fi, fo, _, _, _, ep) in plan.items()}
    steps, at = [], 0
    while True:
        pushed = False
        for n, (_, _, _, _, data, sb, per, ep) in plan.items():
            lo, hi = at * per * sb, (at + 1) * per * sb
            if lo < len(data):
                pool.push_pcm(sid[n], data[lo:hi], finished=hi >= len(data))
                pushed = True
        if not pushed and not any(s.pending for s in pool.sessions.values()):
            break
        res = pool.step()
        ls = dict(pool.last_step)
        steps.append(({n: res.get(sid[n]) for n in plan}, {n: ls["endpoint_commits"].get(sid[n]) for n in plan}, ls))
        at += 1
        assert at < 200
    return steps, {n: pool.utterances(sid[n]) for n in plan if plan[n][7]}


def _replay(pool, plan, d, steps):
    """Plain pcm_in sessions fed exactly the slices and finished flags the first run committed; every answer is compared."""
    sid = {n: pool.open(k, a, dicts=d, pcm_in=fi, pcm_out=fo) for n, (k, a, fi, fo, _, _, _, _) in plan.items()}
    at, compared, content = 0, 0, 0
    for got, commits, _ in steps:
        fins = []
        for n, (_, _, _, _, data, sb, per, ep) in plan.items():
            if ep:
                if commits[n] is not None:
                    a, cnt, fin = commits[n]
                    pool.push_pcm(sid[n], data[a * sb:(a + cnt) * sb], finished=fin)
                    if fin:
                        fins.append(n)
            else:
                lo, hi = at * per * sb, (at + 1) * per * sb
                if lo < len(data):
                    pool.push_pcm(sid[n], data[lo:hi], finished=hi >= len(data))
        res = pool.step()
        assert pool.last_step["vad_scan_calls"] == 0 and pool.last_step["vad_frames"] == 0
        for n in plan:
            want = res.get(sid[n])
            if plan[n][7] and commits[n] is None:                           # outside an utterance: EmptySegment, nothing was pushed
                assert want is None and got[n].is_empty
                continue
            if want is None:                                                # the plain session's stream is over: not stepped in either pool
                assert got[n] is None and not plan[n][7]
                continue
            assert type(got[n]) is type(want) and got[n] == want, (at, n, got[n], want)
            compared += 1
            content += bool(not want.is_empty and len(want.content))
        for n in fins:
            pool.reset(sid[n])
        at += 1
    return compared, content


def test_endpointed_sessions_equal_caller_cut_sessions(model, hip_vocoder, synth_weights):
    from streamspeech_amd.endpoint import Endpoint
    from streamspeech_amd.speech_pool import SpeechSessionPool
    d = RF.dictionaries(synth_weights[0])
    plan = _plan(synth_weights)
    steps, utts = _run_endpointed(SpeechSessionPool(model, 8, 512, vocoder=hip_vocoder), plan, d, Endpoint())
    for n, u in utts.items():
        assert [v["kind"] for v in u] == ["silence", "silence"], (n, u)
        sr = 8000 if n == "phone" else 16000
        H = sr // 100
        # the ranges are the issue's: pre-roll before the onset frame, post-roll and the window's tail behind the last speech frame
        assert u[0]["start"] == 28 * H - sr // 5 and u[0]["end"] == (189 + 1 + 20) * H + 15 * H // 10, (n, u)
        assert u[1]["start"] == 278 * H - sr // 5 and u[1]["end"] == (339 + 1 + 20) * H + 15 * H // 10, (n, u)
    assert all(ls["vad_scan_calls"] <= 1 for _, _, ls in steps) and sum(ls["vad_scan_calls"] for _, _, ls in steps) >= 14
    assert sum(ls["endpoint_starts"] for _, _, ls in steps) == 8 == sum(ls["endpoint_ends"] for _, _, ls in steps)
    # silent sessions hold no slot and encode nothing: the first step has only the plain session in the encoder
    assert steps[0][2]["encoded"] == 1 and all(steps[0][0][n].is_empty for n in utts)
    compared, content = _replay(SpeechSessionPool(model, 8, 512, vocoder=hip_vocoder), plan, d, steps)
    assert compared > 30 and content >= 6, (compared, content)


def test_forced_cut_on_a_small_pool_equals_caller_cut_sessions(model, hip_vocoder, synth_weights):
    from streamspeech_amd import pcm
    from streamspeech_amd.agent_text import StreamSpeechS2TTAgent
    from streamspeech_amd.endpoint import Endpoint
    from streamspeech_amd.speech_pool import SpeechSessionPool
    d = RF.dictionaries(synth_weights[0])
    x = R.make_stream(16000, 90, ((300, 3300),), 4480, dc=0.02)             # three seconds of speech, max_rows holds about one
    plan = {"long": ("s2tt", RF.agent_args(StreamSpeechS2TTAgent, CHUNK_MS, 16000), pcm.PcmFormat("s16le"), None, _encode(x, "s16le"), 2,
                     16000 * CHUNK_MS // 1000, True)}
    pool = SpeechSessionPool(model, 2, 24, vocoder=hip_vocoder)
    steps, utts = _run_endpointed(pool, plan, d, Endpoint())
    u = utts["long"]
    limit = next(iter(pool.sessions.values())).ep.p.max_utterance_samples
    assert len(u) >= 3 and [v["kind"] for v in u[:-1]] == ["forced"] * (len(u) - 1) and u[-1]["kind"] == "silence"
    assert all(v["end"] == w["start"] for v, w in zip(u, u[1:])) and all(0 < v["end"] - v["start"] <= limit for v in u)
    compared, content = _replay(SpeechSessionPool(model, 2, 24, vocoder=hip_vocoder), plan, d, steps)
    assert compared >= 10 and content >= 2, (compared, content)
