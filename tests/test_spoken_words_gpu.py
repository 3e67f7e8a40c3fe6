"""Where each translated word is spoken, end to end on the GPU with the seed-0 synthetic checkpoint: the offline driver
(--spoken-words), the S2ST agent (agent.spoken), the speech session pool (pool.spoken) and the latency bookkeeping over them.
The spans are checked against tests/spans_ref.py on the downloaded arg-max ids and durations; every other output is what it is
without the option, and with the option off the library's ss_batch_unit_spans is never called.

These tests show nothing unless units spread over states: each asserts that at least three words of its utterance hold units, and
the streaming ones that a write comes before the source ends."""
import filecmp
import os

import numpy as np
import pytest
import torch

from tests import ref_fixtures as RF
from tests import spans_ref as R
from tests.test_speech_pool_gpu import HipVocSurface

pytestmark = pytest.mark.gpu

TRACE = "s2st_320_b"          # a reference-agent trace of the suite: 320-ms chunks, two writes before the source ends, six words with units
TRACE_B = "s2st_640_a"        # another length in whole-word mode (a trailing <pad> state in the final write), for the pool
# (chosen on the CPU oracle path: of the suite's 320-ms traces, s2st_320_a and s2st_320_k3 give units to two words only)


class CountCalls:
    """Wraps the ctypes function of the engine's library and counts its calls."""

    def __init__(self, model, name="ss_batch_unit_spans"):
        self.model, self.name, self.calls = model, name, 0
        self.fn = getattr(model.lib, name)

    def __enter__(self):
        def counted(*a):
            self.calls += 1
            return self.fn(*a)
        self.lib = self.model.lib

        class Proxy:
            def __getattr__(_, k):
                return counted if k == self.name else getattr(self.lib, k)
        self.model.lib = Proxy()
        return self

    def __exit__(self, *exc):
        self.model.lib = self.lib


def _agent(model, hip_vocoder, cfg, case, spoken):
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.modules import StreamSpeechModel
    args = RF.agent_args(StreamSpeechS2STAgent, case["segment_ms"], case["sr"], case["over"], extra=("--spoken-words",) if spoken else ())
    return RF.set_dicts(StreamSpeechS2STAgent(args, model=StreamSpeechModel.from_engine(model), vocoder=HipVocSurface(hip_vocoder)), cfg)


def _check_spoken(sp, samples):
    assert sp is not None and sp.total_ms * 16 == samples
    assert sum(1 for w in sp.words if w.n_units > 0) >= 3, "the utterance does not spread units over three words: choose another"
    held = [w for w in sp.words if w.n_units > 0]
    assert all(a.start_ms <= b.start_ms for a, b in zip(held, held[1:])), "words are ordered by first token"
    assert all(0 <= w.start_ms <= w.end_ms <= sp.total_ms for w in sp.words)


# ---- offline ------------------------------------------------------------------------------------------------------------------------
def test_offline_spoken_words(hip_model, hip_vocoder, tmp_path):
    from streamspeech_amd import offline
    from streamspeech_amd.words import segments_from_spans, spoken_from_segments
    from tests import offline_fixture as OF
    from oracle.make_golden_offline import sample_pcm
    cfg = hip_model.cfg
    fix = OF.load()
    g = fix["groups"]["short_search"]
    meta = {s["id"]: s for s in fix["samples"]}
    ids = [int(i) for i in g["hypotheses"]]
    items = [(i, torch.from_numpy(sample_pcm(meta[i]["pcm_seed"], meta[i]["n_samples"])).to("cuda:0")) for i in ids]
    dicts = OF.ref_dicts(cfg)
    batches = []                                  # per batch: {"n", "raw", "toks", "K", "dur"} as the driver's calls saw them
    t2u, fwd, mtg = hip_model.batch_t2u_units, hip_vocoder.batch_forward, hip_model.batch_mt_greedy

    def mtg_spy(*a, **kw):
        out = mtg(*a, **kw)
        batches.append({"toks": [list(t) for t in out[0]]})
        return out

    def t2u_spy(feats, n, **kw):
        out = t2u(feats, n, **kw)
        if kw.get("keep_raw"):
            batches[-1].update(n=list(n), raw=out[-1].cpu().numpy().copy())
        return out

    def fwd_spy(codes, **kw):
        out = fwd(codes, **kw)
        batches[-1].update(K=[len(c) for c in codes], dur=out[1].cpu().numpy().copy())
        return out

    on, off = tmp_path / "on", tmp_path / "off"
    kw = dict(batch_size=3, max_len_b_mt=g["max_len_b_mt"])
    with CountCalls(hip_model) as cnt:
        off_hyps = offline.generate(hip_model, hip_vocoder, items, dicts, str(off), "test", **kw)
        assert cnt.calls == 0                     # option off: the entry point is never called
        hip_model.batch_t2u_units, hip_vocoder.batch_forward, hip_model.batch_mt_greedy = t2u_spy, fwd_spy, mtg_spy
        try:
            hyps = offline.generate(hip_model, hip_vocoder, items, dicts, str(on), "test", spoken_words=True, **kw)
        finally:
            del hip_model.batch_t2u_units, hip_vocoder.batch_forward, hip_model.batch_mt_greedy
        assert cnt.calls == sum(1 for b in batches if "dur" in b) >= 2          # one spans call per batch that speaks
    # every other file is byte-identical
    names = sorted(os.listdir(off))
    assert sorted(os.listdir(on)) == sorted(names + ["generate-test.spoken.words"])
    for nm in names:
        if os.path.isdir(off / nm):
            sub = sorted(os.listdir(off / nm))
            assert sub == sorted(os.listdir(on / nm))
            assert all(filecmp.cmp(off / nm / f, on / nm / f, shallow=False) for f in sub)
        else:
            assert filecmp.cmp(off / nm, on / nm, shallow=False), nm
    assert all(off_hyps[i]["units"] == hyps[i]["units"] for i in ids)
    # the reference on the downloaded raw and durations, batch by batch (rows without units take no part in the vocoder call)
    up, blank = cfg.ctc_upsample, cfg.unit_vocab - 1
    groups = offline.ordered_batches([int(p.numel()) for _, p in items], 3, 0)
    assert len(groups) == len(batches)
    lines = open(on / "generate-test.spoken.words", encoding="utf-8").read().splitlines()
    rich = 0
    for grp, bt in zip(groups, batches):
        o = od = j = 0
        for b, k in enumerate(grp):
            i = items[k][0]
            raw = bt["raw"][o: o + bt["n"][b] * up]
            o += bt["n"][b] * up
            mine = [ln for ln in lines if ln.split("\t")[0] == str(i)]
            if not hyps[i]["units"]:
                assert mine == [] and hyps[i]["spoken"] is None and not R.unit_mask(raw, blank, cfg.pad, R.BOS, cfg.eos).any()
                continue
            K = bt["K"][j]
            dur = bt["dur"][od: od + K]
            od, j = od + K, j + 1
            spans, kk = R.unit_spans(raw, up, blank, cfg.pad, R.BOS, cfg.eos, dur)
            assert kk == K == len(hyps[i]["units"])
            R.check_tiling(spans, 0, K, int(dur.sum()))                                   # every utterance's spans tile ...
            assert (spans[-1, 2] + spans[-1, 3]) * 320 == hyps[i]["wav"].numel()          # ... and end at len(wav) / 320
            sp = hyps[i]["spoken"]
            assert sp == spoken_from_segments(bt["toks"][b], segments_from_spans(spans, 0), dicts["target_unigram"], eos=cfg.eos)
            assert " ".join(w.text for w in sp.words) == hyps[i]["mt"]                    # one line per word of the D- text
            exp = [f"{i}\t{w.text}\t{w.start_ms}\t{w.end_ms}\t{w.n_units}" for w in sp.words]
            if sp.tail_ms > 0:
                exp.append(f"{i}\t</s>\t{sp.total_ms - sp.tail_ms}\t{sp.total_ms}\t0")
            assert mine == exp
            assert sp.total_ms * 16 == hyps[i]["wav"].numel()
            rich += sum(1 for w in sp.words if w.n_units > 0) >= 3
    assert rich >= 1, "no utterance of the fixture spreads units over three words"
    with pytest.raises(ValueError):
        offline.generate(hip_model, hip_vocoder, items[:1], dicts, str(tmp_path / "x"), "test", dump_wav=False, spoken_words=True)


# ---- the agent ----------------------------------------------------------------------------------------------------------------------
def _run(agent, case):
    recs = RF.run_case(agent, case)
    return recs, sum(len(c) for w, c, _ in recs if w)


def test_agent_spoken_words(hip_model, hip_vocoder, synth_weights):
    from streamspeech_amd import streaming_eval as E
    cfg = synth_weights[0]
    _, cases = RF.traces_gold()
    case = cases[TRACE]
    with CountCalls(hip_model) as cnt:
        plain, n_plain = _run(_agent(hip_model, hip_vocoder, cfg, case, False), case)
        assert cnt.calls == 0
        agent = _agent(hip_model, hip_vocoder, cfg, case, True)
        assert agent.spoken is None
        recs, n = _run(agent, case)
        writes = sum(1 for w, c, _ in recs if w and len(c) > 0)
        assert cnt.calls == writes
    assert [w for w, _, _ in recs[:-1]].count(True) >= 1, "no write before the source ends: choose another utterance"
    assert recs == plain and n == n_plain                        # waveform (bit for bit), actions and flags as without the flag
    _check_spoken(agent.spoken, n)                               # readable after the final write's reset()
    first = agent.spoken
    # the latency bookkeeping over the same audio through a fresh agent
    pcm = RF.trace_pcm(case["seed"], case["sr"], case["seconds"])
    agent = _agent(hip_model, hip_vocoder, cfg, case, True)
    r = E.run_utterance(agent, pcm, segment_ms=case["segment_ms"], sr=case["sr"], spoken=True)
    assert agent.spoken == first and r["samples_out"] == n
    assert len(r["spoken_words"]) == len(first.words)
    for w in r["spoken_words"]:
        assert w["play_start_ms"] >= r["StartOffset"] and w["play_end_ms"] <= r["source_ms"] + r["EndOffset"] + 1e-6
    for k in ("BOW", "COW", "EOW"):
        assert sorted(r["SpeechAlign"][k]) == ["AL", "AP", "DAL", "LAAL"]
    assert all(w["play_start_ms"] < w["play_end_ms"] for w in r["spoken_words"] if w["n_units"] > 0)
    assert "SpeechAlign" not in E.run_utterance(_agent(hip_model, hip_vocoder, cfg, case, True), pcm, segment_ms=case["segment_ms"],
                                                sr=case["sr"])


# ---- the pool -----------------------------------------------------------------------------------------------------------------------
def _drive_pool(pool, plan, cfg):
    """plan: {name: (args, pcm, sr, segment_ms, open keywords)} -> ({name: contents per step}, {name: sid})."""
    from streamspeech_amd.simuleval_shim import SpeechSegment
    d = RF.dictionaries(cfg)
    sid = {name: pool.open("s2st", p[0], dicts=d, **p[4]) for name, p in plan.items()}
    pos = {name: 0 for name in plan}
    out = {name: [] for name in plan}
    done = set()
    steps = []
    while len(done) < len(plan):
        segs = {}
        for name, (args, pcm, sr, ms, _) in plan.items():
            if name in done:
                continue
            step = sr * ms // 1000
            chunk = pcm[pos[name]:pos[name] + step]
            pos[name] += step
            segs[sid[name]] = SpeechSegment(content=chunk.tolist(), sample_rate=sr, finished=pos[name] >= len(pcm))
            if pos[name] >= len(pcm):
                done.add(name)
        res = pool.step(segs)
        steps.append(dict(pool.last_step))
        for name in plan:
            if sid[name] in res and not res[sid[name]].is_empty:
                out[name].append(res[sid[name]].content)
    return out, sid, steps


def test_pool_spoken_words(hip_model, hip_vocoder, synth_weights):
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.pcm import PcmOut
    from streamspeech_amd.speech_pool import SpeechSessionPool
    cfg = synth_weights[0]
    _, cases = RF.traces_gold()
    want, plan = {}, {}
    for name in (TRACE, TRACE_B):
        case = cases[name]
        agent = _agent(hip_model, hip_vocoder, cfg, case, True)
        _, n = _run(agent, case)
        want[name] = (agent.spoken, n)
        args = RF.agent_args(StreamSpeechS2STAgent, case["segment_ms"], case["sr"], case["over"])
        plan[name] = (args, RF.trace_pcm(case["seed"], case["sr"], case["seconds"]), case["sr"], case["segment_ms"], {})
    assert len(plan[TRACE][1]) != len(plan[TRACE_B][1])          # sessions at two different lengths in one pool
    plan["ulaw"] = plan[TRACE][:4] + ({"pcm_out": PcmOut("ulaw", sample_rate=8000)},)
    with CountCalls(hip_model) as cnt:
        pool = SpeechSessionPool(hip_model, 8, 512, vocoder=hip_vocoder, spoken=True)
        out, sid, steps = _drive_pool(pool, plan, cfg)
        assert cnt.calls == sum(s.get("span_calls", 0) for s in steps) > 0
        assert all(s.get("span_calls", 0) == s.get("vocoder_tail_calls", 0) <= 1 for s in steps if "vocoder_tail_calls" in s)
        assert any("spans_s" in s for s in steps)
        for name in (TRACE, TRACE_B):
            sp, n = want[name]
            _check_spoken(sp, n)
            assert pool.spoken(sid[name]) == sp
            assert sum(len(c) for c in out[name]) == n
        assert pool.spoken(sid["ulaw"]) == want[TRACE][0]        # times of the speech, not byte offsets of the 8-kHz answer
        assert sum(len(c) for c in out["ulaw"]) < want[TRACE][1]
        pool.reset(sid[TRACE])
        assert pool.spoken(sid[TRACE]) is None
        before = cnt.calls
        plain = SpeechSessionPool(hip_model, 8, 512, vocoder=hip_vocoder)
        out2, sid2, steps2 = _drive_pool(plain, {k: plan[k] for k in (TRACE, TRACE_B)}, cfg)
        assert cnt.calls == before and plain.spoken(sid2[TRACE]) is None
        assert not any("spans_s" in s or "span_calls" in s for s in steps2)
        assert out2[TRACE] == out[TRACE] and out2[TRACE_B] == out[TRACE_B]      # the segments are the same either way
