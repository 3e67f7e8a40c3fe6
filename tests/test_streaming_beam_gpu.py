"""Beam search behind a forced prefix on the GPU (ss_batch_mt_beam_continue, beam.hip) against the reference's offline generator
run with prefix_tokens (fixture tests/golden/streaming_beam.json, written by tests/make_golden_beam_prefix.py): identical n-best
token lists and order, scores within tau / 4 and positional scores within tau for every case whose decisive margin exceeds tau.
Beam 1 is the greedy continuation (ss_batch_mt_continue) bit for bit; no prefix anywhere is the offline beam (ss_batch_mt_beam) bit
for bit; forcing a finished hypothesis re-scores it; an utterance's n-best list is the same alone, in mixed packs and across a split
of more than 256 rows; the scratch books hold; every refusal of the host planner is the device call's, before any launch.

Score identity checked on every hypothesis this file sees (`_check_hyp`): it starts with its prefix, and its score equals the
in-order float32 sum of its positional scores, divided by the length when normalised, WITHIN 1 ULP (not to the last bit: a
positional score is a float32 difference of two cumulative scores, so their sum need not round back to the last cumulative score)."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "streaming_beam.json")
OFFLINE = os.path.join(ROOT, "tests", "golden", "offline_beam.json")


def _fix():
    return json.load(open(FIX, encoding="utf-8"))


def _model_for(group, hip_model, synth_weights):
    if group["eos_scale"] == 1.0:
        return hip_model
    from streamspeech_amd.engine import HipModel
    from tests.make_golden_beam import state_dict
    cfg = synth_weights[0]
    g = np.load(os.path.join(ROOT, "tests", "golden", "gcmvn_fr-en.npz"))
    return HipModel(state_dict(group["eos_scale"], cfg), cfg, cmvn_mean=g["mean"], cmvn_std=g["std"])


def _encode(model, pcms):
    lens = [int(p.numel()) for p in pcms]
    feat, T = model.batch_fbank_cmvn(torch.cat(pcms).cuda(), lens)
    return model.batch_encoder_forward(feat, T)


def _pcm(rec):
    from tests.make_golden_beam import sample_pcm
    return torch.from_numpy(sample_pcm(rec["pcm_seed"], rec["n_samples"]))


def _bits(x):
    return struct.pack("<f", x)


def _ulp_apart(a, b):
    ia, ib = (struct.unpack("<i", struct.pack("<f", v))[0] for v in (a, b))
    return abs(ia - ib)


def _check_hyp(h, prefix, normalize):
    assert h["tokens"][:len(prefix)] == list(prefix), "a hypothesis starts with its prefix"
    assert len(h["positional_scores"]) == len(h["tokens"])
    s = np.float32(0.0)
    for p in h["positional_scores"]:
        s = np.float32(s + np.float32(p))
    if normalize:
        s = np.float32(s / np.float32(len(h["tokens"])))
    assert _ulp_apart(float(s), h["score"]) <= 1, f"score {h['score']} vs in-order sum {float(s)}"


def _synthetic(n, seed0):
    from streamspeech_amd import synth, workload
    utts = sorted(workload.make_utterances(60), key=lambda u: u.seconds)[:n]
    return [torch.from_numpy(synth.synth_pcm(seed0 + u.idx, u.n_samples)) for u in utts]


def _key(h):
    return [(x["tokens"], _bits(x["score"]), [_bits(p) for p in x["positional_scores"]]) for x in h]


@pytest.mark.parametrize("name", ["beam4", "beam10_early_eos", "beam5_unnorm_unkpen"])
def test_forced_beam_nbest_equals_reference(name, hip_model, synth_weights):
    grp = _fix()["groups"][name]
    model = _model_for(grp, hip_model, synth_weights)
    seen_unk = seen_full = 0
    on = {r["sid"]: r["prefix"] for r in grp["cases"]["on"]}
    assert all(r["prefix"] != on[r["sid"]] for r in grp["cases"]["off"]), "an off-path prefix differs from the on-path one"
    for kind, cases in grp["cases"].items():
        if not cases:                      # a group without a case of this kind (no hypothesis of max_len tokens to force)
            continue
        enc, Tp = _encode(model, [_pcm(r) for r in cases])
        nbest, feats = model.batch_mt_beam_continue(enc, Tp, [r["prefix"] for r in cases], [grp["max_len_b_mt"]] * len(cases),
                                                    grp["beam"], 1, grp["unk_penalty"], grp["normalize"])
        worst, worst_pos, under = 0.0, 0.0, []
        for rec, hyps, f in zip(cases, nbest, feats):
            for h in hyps:
                _check_hyp(h, rec["prefix"], grp["normalize"])
            assert f.shape[0] == len(hyps[0]["tokens"])
            if not rec["margin"] > rec["tau"]:
                under.append(rec["sid"])
                continue
            ref = rec["nbest"]
            assert [h["tokens"] for h in hyps] == [h["tokens"] for h in ref], f"{name}/{kind} sample {rec['sid']}: n-best tokens / order"
            for h, r in zip(hyps, ref):
                d = abs(h["score"] - r["score"])
                dp = float(np.abs(np.array(h["positional_scores"]) - np.array(r["positional_scores"])).max())
                worst, worst_pos = max(worst, d), max(worst_pos, dp)
                assert d < rec["tau"] / 4, f"{name}/{kind} sample {rec['sid']}: score {h['score']} vs {r['score']}"
                assert dp < rec["tau"]
            seen_unk += model.cfg.unk in rec["prefix"] and grp["unk_penalty"] != 0
            seen_full += len(rec["prefix"]) == grp["max_len_b_mt"]
        print(f"{name}/{kind}: worst |HIP - reference| score {worst:.3g}, positional {worst_pos:.3g}; cases under the margin "
              f"(not compared): {len(under)} {under}")
        if kind in ("on", "off"):
            assert len(cases) - len(under) >= 6
    if grp["unk_penalty"]:
        assert seen_unk >= 1, "a forced <unk> under a non-zero unk_penalty"
    if "full" in grp["cases"] and grp["cases"]["full"]:
        assert seen_full >= 1, "a case with n_prefix == max_len"


def _offline_utterances(hip_model):
    from tests.offline_fixture import load
    from oracle.make_golden_offline import sample_pcm
    fix = load()
    pcms = [torch.from_numpy(sample_pcm(s["pcm_seed"], s["n_samples"])) for s in fix["samples"]]
    return _encode(hip_model, pcms)


def test_beam1_is_the_greedy_continuation(hip_model):
    enc, Tp = _offline_utterances(hip_model)
    for ml in (10, 40):
        mx = [ml] * len(Tp)
        free, _, _ = hip_model.batch_mt_greedy(enc, Tp, mx)
        lens = [0, 1, 7, ml]
        prefixes = []
        for b in range(len(Tp)):
            body = [t for t in free[b] if t != hip_model.cfg.eos]
            n = min(lens[b % 4], len(body))
            if lens[b % 4] == ml and len(body) < ml:       # a full-length prefix needs max_len tokens: repeat the body
                body = (body * ml)[:ml]
                n = ml
            prefixes.append(body[:n])
        assert {len(p) for p in prefixes} >= {0, 1, 7, ml}
        ref = hip_model.batch_mt_continue(enc, Tp, prefixes, mx)
        nbest, feats = hip_model.batch_mt_beam_continue(enc, Tp, prefixes, mx, 1)
        for b in range(len(Tp)):
            _check_hyp(nbest[b][0], prefixes[b], True)
            assert len(nbest[b]) == 1
            assert nbest[b][0]["tokens"] == prefixes[b] + ref[b][0], f"row {b} (prefix {len(prefixes[b])})"
            assert feats[b].shape == ref[b][1].shape and torch.equal(feats[b], ref[b][1]), f"row {b}: decoder states"


def test_ragged_continuations_share_one_decode_step(hip_model):
    """A pack of three rows behind prefixes of 0, 3 and 7 tokens, the last with max_len == n_prefix (it takes no lock-step step): at
    beam 1 the forced beam search is batch_mt_continue bit for bit, tokens and decoder states, and every row of batch_mt_continue
    generates what mt_greedy generates behind the same prefix."""
    enc, Tp = _offline_utterances(hip_model)
    Tp = [int(t) for t in Tp[:3]]
    enc = enc[:sum(Tp)]
    free, _, _ = hip_model.batch_mt_greedy(enc, Tp, [12] * 3)
    prefixes = []
    for b, n in enumerate((0, 3, 7)):
        body = [t for t in free[b] if t != hip_model.cfg.eos]
        prefixes.append((body * n)[:n])                   # a short search: repeat its tokens
    assert [len(p) for p in prefixes] == [0, 3, 7]
    mx = [10, 10, 7]
    ref = hip_model.batch_mt_continue(enc, Tp, prefixes, mx)
    nbest, feats = hip_model.batch_mt_beam_continue(enc, Tp, prefixes, mx, 1)
    assert ref[2][0] == [hip_model.cfg.eos], "the full-length prefix is followed by the forced </s> alone"
    off = np.concatenate([[0], np.cumsum(Tp)])
    for b in range(3):
        assert len(nbest[b]) == 1
        assert nbest[b][0]["tokens"] == prefixes[b] + ref[b][0], f"row {b} (prefix {len(prefixes[b])})"
        assert feats[b].shape == ref[b][1].shape and torch.equal(feats[b], ref[b][1]), f"row {b}: decoder states"
        alone, _ = hip_model.mt_greedy(enc[int(off[b]):int(off[b + 1])], prefixes[b], mx[b])
        assert alone == ref[b][0], f"row {b}: batch_mt_continue against mt_greedy"


def test_no_prefix_is_the_offline_beam(hip_model):
    enc, Tp = _offline_utterances(hip_model)
    mx = [12 + (b % 3) for b in range(len(Tp))]
    for beam in (4, 10):
        ref, rf, rn = hip_model.batch_mt_beam(enc, Tp, mx, beam)
        got, gf = hip_model.batch_mt_beam_continue(enc, Tp, [[] for _ in Tp], mx, beam)
        for b in range(len(Tp)):
            assert _key(got[b]) == _key(ref[b]), f"beam {beam} utterance {b}"
            assert torch.equal(gf[b], rf[b, :rn[b]])
            for h in got[b]:
                _check_hyp(h, [], True)


@pytest.mark.parametrize("name", ["beam4", "beam10_early_eos"])
def test_forcing_a_hypothesis_rescores_it(name, hip_model, synth_weights):
    """Every hypothesis y_1 .. y_n </s> of a pinned search, forced whole with max_len = n: the ragged prefix pass and the prefix-score
    kernel must give the positional scores the k lock-step steps gave (within tau; the score within tau / 4).  Measured on the
    MI355X: worst difference 3.6e-7 (score) / 1.9e-6 (positional) over 24 hypotheses at beam 4, 1.4e-6 / 7.6e-6 over 60 at beam 10 --
    not 0.0, so the two routes do not share bits and the bars stay tolerances."""
    fix = json.load(open(OFFLINE, encoding="utf-8"))["groups"][name]
    model = _model_for(fix, hip_model, synth_weights)
    recs = [r for r in fix["hypotheses"].values() if r["margin"] > r["tau"]]
    enc, Tp = _encode(model, [_pcm(r) for r in recs])
    off = np.concatenate([[0], np.cumsum(Tp)])
    nbest, _, _ = model.batch_mt_beam(enc, Tp, [fix["max_len_b_mt"]] * len(recs), fix["beam"], 1, fix["unk_penalty"], fix["normalize"])
    rows, pre, taus, orig = [], [], [], []
    for b, (rec, hyps) in enumerate(zip(recs, nbest)):
        for h in hyps:
            if len(h["tokens"]) < 2:
                continue
            rows.append(b); pre.append(h["tokens"][:-1]); taus.append(rec["tau"]); orig.append(h)
    enc_r = torch.cat([enc[off[b]:off[b + 1]] for b in rows])
    got, _ = model.batch_mt_beam_continue(enc_r, [Tp[b] for b in rows], pre, [len(p) for p in pre], fix["beam"], 1,
                                          fix["unk_penalty"], fix["normalize"])
    worst_s = worst_p = 0.0
    for g, p, t, o in zip(got, pre, taus, orig):
        assert len(g) == 1 and g[0]["tokens"] == o["tokens"]
        _check_hyp(g[0], p, fix["normalize"])
        ds = abs(g[0]["score"] - o["score"])
        dp = float(np.abs(np.array(g[0]["positional_scores"]) - np.array(o["positional_scores"])).max())
        worst_s, worst_p = max(worst_s, ds), max(worst_p, dp)
        assert ds < t / 4 and dp < t
    print(f"{name}: {len(got)} hypotheses re-scored by forcing; worst difference score {worst_s:.3g}, positional {worst_p:.3g}"
          + (" -- 0.0 everywhere: the two routes share bits" if worst_s == 0.0 and worst_p == 0.0 else ""))


def test_forced_beam_pack_invariance_and_split(hip_model):
    pcms = _synthetic(30, 900)
    enc, Tp = _encode(hip_model, pcms)
    off = np.concatenate([[0], np.cumsum(Tp)])
    beam, ml = 10, 12
    mx = [ml + (b % 3) for b in range(len(Tp))]
    free, _, _ = hip_model.batch_mt_greedy(enc, Tp, mx)
    lens = [0, 3, 1, 7, 0, 5]
    pre = [[t for t in free[b] if t != hip_model.cfg.eos][:lens[b % len(lens)]] for b in range(len(Tp))]
    whole, wf = hip_model.batch_mt_beam_continue(enc, Tp, pre, mx, beam)       # 300 rows: split 25 + 5
    for b in (0, 7, 26, 29):
        alone, af = hip_model.batch_mt_beam_continue(enc[off[b]:off[b + 1]], [Tp[b]], [pre[b]], [mx[b]], beam)
        assert _key(alone[0]) == _key(whole[b]), f"utterance {b}: alone vs in a split pack of {len(Tp)}"
        assert torch.equal(af[0], wf[b])
    sel = [26, 3, 11]
    enc3 = torch.cat([enc[off[b]:off[b + 1]] for b in sel])
    three, tf = hip_model.batch_mt_beam_continue(enc3, [Tp[b] for b in sel], [pre[b] for b in sel], [mx[b] for b in sel], beam)
    for j, b in enumerate(sel):
        assert _key(three[j]) == _key(whole[b]) and torch.equal(tf[j], wf[b])
    for b in range(len(Tp)):
        for h in whole[b]:
            _check_hyp(h, pre[b], True)
    assert {len(pre[b]) for b in (0, 7, 26, 29, 3, 11)} >= {0, 1, 3}


def test_forced_beam_keeps_scratch_books_and_cap(hip_model):
    from streamspeech_amd import lib as L
    from streamspeech_amd.engine import Scratch
    sc = Scratch()
    m = hip_model.new_context(scratch=sc)
    enc, Tp = _encode(m, _synthetic(6, 950))
    free, _, _ = m.batch_mt_greedy(enc, Tp, [12] * len(Tp))
    pre = [[t for t in free[b] if t != m.cfg.eos][:b] for b in range(len(Tp))]
    booked0, _ = sc.audit()
    ref, rf = m.batch_mt_beam_continue(enc, Tp, pre, [12] * len(Tp), 8)
    booked, held = sc.audit()
    assert booked == held and booked > booked0
    sc.trim(0)
    sc.set_cap(sc.bytes() + (1 << 20))
    with pytest.raises(L.StreamSpeechHipError) as e:
        m.batch_mt_beam_continue(enc, Tp, pre, [12] * len(Tp), 8)
    assert e.value.code == L.SS_ERR_SCRATCH_CAP
    booked, held = sc.audit()
    assert booked == held
    sc.set_cap(0)
    got, gf = m.batch_mt_beam_continue(enc, Tp, pre, [12] * len(Tp), 8)
    assert got == ref and all(torch.equal(a, b) for a, b in zip(gf, rf))
    for hyps, p in zip(ref, pre):
        for h in hyps:
            _check_hyp(h, p, True)


def test_forced_beam_refusals_are_the_planners(hip_model):
    """Every refusal of ss_batch_mt_beam_continue_plan comes from the device call too, with the same code and before any launch; a
    valid call right after each refusal gives the bits it gave before."""
    from streamspeech_amd import lib as L
    from streamspeech_amd.engine import ContinueRefused, Scratch, plan_mt_beam_continue
    from tests.test_streaming_beam_cpu import REFUSALS
    sc = Scratch()
    m = hip_model.new_context(scratch=sc)
    enc, Tp = _encode(m, _synthetic(1, 990))
    cfg = m.cfg
    lib = L.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    ref, rf = m.batch_mt_beam_continue(enc, Tp, [[5, 6]], [10], 4)
    for h in ref[0]:
        _check_hyp(h, [5, 6], True)
    for case in REFUSALS:
        B, beam = case["B"], case["beam"]
        tp = [Tp[0] if t is None else t for t in case["Tp"]]
        with pytest.raises(ContinueRefused) as e:
            plan_mt_beam_continue(tp, case["n_prefix"], case["max_len"], beam, case.get("min_len", 1), feat_rows=case["feat_rows"],
                                  out_stride=case["out_stride"],
                                  max_tgt_pos=case.get("planner_max_tgt_pos") or m.max_tgt_pos,
                                  prefix_ids=case["ids"], vocab=cfg.tgt_vocab, eos=cfg.eos, pad=cfg.pad)
        assert e.value.code == case["code"], case["name"]
        if case.get("planner_max_tgt_pos") is not None:
            continue                                       # a position bound of another table size: the planner's case only
        n = max(B * beam, 1)
        feats = torch.zeros((max(B, 1), max(case["feat_rows"], 1), cfg.dec_dim), device="cuda")
        out = (C.c_int32 * (n * max(case["out_stride"], 1)))()
        n_out, s = (C.c_int32 * n)(), (C.c_float * n)()
        i32 = lambda v: (C.c_int32 * max(len(v), 1))(*v)   # noqa: E731
        torch.cuda.synchronize()
        before = sc.bytes()
        rc = lib.ss_batch_mt_beam_continue(m.h, stream, B, beam, C.c_void_p(enc.data_ptr()), i32(tp), i32(case["ids"]),
                                           i32(case["n_prefix"]), i32(case["max_len"]), case.get("min_len", 1), 0.0, 1, out,
                                           case["out_stride"], n_out, s, None, C.c_void_p(feats.data_ptr()), case["feat_rows"])
        torch.cuda.synchronize()
        assert rc == case["code"], case["name"]
        assert sc.bytes() == before and torch.count_nonzero(feats) == 0, case["name"]
        got, gf = m.batch_mt_beam_continue(enc, Tp, [[5, 6]], [10], 4)
        assert _key(got[0]) == _key(ref[0]) and torch.equal(gf[0], rf[0]), f"after refusing {case['name']}"
        for h in got[0]:
            _check_hyp(h, [5, 6], True)


# ---- agents and pools ------------------------------------------------------------------------------------------------------------------
BATCH_RMS_TOL = 1e-5        # pool against single-session agents: the bar of tests/test_speech_pool_gpu.py


class _VocSurface:
    """CodeHiFiGANVocoderWithDur call surface over the shared fixture handle (as tests/test_speech_pool_gpu.py)."""

    def __init__(self, hv):
        self.hip = hv

    def __call__(self, x, dur_prediction=False):
        from streamspeech_amd.modules import CodeHiFiGANVocoderWithDur
        return CodeHiFiGANVocoderWithDur.__call__(self, x, dur_prediction)


def _agent(kind, hip_model, hip_vocoder, cfg, segment_ms, flags):
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.agent_text import StreamSpeechS2TTAgent
    from streamspeech_amd.modules import StreamSpeechModel
    from tests import ref_fixtures as RF
    model = StreamSpeechModel.from_engine(hip_model.new_context())     # its own context: a greedy agent arms the persistent MT step
    if kind == "s2st":
        return RF.set_dicts(StreamSpeechS2STAgent(RF.agent_args(StreamSpeechS2STAgent, segment_ms, 16000, extra=flags), model=model,
                                                  vocoder=_VocSurface(hip_vocoder)), cfg)
    return RF.set_dicts(StreamSpeechS2TTAgent(RF.agent_args(StreamSpeechS2TTAgent, segment_ms, 16000, extra=flags), model=model), cfg)


def _run_agent(agent, pcm, segment_ms=320, sr=16000):
    """-> per policy() call (is_write, content, finished, committed text tokens, units so far)."""
    from streamspeech_amd.simuleval_shim import SpeechSegment
    step, pos, recs = sr * segment_ms // 1000, 0, []
    while True:
        chunk = pcm[pos:pos + step]
        pos += step
        fin = pos >= len(pcm)
        o = agent.pushpop(SpeechSegment(content=chunk.tolist(), sample_rate=sr, finished=fin))
        t = agent.tgt_subwords_indices
        recs.append((not o.is_empty, None if o.is_empty else o.content, bool(o.finished),
                     None if t is None else [int(x) for x in t.view(-1).tolist()],
                     None if getattr(agent, "unit", None) is None else list(agent.unit)))
        if fin:
            return recs


@pytest.mark.parametrize("kind", ["s2tt", "s2st"])
def test_agents_with_a_beam_end_to_end(kind, hip_model, hip_vocoder, synth_weights):
    from streamspeech_amd import synth
    cfg = synth_weights[0]
    for seed, secs in ((3, 2.0), (4, 3.2)):
        pcm = synth.synth_pcm(seed, int(16000 * secs))
        recs = _run_agent(_agent(kind, hip_model, hip_vocoder, cfg, 320, ["--beam-mt", "4"]), pcm)
        committed, writes = [], 0
        for w, content, fin, toks, _ in recs:
            writes += w
            if toks is not None:                         # committed tokens are never rewritten: every write extends the text prefix
                assert toks[:len(committed)] == committed, "a write rewrote committed tokens"
                committed = toks
        assert writes >= 1 and len(recs) == -(-len(pcm) // 5120)          # the run finishes: one policy() call per segment
        # --beam-mt 1 builds and computes exactly what the agent without the flag does
        plain = _run_agent(_agent(kind, hip_model, hip_vocoder, cfg, 320, []), pcm)
        one = _run_agent(_agent(kind, hip_model, hip_vocoder, cfg, 320, ["--beam-mt", "1"]), pcm)
        assert [(w, f, t, u) for w, _, f, t, u in one] == [(w, f, t, u) for w, _, f, t, u in plain]
        for (_, a, _, _, _), (_, b, _, _, _) in zip(one, plain):
            assert (a == b) if (a is None or isinstance(a, str)) else np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.parametrize("kind,ms", [("s2tt", 320), ("s2st", 320), ("s2st", 640)])
def test_pools_with_a_beam_match_single_agents(kind, ms, hip_model, hip_vocoder, synth_weights):
    """Six sessions of different lengths in one pool with beam_mt = 4 against six single agents with --beam-mt 4: the same text, the
    same units, the waveform within the batched-vocoder bar.  At 640 ms the S2ST sessions run in whole-word mode: a final write
    carries a trailing <pad>, whose decoder state the agent takes from batch_mt_features at a beam (no KV cache to append to)."""
    from streamspeech_amd import synth
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.agent_text import StreamSpeechS2TTAgent
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.speech_pool import SpeechSessionPool
    from streamspeech_amd.text_pool import TextSessionPool
    from tests import ref_fixtures as RF
    cfg = synth_weights[0]
    pcms = [synth.synth_pcm(4000 + i, int(16000 * (1.0 + 0.6 * i))) for i in range(6)]
    step = 16 * ms
    cls = StreamSpeechS2STAgent if kind == "s2st" else StreamSpeechS2TTAgent
    pool = (SpeechSessionPool(hip_model, 8, 256, vocoder=hip_vocoder, beam_mt=4) if kind == "s2st"
            else TextSessionPool(hip_model, 8, 256, beam_mt=4))
    d = RF.dictionaries(cfg)
    sids = [pool.open(kind, RF.agent_args(cls, ms, 16000), dicts=d) for _ in pcms]
    got, pos, live, writing_steps = [[] for _ in pcms], [0] * len(pcms), set(range(len(pcms))), 0
    while live:
        segs = {}
        for i in sorted(live):
            chunk = pcms[i][pos[i]:pos[i] + step]
            pos[i] += step
            segs[sids[i]] = SpeechSegment(content=chunk.tolist(), sample_rate=16000, finished=pos[i] >= len(pcms[i]))
        out = pool.step(segs)
        n_w = pool.last_step["writers"]                  # every writer of a step shares ONE continuation: 4 rows each, one device call
        assert pool.last_step["mt_groups"] == ([(0, n_w)] if n_w else [])
        writing_steps += n_w > 0
        for i in sorted(live):
            o, s = out[sids[i]], pool.sessions[sids[i]]
            got[i].append((not o.is_empty, None if o.is_empty else o.content, bool(o.finished),
                           None if s.tgt_subwords is None else list(s.tgt_subwords),
                           None if getattr(s, "unit", None) is None else list(s.unit)))
            if segs[sids[i]].finished:
                live.discard(i)
    assert writing_steps >= 1
    n_writes = n_pad_states = 0
    for i, pcm in enumerate(pcms):
        agent = _agent(kind, hip_model, hip_vocoder, cfg, ms, ["--beam-mt", "4"])
        real = agent.engine.batch_mt_features

        def counted(*a, _real=real, **kw):
            nonlocal n_pad_states
            n_pad_states += 1
            return _real(*a, **kw)
        agent.engine.batch_mt_features = counted
        want = _run_agent(agent, pcm, ms)
        assert [(w, f, t, u) for w, _, f, t, u in got[i]] == [(w, f, t, u) for w, _, f, t, u in want], f"session {i}: text / units"
        for (_, a, _, _, _), (_, b, _, _, _) in zip(got[i], want):
            if a is None or isinstance(a, str):
                assert a == b
                continue
            assert len(a) == len(b)
            if len(a) == 0:                          # the agent's empty final write
                continue
            n_writes += 1
            rms = float(np.sqrt(np.mean((np.asarray(a, np.float32) - np.asarray(b, np.float32)) ** 2)))
            assert rms < BATCH_RMS_TOL, (i, rms)
    assert kind == "s2tt" or n_writes >= len(pcms)
    if ms >= 640:
        assert n_pad_states >= 1, "no whole-word final write with a trailing <pad> was reached"
