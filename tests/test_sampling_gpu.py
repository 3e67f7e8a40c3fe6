"""Sampling from the first-pass text decoder end to end on the synthetic checkpoint (ss_batch_mt_sample / _continue through the
engine, SequenceGenerator, the offline driver, the S2TT agent and the TextSessionPool): 4 utterances, k = 4 chains, max_len_b_mt 10.

What a sample must be whatever the random stream gives: its positional scores are the teacher-forced scores of its own tokens
(batch_mt_score, temperature 1) within 2e-5, the margin tests/test_mt_score_gpu.py allows between the search and the scorer; every
token lies in the kept set recomputed from a teacher-forced pass (its decoder states times the output projection, through
tests/sampling_ref.py; _check_lists says where a band applies); the cumulative score is the sum of the positional ones; the lists are
ordered by score; the same seed and keys give the same bits, alone or in a pack in any order."""
import os
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, MLB, EOS, PAD = 4, 10, 2, 1
KEYS = [11, 12, 13, 2 ** 63 + 5]
SCORE_MARGIN = 2e-5


def _synthetic(n, seed0):
    from streamspeech_amd import synth, workload
    utts = sorted(workload.make_utterances(60), key=lambda u: u.seconds)[:n]
    return [torch.from_numpy(synth.synth_pcm(seed0 + u.idx, u.n_samples)) for u in utts]


def _encode(model, pcms):
    lens = [int(p.numel()) for p in pcms]
    feat, T = model.batch_fbank_cmvn(torch.cat(pcms).cuda(), lens)
    enc, Tp = model.batch_encoder_forward(feat, T)
    return enc, Tp, T


@pytest.fixture(scope="module")
def pack(hip_model):
    enc, Tp, T = _encode(hip_model, _synthetic(4, 1300))
    return enc, Tp, T, np.concatenate([[0], np.cumsum(Tp)])


@pytest.fixture(scope="module")
def eos_model(synth_weights):
    """The eos-scaled model of tests/make_golden_beam.py: </s> is likely early, so chains end at different lengths."""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd.engine import HipModel
    from tests.make_golden_beam import state_dict
    cfg = synth_weights[0]
    g = np.load(os.path.join(ROOT, "tests", "golden", "gcmvn_fr-en.npz"))
    return HipModel(state_dict(3.0, cfg), cfg, cmvn_mean=g["mean"], cmvn_std=g["std"])


def _key(hyps):
    return [(h["tokens"], struct.pack("<f", h["score"]), [struct.pack("<f", p) for p in h["positional_scores"]]) for h in hyps]


PROJ = "target_unigram_decoder.output_projection.weight"
EPS = 2 * SCORE_MARGIN      # two values of one row, each within the margin of its teacher-forced twin


def _check_lists(model, sd, enc, Tp, nbest, prefixes=None, topk=0, topp=0.0, normalize=True, temperature=1.0, ngram=0, max_len=None):
    """The properties every sampled list has.  One teacher-forced pass (batch_mt_score with its decoder states) runs over all samples
    of the pack; the states times the output projection `sd[PROJ]`, in float64, are the logits of every drawn position, and
    sampling_ref.row_values makes the candidate values v of the rule from them (temperature, masks, ban, the row's own step and
    max_len).  Every drawn token t must then lie in sampling_ref.kept_set(v).  The lock-step rows that drew it differ from the
    teacher-forced ones by up to SCORE_MARGIN per value, so a token outside the recomputed set is accepted only inside that band:
      top-k   fewer than K tokens have v > v[t] + EPS (nothing that is certainly ahead of t fills the set);
      top-p   the mass of the tokens with v > v[t] + EPS is < P + tau, tau = V * 2^-23 (the float32 scan, as at op level) + EPS
              (the masses move with the values);
      plain   no band: v[t] > -inf.
    Where no other value lies within EPS of v[t] or of the set's edge, and no prefix mass within tau of P, the band is empty and the
    check is plain membership.  The band is there for rounding, not to carry the check: at most one token in twenty may need it."""
    from tests import sampling_ref as SR
    from tests import search_ref as BR
    B, V = len(Tp), model.cfg.tgt_vocab
    prefixes = prefixes or [[]] * B
    max_len = max_len or [MLB] * B
    W = np.asarray(sd[PROJ], np.float64)
    tau = V * 2.0 ** -23 + EPS
    rows, src = [], []
    for b, hyps in enumerate(nbest):
        assert len(hyps) == K, f"utterance {b}: {len(hyps)} samples"
        sc = [h["score"] for h in hyps]
        assert all(np.isfinite(sc)) and sc == sorted(sc, reverse=True)
        for h in hyps:
            t = h["tokens"]
            assert t[:len(prefixes[b])] == prefixes[b] and t[-1] == EOS and EOS not in t[:-1] and PAD not in t
            assert len(t) <= max_len[b] + 1 and len(h["positional_scores"]) == len(t)
            rows.append(t[:-1])
            src.append(b)
    scored = model.batch_mt_score(enc, Tp, rows, src=src, want_feats=True)
    worst, i, n_tokens, n_band = 0.0, 0, 0, 0
    for b, hyps in enumerate(nbest):
        for h in hyps:
            r = scored[i]
            i += 1
            toks, n0 = h["tokens"], len(prefixes[b])
            pos = np.asarray(h["positional_scores"], np.float64)
            if temperature == 1.0:                                           # the scorer knows no temperature
                ref = r["positional_scores"].double().numpy()
                worst = max(worst, float(np.abs(pos - ref).max()))
                assert np.abs(pos - ref).max() <= SCORE_MARGIN, (b, toks, np.abs(pos - ref).max())
            cum = np.float32(0)
            for p in h["positional_scores"]:                                 # the in-order float32 sum, the prefix included
                cum = np.float32(cum + np.float32(p))
            want = cum / np.float32(len(pos)) if normalize else cum
            assert abs(h["score"] - float(want)) <= 2.0 ** -22 * abs(float(want)) + 1e-7, (h["score"], want)
            logits = r["feats"][:len(toks)].double().cpu().numpy() @ W.T     # row p predicts token p
            for p in range(n0, len(toks)):                                   # the drawn positions; reference step p
                banned = BR.banned_tokens([EOS] + toks[:p], ngram) if ngram else ()
                v = SR.row_values(logits[p], temperature, PAD, model.cfg.unk, EOS, 0.0, p, 1, max_len[b], banned)
                t = toks[p]
                assert abs(v[t] - pos[p]) <= SCORE_MARGIN, (b, toks, p, v[t], pos[p])   # the recomputed row is the row that was drawn from
                kept, _ = SR.kept_set(v, topk, topp)
                n_tokens += 1
                if p >= max_len[b]:
                    assert kept == [EOS] and t == EOS                        # a row at max_len keeps </s> alone
                if t in kept:
                    continue
                ahead = v > v[t] + EPS
                assert (topk or topp) and v[t] > -np.inf, (b, toks, p, "not in the kept set")
                if topk:
                    assert int(ahead.sum()) < topk, (b, toks, p, int(ahead.sum()))
                else:
                    assert float(np.exp(v[ahead]).sum()) < topp + tau, (b, toks, p, float(np.exp(v[ahead]).sum()))
                n_band += 1
    assert 20 * n_band <= n_tokens, f"{n_band} of {n_tokens} tokens were admitted by the band alone"
    return worst


@pytest.mark.parametrize("kw", [dict(), dict(topk=5), dict(topp=0.9), dict(topp=0.3)], ids=["plain", "topk5", "topp0.9", "topp0.3"])
def test_samples_are_scored_as_the_scorer_scores_them(hip_model, synth_weights, pack, kw):
    enc, Tp, _, _ = pack
    nbest, feats, n = hip_model.batch_mt_sample(enc, Tp, [MLB] * 4, K, KEYS, seed=3, **kw)
    worst = _check_lists(hip_model, synth_weights[2], enc, Tp, nbest, **kw)
    assert n == [len(h[0]["tokens"]) for h in nbest] and feats.shape[0] == 4
    print(f"sampling {kw}: worst |sample - scorer| positional score {worst:.3g}; lengths {[[len(h['tokens']) for h in hy] for hy in nbest]}")


def test_same_seed_same_lists_another_seed_other_lists(hip_model, pack):
    enc, Tp, _, _ = pack
    a, fa, na = hip_model.batch_mt_sample(enc, Tp, [MLB] * 4, K, KEYS, seed=3, topk=10)
    b, fb, nb = hip_model.batch_mt_sample(enc, Tp, [MLB] * 4, K, KEYS, seed=3, topk=10)
    assert [_key(h) for h in a] == [_key(h) for h in b] and na == nb
    assert all(torch.equal(fa[i, :na[i]], fb[i, :nb[i]]) for i in range(4))
    c, _, _ = hip_model.batch_mt_sample(enc, Tp, [MLB] * 4, K, KEYS, seed=4, topk=10)
    assert any(_key(x) != _key(y) for x, y in zip(a, c))
    d, _, _ = hip_model.batch_mt_sample(enc, Tp, [MLB] * 4, K, [k + 100 for k in KEYS], seed=3, topk=10)
    assert any(_key(x) != _key(y) for x, y in zip(a, d))                    # another key is another stream


def test_alone_and_in_a_pack_in_any_order(hip_model, synth_weights, pack):
    enc, Tp, _, off = pack
    kw = dict(seed=9, topp=0.9, temperature=1.7, no_repeat_ngram_size=3)
    whole, wf, wn = hip_model.batch_mt_sample(enc, Tp, [MLB, MLB - 1, MLB, MLB - 2], K, KEYS, **kw)
    _check_lists(hip_model, synth_weights[2], enc, Tp, whole, topp=0.9, temperature=1.7, ngram=3, max_len=[MLB, MLB - 1, MLB, MLB - 2])
    for b in range(4):
        alone, af, an = hip_model.batch_mt_sample(enc[off[b]:off[b + 1]], [Tp[b]], [[MLB, MLB - 1, MLB, MLB - 2][b]], K, [KEYS[b]], **kw)
        assert _key(alone[0]) == _key(whole[b]), f"utterance {b}: alone vs in the pack"
        assert an[0] == wn[b] and torch.equal(af[0, :an[0]], wf[b, :wn[b]])
    order = [2, 0, 3, 1]
    enc_p = torch.cat([enc[off[b]:off[b + 1]] for b in order])
    perm, _, _ = hip_model.batch_mt_sample(enc_p, [Tp[b] for b in order], [[MLB, MLB - 1, MLB, MLB - 2][b] for b in order], K,
                                           [KEYS[b] for b in order], **kw)
    for i, b in enumerate(order):
        assert _key(perm[i]) == _key(whole[b]), f"utterance {b}: permuted pack"


def test_topk_1_is_the_greedy_search(hip_model, pack):
    enc, Tp, _, _ = pack
    greedy, gf, gn = hip_model.batch_mt_greedy(enc, Tp, [MLB] * 4)
    nbest, feats, n = hip_model.batch_mt_sample(enc, Tp, [MLB] * 4, K, KEYS, seed=5, topk=1)
    for b in range(4):
        assert all(h["tokens"] == list(greedy[b]) for h in nbest[b]), (b, greedy[b], [h["tokens"] for h in nbest[b]])
        assert len({struct.pack("<f", h["score"]) for h in nbest[b]}) == 1   # k equal chains, bit for bit
        assert n[b] == gn[b] and torch.equal(feats[b, :n[b]], gf[b, :gn[b]])


def test_max_len_forces_eos(hip_model, pack):
    enc, Tp, _, _ = pack
    mx = [1, 2, 3, 4]
    nbest, _, _ = hip_model.batch_mt_sample(enc, Tp, mx, K, KEYS, seed=1)
    for b, hyps in enumerate(nbest):
        assert len(hyps) == K
        for h in hyps:
            assert h["tokens"][-1] == EOS and len(h["tokens"]) <= mx[b] + 1 and np.isfinite(h["score"])
        assert any(len(h["tokens"]) == mx[b] + 1 for h in hyps)              # min_len 1 and the synthetic model: the limit is reached


def test_chains_of_one_utterance_differ(eos_model, synth_weights, pack):
    from tests.make_golden_beam import state_dict
    pcms = _synthetic(4, 1300)
    enc, Tp, _ = _encode(eos_model, pcms)
    nbest, _, _ = eos_model.batch_mt_sample(enc, Tp, [MLB] * 4, K, KEYS, seed=2)
    _check_lists(eos_model, state_dict(3.0, synth_weights[0]), enc, Tp, nbest)
    for b, hyps in enumerate(nbest):
        print(f"utterance {b}: {[h['tokens'] for h in hyps]}")
        assert len({tuple(h["tokens"]) for h in hyps}) == K, (b, [h["tokens"] for h in hyps])


def test_forced_prefix_is_kept_and_counted(hip_model, synth_weights, pack):
    enc, Tp, _, off = pack
    prefixes = [[], [9, 4], [11], [9, 4, 17]]
    for k in (K, 1):
        nbest, feats = hip_model.batch_mt_sample_continue(enc, Tp, prefixes, [MLB] * 4, k, KEYS, seed=6, topk=8)
        if k == K:
            _check_lists(hip_model, synth_weights[2], enc, Tp, nbest, prefixes=prefixes, topk=8)
        for b, hyps in enumerate(nbest):
            assert len(hyps) == k and feats[b].shape[0] == len(hyps[0]["tokens"])
            for h in hyps:
                assert h["tokens"][:len(prefixes[b])] == prefixes[b]
                assert h["score"] == pytest.approx(sum(h["positional_scores"]) / len(h["tokens"]), rel=1e-5)
        # the prefix' own scores are those of the beam search behind the same prefix
        beam, _ = hip_model.batch_mt_beam_continue(enc, Tp, prefixes, [MLB] * 4, k)
        for b in range(4):
            n0 = len(prefixes[b])
            assert _key(nbest[b])[0][2][:n0] == _key(beam[b])[0][2][:n0]
    # no prefix anywhere through the continue entry: the samples of batch_mt_sample
    a, _ = hip_model.batch_mt_sample_continue(enc, Tp, [[]] * 4, [MLB] * 4, K, KEYS, seed=6, topk=8)
    b_, _, _ = hip_model.batch_mt_sample(enc, Tp, [MLB] * 4, K, KEYS, seed=6, topk=8)
    assert [_key(h) for h in a] == [_key(h) for h in b_]


def test_refusals_through_the_engine(hip_model, pack):
    from streamspeech_amd import lib as L
    enc, Tp, _, _ = pack
    for bad in (dict(topk=-1), dict(topp=1.5), dict(topk=3, topp=0.5), dict(topk=hip_model.cfg.tgt_vocab + 1)):
        with pytest.raises(ValueError):
            hip_model.batch_mt_sample(enc, Tp, [MLB] * 4, K, KEYS, **bad)
    with pytest.raises(ValueError):
        hip_model.batch_mt_sample(enc, Tp, [MLB] * 4, K, KEYS[:3])
    with pytest.raises(L.StreamSpeechHipError) as e:                         # the library's own refusal of a repeated prefix stays
        hip_model.batch_mt_sample_continue(enc[:Tp[0]], Tp[:1], [[7, 8, 7, 8]], [MLB], K, KEYS[:1], no_repeat_ngram_size=2)
    assert e.value.code == L.SS_ERR_ARG


def test_generator_and_offline_driver(hip_model, pack, tmp_path):
    from oracle.ref_agent import make_dicts
    from streamspeech_amd import offline
    from streamspeech_amd.generators import SequenceGenerator
    enc, Tp, T, off = pack
    dicts = make_dicts(hip_model.cfg)
    want, _, _ = hip_model.batch_mt_sample(enc, Tp, [MLB] * 4, K, [300, 301, 302, 303], seed=7, topk=10)
    gen = SequenceGenerator(hip_model, dicts["target_unigram"], beam_size=K, max_len_a=0, max_len_b=MLB, sampling=True, sampling_topk=10,
                            seed=7)
    for b in range(4):
        out = gen.generate_decoder([{"encoder_out": [enc[off[b]:off[b + 1]].unsqueeze(1)]}], torch.zeros(1, T[b], 80), None,
                                   sample={"id": torch.tensor([300 + b])})[0]
        assert [h["tokens"].tolist() for h in out] == [h["tokens"] for h in want[b]]
        assert [struct.pack("<f", h["score"]) for h in out] == [struct.pack("<f", h["score"]) for h in want[b]]
    items = [(300 + i, p.cuda()) for i, p in enumerate(_synthetic(4, 1300))]
    hyp = offline.generate(hip_model, None, items, dicts, str(tmp_path), "test", max_len_b_mt=MLB, dump_wav=False, beam_mt=K,
                           sampling=True, sampling_topk=10, seed=7)
    lines = [ln.rstrip("\n").split("\t") for ln in open(tmp_path / "generate-test.mt.samples", encoding="utf-8")]
    assert len(lines) == 4 * K
    for b in range(4):
        mine = [ln for ln in lines if int(ln[0]) == 300 + b]
        assert [int(ln[1]) for ln in mine] == list(range(K))
        texts = [offline.detok([dicts["target_unigram"][t] for t in h["tokens"] if t != EOS]) for h in want[b]]
        assert [ln[3] for ln in mine] == texts
        assert [float(ln[2]) for ln in mine] == pytest.approx([h["score"] for h in want[b]], abs=1e-6)
        assert hyp[300 + b]["mt"] == texts[0]                                # the best-scoring sample is the D- text
    assert not os.path.exists(tmp_path / "generate-test.mt.words")


# ---- the streaming surfaces --------------------------------------------------------------------------------------------------------
def _s2tt_agent(hip_model, cfg, flags, ms=320):
    from streamspeech_amd.agent_text import StreamSpeechS2TTAgent
    from streamspeech_amd.modules import StreamSpeechModel
    from tests import ref_fixtures as RF
    model = StreamSpeechModel.from_engine(hip_model.new_context())
    return RF.set_dicts(StreamSpeechS2TTAgent(RF.agent_args(StreamSpeechS2TTAgent, ms, 16000, extra=flags), model=model), cfg)


def _run_agent(agent, pcm, ms=320):
    from streamspeech_amd.simuleval_shim import SpeechSegment
    step, pos, recs = 16 * ms, 0, []
    while True:
        chunk = pcm[pos:pos + step]
        pos += step
        fin = pos >= len(pcm)
        o = agent.pushpop(SpeechSegment(content=chunk.tolist(), sample_rate=16000, finished=fin))
        t = agent.tgt_subwords_indices
        recs.append((not o.is_empty, None if o.is_empty else o.content, bool(o.finished),
                     None if t is None else [int(x) for x in t.view(-1).tolist()]))
        if fin:
            return recs


def _run_pool(pool, pcms, cfg):
    from streamspeech_amd.agent_text import StreamSpeechS2TTAgent
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from tests import ref_fixtures as RF
    d = RF.dictionaries(cfg)
    sids = [pool.open("s2tt", RF.agent_args(StreamSpeechS2TTAgent, 320, 16000), dicts=d) for _ in pcms]
    got, pos, live = [[] for _ in pcms], [0] * len(pcms), set(range(len(pcms)))
    while live:
        segs = {}
        for i in sorted(live):
            chunk = pcms[i][pos[i]:pos[i] + 5120]
            pos[i] += 5120
            segs[sids[i]] = SpeechSegment(content=chunk.tolist(), sample_rate=16000, finished=pos[i] >= len(pcms[i]))
        out = pool.step(segs)
        for i in sorted(live):
            o, s = out[sids[i]], pool.sessions[sids[i]]
            got[i].append((not o.is_empty, None if o.is_empty else o.content, bool(o.finished),
                           None if s.tgt_subwords is None else list(s.tgt_subwords)))
            if segs[sids[i]].finished:
                live.discard(i)
    return sids, got


def test_s2tt_agent_and_text_pool_replay_identically(hip_model, synth_weights):
    """--sampling at the agent and search=SamplingOptions at the pool: a replayed session commits the same text, another seed another
    one, two sessions of a pool sample from different streams, and the pool's session with id s is the agent with --sampling-session
    s."""
    from streamspeech_amd import synth
    from streamspeech_amd.engine import SamplingOptions
    from streamspeech_amd.text_pool import TextSessionPool
    cfg = synth_weights[0]
    pcm = synth.synth_pcm(4100, int(16000 * 2.4))
    flags = ["--sampling", "--sampling-topk", "20", "--seed", "5", "--beam-mt", "2"]
    agent = _s2tt_agent(hip_model, cfg, flags)
    assert agent.generator_mt.sampling is not None and agent.generator_mt.sampling.kwargs() == {"topk": 20, "topp": 0.0, "seed": 5}
    a = _run_agent(agent, pcm)
    b = _run_agent(_s2tt_agent(hip_model, cfg, flags), pcm)
    assert a == b and sum(1 for r in a if r[0]) >= 2                         # several writes, the same each time
    agent.reset()
    assert _run_agent(agent, pcm) == a                                       # reset() starts the stream again
    other = _run_agent(_s2tt_agent(hip_model, cfg, flags[:4] + ["6"] + flags[5:]), pcm)
    plain = _run_agent(_s2tt_agent(hip_model, cfg, []), pcm)
    final = lambda recs: next(t for _, _, _, t in reversed(recs) if t is not None)   # noqa: E731
    assert final(other) != final(a) and final(plain) != final(a)
    opts = SamplingOptions(topk=20, seed=5)
    sids, got = _run_pool(TextSessionPool(hip_model, 4, 256, beam_mt=2, search=opts), [pcm, pcm], cfg)
    sids2, again = _run_pool(TextSessionPool(hip_model, 4, 256, beam_mt=2, search=opts), [pcm, pcm], cfg)
    assert sids == sids2 and got == again
    assert final(got[0]) != final(got[1])                                    # the same audio in two sessions: two streams
    for sid, recs in zip(sids, got):
        assert recs == _run_agent(_s2tt_agent(hip_model, cfg, flags + ["--sampling-session", str(sid)]), pcm)
