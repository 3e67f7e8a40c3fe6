"""Keyword spotting on the CTC heads on the GPU (csrc/ctc_spot.hip).  The oracle of the kernels is the host twin, which
tests/test_ctc_spot_cpu.py pins to the two float64 references, and every comparison is memcmp of the records: the per-frame cost
is one float32 subtraction from the row maximum and the recursion is float64 additions in frame order, so device and twin agree
bit for bit.  First ss_op_ctc_spot and ss_op_ctc_spot_stream_advance on the CPU test's cases, extended to the DP kernel's LDS
staging depth (16 frames) minus one, exact and plus one and to one keyword more than a workgroup owns; then the seeded synthetic
checkpoint: ss_batch_ctc_spot alone, in a pack and in the reversed pack, a planted hit, the resumable object on chosen splits, the
session pool, the ASR agent and the offline driver."""
import numpy as np
import pytest
import torch

from tests import ctc_spot_ref as R
from tests.test_ctc_spot_cpu import (CASES, PAD, UNK, case_logits, check_bad_rows, check_call_refusals, check_overflow, check_pack,
                                     check_splits, check_stream_rules, constructed, keyword_set, quarter_logits, random_logits, spans,
                                     stream_case)

pytestmark = pytest.mark.gpu
STAGE = 16                                                    # CTC_SPOT_STAGE of csrc/ctc_spot.hpp


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import lib as L
    return L.load()


def against_the_twin(lib, x, phrases, taus, V, max_hits=4096):
    with R.KeywordSet(lib, phrases, taus, V, PAD, UNK) as ks:
        assert ks.rc == 0
        rc0, h0, c0 = R.run(lib, ks, [x], max_hits)
        rc1, h1, c1 = R.run(lib, ks, [x], max_hits, gpu=True)
    assert rc0 == 0 and rc1 == 0 and c0["overflow"][0] == 0
    assert c1.tobytes() == c0.tobytes()
    assert R.written(h1, c1).tobytes() == R.written(h0, c0).tobytes()
    return R.written(h1, c1)


# ---- the kernels on the caller's logits ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,V,T,kind", CASES + [("five", 37, STAGE - 1, "q"), ("five", 37, STAGE, "q"), ("five", 37, STAGE + 1, "r"),
                                                   ("300", 37, 2 * STAGE + 1, "r"), ("257x1", 37, STAGE + 1, "q")])
def test_op_against_the_host_twin(lib, name, V, T, kind):
    phrases, taus = keyword_set(name, V)
    got = against_the_twin(lib, case_logits(name, V, T, kind), phrases, taus, V)
    if name == "257x1":
        assert (got["keyword"] == 256).any() and (got["keyword"] < 256).any()    # both workgroups report


@pytest.mark.parametrize("name", sorted(constructed()[1]))
def test_op_constructed_logits(lib, name):
    V, cases = constructed()
    x, phrases, taus, want = cases[name]
    assert spans(against_the_twin(lib, x, phrases, taus, V)) == want


def test_op_pack_bad_rows_overflow_and_refusals(lib):
    check_pack(lib, gpu=True)
    check_bad_rows(lib, gpu=True)
    check_overflow(lib, gpu=True)
    check_call_refusals(lib, gpu=True)


def test_op_stream_splits_and_rules(lib):
    """The resumable kernels: the 12-frame case on single cuts, one frame per call and all at once; a 40-frame utterance with 300
    keywords cut around the staging depth; the slot rules."""
    V, phrases, taus, x = stream_case()
    cuts = [()] + [(c,) for c in range(1, 12)] + [tuple(range(1, 12)), (3, 3, 7), (5, 6)]
    check_splits(lib, V, phrases, taus, x, cuts, gpu=True)
    V = 37
    phrases, taus = keyword_set("300", V)
    x = random_logits(77, 40, V)
    with R.KeywordSet(lib, phrases, taus, V, PAD, UNK) as ks:
        rc, hits, counts = R.run(lib, ks, [x], 4096)
        want = R.written(hits, counts)
        assert rc == 0 and len(want) > 10
        with R.Stream(lib, ks, 1, gpu=True) as st:
            for cuts in ((STAGE - 1,), (STAGE,), (STAGE + 1, 2 * STAGE + 1), (1, 2, 39)):
                got, _ = R.stream_utterance(st, x, cuts, max_hits=4096)
                assert got.tobytes() == want.tobytes(), cuts
    check_stream_rules(lib, gpu=True)


def test_op_large_vocabulary_many_keywords(lib):
    """V = 6004, 1000 keywords of 1 .. 8 labels over the whole vocabulary (U in the hundreds, several workgroups), T = 33."""
    V, T = 6004, 2 * STAGE + 1
    rng = np.random.default_rng(9)
    phrases = [[int(v) for v in rng.integers(4, V, int(rng.integers(1, 9)))] for _ in range(1000)]
    x = random_logits(3, T, V, 1.0)
    got = against_the_twin(lib, x, phrases, [8.0] * 1000, V, max_hits=16384)
    assert len(got) > 0


# ---- the model -------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model(hip_model):
    return hip_model


@pytest.fixture(scope="module")
def pack(model):
    """Five utterances through the encoder: (packed rows, Tp, the scored greedy records of head 0 with raw, its logits)."""
    from streamspeech_amd import synth
    T = (97, 260, 533, 41, 180)
    fb = torch.cat([torch.from_numpy(synth.synth_fbank(300 + k, t)) for k, t in enumerate(T)]).to(model.device)
    enc, Tp = model.batch_encoder_forward(fb.contiguous(), list(T))
    greedy = model.batch_ctc_greedy(0, enc, Tp, return_raw=True, return_scores=True)
    logits = model.last_logits().cpu().numpy().copy()
    return enc, Tp, greedy, logits


def planted(pack_, V):
    """Per utterance three consecutive tokens of the greedy transcript whose frames' UNMASKED arg-max is the greedy path's (the
    greedy search masks pad and unk, the spotter does not) -> [(utterance, tokens, first frame, last frame)]."""
    enc, Tp, greedy, logits = pack_
    out, r0 = [], 0
    for b, (toks, first, last, _, _, raw) in enumerate(greedy):
        am = logits[r0:r0 + Tp[b], :V].argmax(axis=1)
        for i in range(len(toks) - 2):
            a, z = first[i], last[i + 2]
            if PAD not in toks[i:i + 3] and (am[a:z + 1] == np.asarray(raw[a:z + 1])).all():
                out.append((b, toks[i:i + 3], a, z))
                break
        r0 += Tp[b]
    return out


def model_keywords(model, pack_):
    """The planted triples at tau = 0 (only a path that IS the arg-max path is a candidate), then bigrams and single tokens of the
    transcripts at the default threshold."""
    from streamspeech_amd.keywords import CtcKeywords
    V = model.cfg.src_vocab
    plants = planted(pack_, V)
    assert plants
    phrases, taus = [p[1] for p in plants], [0.0] * len(plants)
    for toks, *_ in pack_[2]:
        for i in range(0, max(len(toks) - 1, 0), 3):
            if model.cfg.pad not in toks[i:i + 2]:
                phrases.append(toks[i:i + 2])
                taus.append(1.0)
    return CtcKeywords(phrases, taus, V, model.cfg.pad, model.cfg.unk), plants


def test_batch_alone_in_a_pack_and_reversed_and_the_planted_hit(model, pack):
    from streamspeech_amd import lib as L
    enc, Tp, greedy, logits = pack
    kw, plants = model_keywords(model, pack)
    with kw:
        hits, counts = model.batch_ctc_spot(0, enc, Tp, kw, 512, return_counts=True)
        assert (counts["status"] == 0).all() and (counts["overflow"] == 0).all() and counts["frames"].tolist() == Tp
        assert [len(h) for h in hits] == counts["n_hits"].tolist()
        off = np.cumsum([0] + Tp)
        views = [enc[off[b]:off[b + 1]] for b in range(len(Tp))]
        for b, v in enumerate(views):
            assert model.ctc_spot(0, v, kw, 512) == hits[b], b
        rev = model.batch_ctc_spot(0, torch.cat(views[::-1]).contiguous(), Tp[::-1], kw, 512)
        assert rev[::-1] == hits
        # the host twin on the head's own logits: the same records
        h0, c0 = kw.spot_host(logits[:, :model.cfg.src_vocab], Tp, 512)
        from streamspeech_amd.keywords import hits_from_records
        assert [hits_from_records(h0[b, :c0["n_hits"][b]]) for b in range(len(Tp))] == hits
        for k, (b, toks, a, z) in enumerate(plants):
            mine = [h for h in hits[b] if h.keyword == k and h.start == a]
            assert mine and mine[0].end == z and mine[0].score == 0.0 and mine[0].norm == 0.0, (k, b, a, z, hits[b])
        print(f"ctc_spot model: {kw.n_keywords} keywords, {sum(len(h) for h in hits)} hits over {sum(Tp)} rows, {len(plants)} planted")
        # refusals: nothing launched, the context as usable as before
        for bad in (dict(max_hits=0), dict(max_hits=16385), dict(Tp=[Tp[0] + 1500] + Tp[1:]), dict(Tp=[0] + Tp[1:])):
            a = dict(head=0, Tp=Tp, max_hits=512)
            a.update(bad)
            with pytest.raises(L.StreamSpeechHipError) as e:
                model.batch_ctc_spot(a["head"], enc, a["Tp"], kw, a["max_hits"])
            assert e.value.code == L.SS_ERR_ARG
        with pytest.raises(L.StreamSpeechHipError):
            model.batch_ctc_spot(2, enc, Tp, kw, 512)
        from streamspeech_amd.keywords import CtcKeywords
        for other in (CtcKeywords([[5]], 1.0, model.cfg.src_vocab + 1, model.cfg.pad, model.cfg.unk),
                      CtcKeywords([[5]], 1.0, model.cfg.src_vocab, -1, model.cfg.unk)):       # not this head's V / pad
            with other, pytest.raises(L.StreamSpeechHipError) as e:
                model.batch_ctc_spot(0, enc, Tp, other, 512)
            assert e.value.code == L.SS_ERR_ARG
        assert model.batch_ctc_spot(0, enc, Tp, kw, 512) == hits


def test_stream_object_on_splits_of_a_hit(model, pack):
    """engine.CtcSpotStream on the rows of utterance 1: all at once, one frame per call, a cut inside the planted hit, a cut on the
    frame after its end, and two sessions in one call; the scratch booking is the header's formula."""
    from streamspeech_amd.engine import CtcSpotStream
    enc, Tp, greedy, logits = pack
    kw, plants = model_keywords(model, pack)
    with kw:
        off = np.cumsum([0] + Tp)
        b, _, a, z = [p for p in plants if p[0] in (1, 2, 4)][0]
        rows = enc[off[b]:off[b + 1]].contiguous()
        T = Tp[b]
        want = model.ctc_spot(0, rows, kw, 512)
        # the state: one piece of the header's size on the context's scratch set, refused on the cap, released by close()
        from streamspeech_amd import lib as L
        from streamspeech_amd.engine import Scratch
        sc = Scratch(model.device)
        ctx = model.new_context(sc)
        assert ctx.ctc_spot(0, rows, kw, 512) == want
        start, need = sc.bytes(), (3 * (12 * kw.states + 20 * kw.n_keywords + 4) + 7) // 8 * 8
        sc.set_cap(start + need - 1)
        with pytest.raises(L.StreamSpeechHipError) as e:
            CtcSpotStream(ctx, 0, 3, kw)
        assert e.value.code == L.SS_ERR_SCRATCH_CAP and sc.bytes() == start and sc.audit()[0] == sc.audit()[1]
        sc.set_cap(start + need)
        with CtcSpotStream(ctx, 0, 3, kw) as st3:
            assert sc.bytes() == start + need and sc.audit()[0] == sc.audit()[1]
            sc.set_cap(0)
            for bad in (dict(upto=[T + 1]), dict(T=[T - 1]), dict(slots=[3]), dict(max_hits=0)):
                a_ = dict(slots=[2], T=[T], upto=[T], max_hits=8)
                a_.update(bad)
                with pytest.raises(L.StreamSpeechHipError) as e:
                    st3.advance(a_["slots"], rows, a_["T"], a_["upto"], [True], a_["max_hits"])
                assert e.value.code == L.SS_ERR_ARG
            st3.model = model                                   # a model on another scratch set than the object's
            with pytest.raises(L.StreamSpeechHipError):
                st3.advance([2], rows, [T], [T], [True])
            st3.model = ctx
            assert st3.advance([2], rows, [T], [T], [True], 512)[0].hits == want
            held = sc.bytes()
        assert sc.bytes() == held - need
        for bad in (dict(head=2), dict(max_sessions=0), dict(head=1)):      # (head 1: the set is the source head's)
            a_ = dict(head=0, max_sessions=1)
            a_.update(bad)
            if a_["head"] == 1 and model.cfg.src_vocab == model.cfg.tgt_vocab:
                continue
            with pytest.raises(L.StreamSpeechHipError) as e:
                CtcSpotStream(ctx, a_["head"], a_["max_sessions"], kw)
            assert e.value.code == L.SS_ERR_ARG
        with CtcSpotStream(model, 0, 2, kw) as st:
            for cuts in ([], list(range(1, T)), [a + 1], [z + 1], [a, z, z + 1, z + 2]):
                got, f = [], 0
                for t in [c for c in cuts if 0 < c < T] + [T]:
                    part = st.advance([1], rows[:t].contiguous(), [t], [t], [t == T], 512)[0]
                    assert part.frames == t and part.status == 0 and part.final == (t == T) and part.n_hits == len(part.hits)
                    got += part.hits
                    f = t
                assert sorted(got, key=lambda h: (h.end, h.keyword, h.start)) == want, cuts
            b2 = 3
            rows2 = enc[off[b2]:off[b2 + 1]].contiguous()
            both = torch.cat([rows[:T // 2], rows2]).contiguous()
            p0, p1 = st.advance([0, 1], both, [T // 2, Tp[b2]], [T // 2, Tp[b2]], [False, True], 512)
            assert p1.hits == model.ctc_spot(0, rows2, kw, 512)
            p2 = st.advance([0], rows, [T], [T], [True], 512)[0]
            assert sorted(p0.hits + p2.hits, key=lambda h: (h.end, h.keyword, h.start)) == want


def test_pool_agent_and_driver(model, synth_weights, tmp_path):
    """TextSessionPool(spot=...): per ASR session the hits of all steps are batch_ctc_spot's on the rows its last advance saw, in
    ms; every segment of every session equals a pool without spot (greedy, and with ctc_beam).  The ASR agent with --ctc-keywords
    reports the pool session's hits.  The driver writes the .hits files and nothing else changes."""
    from streamspeech_amd import offline
    from streamspeech_amd.agent_text import StreamSpeechASRAgent
    from streamspeech_amd.keywords import CtcKeywords, KeywordHit
    from streamspeech_amd.modules import Dictionary, StreamSpeechModel
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.text_policy import CtcBeamOptions
    from streamspeech_amd.text_pool import TextSessionPool
    from streamspeech_amd.words import FRAME_MS
    from tests import ref_fixtures as RF
    from tests.test_ctc_stream_gpu import _pool_plan
    from tests.test_text_pool_gpu import _drive
    cfg = synth_weights[0]
    plan = {k: v for k, v in _pool_plan().items() if k in ("asr0", "asr1", "s2tt2")}
    base = TextSessionPool(model, 8, 256)
    want_segs = _drive(base, plan, cfg)
    d = RF.dictionaries(cfg)
    # keywords from what the sessions say: bigrams of their transcripts
    phrases = []
    for name in ("asr0", "asr1"):
        text = "".join(c or "" for _, c, _ in want_segs[name]).split(" ")
        ids = [d["source_unigram"].index(w) for w in text if w]
        phrases += [ids[i:i + 2] for i in range(0, len(ids) - 1, 2) if not {cfg.pad, cfg.unk, 0} & set(ids[i:i + 2])]
    assert phrases
    phrases = [p for i, p in enumerate(phrases) if p not in phrases[:i]]
    with CtcKeywords(phrases, 1.0, model.cfg.src_vocab, model.cfg.pad, model.cfg.unk) as kw:
        for extra in ({}, {"ctc_beam": CtcBeamOptions(4)}, {"details": True}):
            ref_pool = base if not extra else TextSessionPool(model, 8, 256, **extra)
            ref_segs = want_segs if not extra else _drive(ref_pool, plan, cfg)
            pool = TextSessionPool(model, 8, 256, spot=kw, **extra)
            finals, advance = {}, pool.spot_stream.advance

            def spy(slots, enc_packed, T, upto, final, max_hits):
                got = advance(slots, enc_packed, T, upto, final, max_hits)
                sid_of = {s.slot: sid for sid, s in pool.sessions.items() if s.slot is not None}
                off = 0
                for sl, t, fin in zip(slots, T, final):
                    if fin:
                        finals[sid_of[sl]] = model.batch_ctc_spot(0, enc_packed[off:off + t].contiguous(), [t], kw, 512)[0]
                    off += t
                return got

            pool.spot_stream.advance = spy
            got_segs = _drive(pool, plan, cfg)
            assert got_segs == ref_segs, extra
            assert ref_pool.hits(0) is None
            total = 0
            for sid, name in enumerate(plan):
                got = pool.hits(sid)
                if name.startswith("s2tt"):
                    assert got == [] and sid not in finals
                    continue
                want = [KeywordHit(h.keyword, kw.texts[h.keyword], h.start * FRAME_MS, (h.end + 1) * FRAME_MS, h.score, h.norm)
                        for h in finals[sid]]
                assert sorted(got, key=lambda h: (h.end_ms, h.keyword, h.start_ms)) == want, (name, extra)
                assert pool.hits(sid) == []
                total += len(got)
            assert total > 0
            assert pool.last_step["ctc_spot_lost"] == 0 and "ctc_spot_calls" not in ref_pool.last_step
            pool.spot_stream.close()
            if extra.get("ctc_beam"):
                pool.ctc_stream.close()
                ref_pool.ctc_stream.close()
            pool_hits = {name: finals[sid] for sid, name in enumerate(plan) if sid in finals}
    # ---- the agent: the same set, read from a file over the agent's own dictionary ----
    ph = Dictionary.placeholder(model.cfg.src_vocab)
    kwf = tmp_path / "kw.txt"
    kwf.write_text("".join(" ".join(ph[c] for c in p) + "\n" for p in phrases), encoding="utf-8")
    kind, _, pcm, sr, ms, _ = plan["asr1"]
    args = RF.agent_args(StreamSpeechASRAgent, ms, sr, extra=("--ctc-keywords", str(kwf)))
    agent = RF.set_dicts(StreamSpeechASRAgent(args, model=StreamSpeechModel.from_engine(model)), cfg)
    plain = RF.set_dicts(StreamSpeechASRAgent(RF.agent_args(StreamSpeechASRAgent, ms, sr), model=StreamSpeechModel.from_engine(model)), cfg)
    try:
        assert plain.hits is None and plain.spot_stream is None and agent.keywords.n_keywords == len(phrases)
        seen, adv = {}, agent.spot_stream.advance

        def spy_agent(slots, rows, T, upto, final, max_hits=64):    # (the agent's own encoder rows: its own oracle)
            if final[0]:
                seen["want"] = model.batch_ctc_spot(0, rows.contiguous(), T, agent.keywords, 512)[0]
            return adv(slots, rows, T, upto, final, max_hits)

        agent.spot_stream.advance = spy_agent
        texts = []
        for ag in (agent, plain):
            step, pos, text = sr * ms // 1000, 0, ""
            while True:
                chunk = pcm[pos:pos + step]
                pos += step
                fin = pos >= len(pcm)
                o = ag.pushpop(SpeechSegment(content=chunk.tolist(), sample_rate=sr, finished=fin))
                text += "" if o.is_empty else o.content
                if fin:
                    break
            texts.append(text)
        assert texts[0] == texts[1] and texts[0]
        got = sorted(agent.hits, key=lambda h: (h.end_ms, h.keyword, h.start_ms))
        assert [(h.keyword, h.start_ms, h.end_ms, h.score) for h in got] == \
            [(h.keyword, h.start * FRAME_MS, (h.end + 1) * FRAME_MS, h.score) for h in seen["want"]]
        assert [(h.keyword, h.start_ms, h.end_ms) for h in got] == \
            [(h.keyword, h.start * FRAME_MS, (h.end + 1) * FRAME_MS) for h in pool_hits["asr1"]]      # the pool session: the same spans
    finally:
        agent.spot_stream.close()
        agent.keywords.close()
        model.encoder_stream_set_tail(0)
    # ---- the driver ----
    common = ["--path", "synthetic:0", "--vocoder", "synthetic:0", "--synthetic", "3", "--no-wav", "--max-len-b-mt", "6"]
    offline.main(common + ["--results-path", str(tmp_path / "plain")])
    kwa, kws = tmp_path / "kwa.txt", tmp_path / "kws.txt"
    kwa.write_text("".join(f"{ph[c]}\n" for c in range(4, 44)) + f"{ph[50]} {ph[51]}\t3.5\n", encoding="utf-8")
    pt = Dictionary.placeholder(model.cfg.tgt_vocab)
    kws.write_text("".join(f"{pt[c]}\n" for c in range(4, 44)), encoding="utf-8")
    offline.main(common + ["--results-path", str(tmp_path / "kw"), "--ctc-keywords-asr", str(kwa), "--ctc-keywords-st", str(kws),
                           "--ctc-keyword-threshold", "6.0"])
    a = sorted(p.name for p in (tmp_path / "plain").iterdir())
    b = sorted(p.name for p in (tmp_path / "kw").iterdir())
    assert sorted(set(b) - set(a)) == ["generate-test.asr.hits", "generate-test.st.hits"]
    for name in a:
        if (tmp_path / "plain" / name).is_file():
            assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "kw" / name).read_bytes(), name
    n = 0
    for key in ("asr", "st"):
        for ln in (tmp_path / "kw" / f"generate-test.{key}.hits").read_text(encoding="utf-8").splitlines():
            sid, phrase, s_ms, e_ms, score, norm = ln.split("\t")
            assert int(s_ms) % FRAME_MS == 0 and int(e_ms) > int(s_ms) and float(score) <= 0.0 and -6.0 <= float(norm) <= 0.0
            assert abs(float(score) - float(norm) * len(phrase.split())) < 1e-4
            n += 1
    assert n > 0
