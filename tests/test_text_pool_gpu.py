"""Concurrent ASR / S2TT sessions over the session pool (streamspeech_amd/text_pool.py) and the ragged continuation of the text search
(ss_batch_mt_continue), on the GPU: reference traces served concurrently, agreement with the single-session agents, the continuation
against ss_mt_greedy row by row, pack invariance, refusals before any launch, the batched front-end's bits, a launch count flat in B,
and the pool's lifecycle."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from tests import ref_fixtures as RF

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model(hip_model):
    return hip_model


def _enc(model, seed, T):
    from streamspeech_amd import synth
    fb = torch.from_numpy(synth.synth_fbank(seed, T)).to(model.device)
    return model.encoder_forward(fb, 8, 8)


def _text_args(kind, segment_ms, sr, over=None):
    from streamspeech_amd.agent_text import StreamSpeechASRAgent, StreamSpeechS2TTAgent
    cls = StreamSpeechS2TTAgent if kind == "s2tt" else StreamSpeechASRAgent
    return cls, RF.agent_args(cls, segment_ms, sr, over)


def _drive(pool, plan, cfg):
    """plan: {name: (kind, args, pcm, sr, segment_ms, start_step)} -> {name: [(is_write, content, finished)]} through pool.step()."""
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
        for k, (name, seg) in segs.items():
            o = out[k]
            recs[name].append((not o.is_empty, None if o.is_empty else o.content, bool(o.finished)))
            if seg.finished:
                done.add(name)
        st += 1
    return recs


def test_reference_traces_concurrently(model, synth_weights):
    """s2tt_320_a, s2tt_640_a and asr_320_a in ONE pool, plus a second copy of each started a few steps later: every session's record
    is the reference agent's (actions and text)."""
    from streamspeech_amd.text_pool import TextSessionPool
    cfg = synth_weights[0]
    g, cases = RF.traces_gold()
    pool = TextSessionPool(model, 8, 512)
    plan = {}
    for name in ("s2tt_320_a", "s2tt_640_a", "asr_320_a"):
        c = cases[name]
        _, args = _text_args(c["kind"], c["segment_ms"], c["sr"], c["over"])
        pcm = RF.trace_pcm(c["seed"], c["sr"], c["seconds"])
        for copy, start in (("", 0), ("#2", 3)):
            plan[name + copy] = (c["kind"], args, pcm, c["sr"], c["segment_ms"], start)
    recs = _drive(pool, plan, cfg)
    for name in plan:
        RF.check_text_trace(g, name.split("#")[0], recs[name])


def _sessions(n=24, seed=7):
    from streamspeech_amd import synth
    rng = random.Random(seed)
    out = {}
    for i in range(n):
        kind = "asr" if i % 4 == 3 else "s2tt"
        ms = (320, 640, 960)[i % 3]
        sr = 48000 if i == 5 else 16000
        over = {"lagging_k1": (0, 1, 2)[i % 3], "stride_n": (1, 2)[(i // 3) % 2]}
        secs = 1.0 + 7.0 * rng.random()
        n16 = int(16000 * secs)
        pcm = synth.synth_pcm(1000 + i, n16)
        if sr != 16000:
            pcm = np.repeat(pcm, 3)
        out[f"{kind}{i}"] = (kind, ms, sr, over, pcm, i % 5)
    return out


def test_against_single_session_agents(model, synth_weights):
    """~24 seeded sessions (1-8 s, 320 / 640 / 960 ms segments, lagging / stride variants, one 48-kHz source, ASR and S2TT): each
    session's (is_write, content, finished) sequence equals its own single-session agent's, fed the same segments."""
    from streamspeech_amd.modules import StreamSpeechModel
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.text_pool import TextSessionPool
    cfg = synth_weights[0]
    sess = _sessions()
    plan = {}
    for name, (kind, ms, sr, over, pcm, start) in sess.items():
        _, args = _text_args(kind, ms, sr, over)
        plan[name] = (kind, args, pcm, sr, ms, start)
    pool = TextSessionPool(model, 32, 256)
    got = _drive(pool, plan, cfg)
    for name, (kind, ms, sr, over, pcm, start) in sess.items():
        cls, args = _text_args(kind, ms, sr, over)
        agent = RF.set_dicts(cls(args, model=StreamSpeechModel.from_engine(model)), cfg)
        step, pos, want = sr * ms // 1000, 0, []
        while True:
            chunk = pcm[pos:pos + step]
            pos += step
            fin = pos >= len(pcm)
            o = agent.pushpop(SpeechSegment(content=chunk.tolist(), sample_rate=sr, finished=fin))
            want.append((not o.is_empty, None if o.is_empty else o.content, bool(o.finished)))
            if fin:
                break
        assert got[name] == want, (name, got[name], want)
    model.encoder_stream_set_tail(0)


def _cases(model):
    """Rows of a continuation call: (encoder rows, prefix, max_len) -- an empty prefix, start == max_len (immediate </s>), rows that
    stop at different steps, long and short prefixes."""
    rng = random.Random(3)
    rows = []
    for i in range(10):
        enc = _enc(model, 50 + i, 60 + 23 * i)
        n_pre = [0, 3, 5, 0, 12, 1, 7, 2, 20, 4][i]
        prefix = [rng.randrange(4, model.cfg.tgt_vocab) for _ in range(n_pre)]
        max_len = [n_pre + 6, n_pre, n_pre + 1, 12, n_pre + 3, n_pre + 20, n_pre + 2, n_pre + 9, n_pre + 4, n_pre + 15][i]
        rows.append((enc, prefix, max_len))
    return rows


def _continue(model, rows, min_len=1):
    enc = torch.cat([r[0] for r in rows], 0)
    return model.batch_mt_continue(enc, [r[0].shape[0] for r in rows], [r[1] for r in rows], [r[2] for r in rows], min_len)


@pytest.mark.parametrize("min_len", [1, 4])
def test_continue_matches_mt_greedy_row_by_row(model, min_len):
    rows = _cases(model)
    if min_len > 1:
        rows = [r for r in rows if r[2] >= min_len]
    res = _continue(model, rows, min_len)
    ctx = model.new_context()
    for (enc, prefix, ml), (toks, feats) in zip(rows, res):
        want, wf = ctx.mt_greedy(enc, prefix, ml, min_len)
        assert toks == want, (prefix, ml, toks, want)
        assert feats.shape == wf.shape
        assert float((feats - wf).abs().max()) < 5e-5
        if len(prefix) == ml:
            assert toks == [model.cfg.eos]


def test_continue_pack_invariance(model):
    rows = _cases(model)
    pack = (rows * 2)[:16]
    alone = [_continue(model, [r])[0] for r in rows[:4]]
    inpack = _continue(model, pack)
    rev = _continue(model, pack[::-1])
    for i in range(4):
        for other in (inpack[i], inpack[i + 10] if i + 10 < 16 else inpack[i], rev[15 - i]):
            assert alone[i][0] == other[0]
            assert torch.equal(alone[i][1], other[1])


def test_continue_refusals_before_any_launch(model):
    from streamspeech_amd import lib as L
    from streamspeech_amd.engine import Scratch, _ptr, _stream, _i32
    lib, D = model.lib, model.cfg.dec_dim
    enc = _enc(model, 9, 80)
    Tp = enc.shape[0]
    feats = torch.zeros((2, 40, D), device=model.device)
    out, n_out, n_f = (C.c_int32 * 80)(), (C.c_int32 * 2)(), (C.c_int32 * 2)()

    def call(ctx, B, Tps, pre, npre, ml, stride=40, rows=40):
        return ctx.lib.ss_batch_mt_continue(ctx.h, _stream(), B, _ptr(torch.cat([enc] * B)), _i32(Tps), _i32(pre or [0]), _i32(npre),
                                            _i32(ml), 1, out, stride, n_out, _ptr(feats), rows, n_f)
    torch.cuda.synchronize()
    before = feats.clone()
    assert call(model, 1, [Tp], [5, 6, 7], [3], [2]) == L.SS_ERR_ARG            # start > max_len
    assert call(model, 1, [0], [], [0], [4]) == L.SS_ERR_ARG                     # no encoder rows
    assert call(model, 300, [Tp] * 300, [], [0] * 300, [3] * 300) == L.SS_ERR_ARG
    assert call(model, 1, [Tp], [9999999], [1], [4]) == L.SS_ERR_ARG             # id outside the vocabulary
    assert call(model, 1, [Tp], [], [0], [40]) == L.SS_ERR_CAPACITY              # past feat_rows
    assert call(model, 1, [Tp], [], [0], [30], stride=10) == L.SS_ERR_CAPACITY   # past out_stride
    assert call(model, 1, [Tp], [], [0], [1030], stride=2000, rows=2000) == L.SS_ERR_CAPACITY   # past the decoder's positions
    torch.cuda.synchronize()
    assert torch.equal(feats, before)
    sc = Scratch(model.device)
    ctx = model.new_context(sc)
    sc.set_cap(sc.bytes() + (1 << 20))
    assert call(ctx, 2, [Tp, Tp], [], [0, 0], [20, 20]) == L.SS_ERR_SCRATCH_CAP
    sc.set_cap(0)
    assert call(ctx, 2, [Tp, Tp], [], [0, 0], [20, 20]) == 0
    booked, held = sc.audit()
    assert booked == held


def test_batched_front_end_bits(model):
    """ss_batch_fbank_frames: the new rows of many histories in one launch are the bits of the per-session extractor's rows."""
    from streamspeech_amd import synth
    hist, first, cnt, outs, want = [], [], [], [], []
    for i in range(7):
        n = 4000 + 2311 * i
        pcm = torch.from_numpy(synth.synth_pcm(200 + i, n)).to(model.device)
        nf = model.lib.ss_fbank_num_frames(n)
        k = (5 * i) % max(nf, 1)
        hist.append(pcm); first.append(k); cnt.append(nf - k)
        outs.append(torch.full((nf - k, 80), float("nan"), device=model.device))
        want.append(model.fbank_cmvn(pcm)[k:nf])
    cnt[2] = 0
    outs[2] = outs[2][:0]
    model.batch_fbank_frames(hist, first, cnt, outs)
    for i in range(7):
        if cnt[i]:
            assert torch.equal(outs[i], want[i]), i


def _gemm_dispatch(lib):
    n = lib.ss_prof_shape_dump(None, 0)
    buf = C.create_string_buffer(n)
    lib.ss_prof_shape_dump(buf, n)
    out = {}
    for line in buf.value.decode().splitlines()[1:]:
        f = [int(v) for v in line.split()[:6]]
        out[tuple(f[1:5])] = out.get(tuple(f[1:5]), 0) + f[5]
    return out


def test_launch_count_flat_in_B(model):
    """At a fixed number of lock-step steps (every row forced to </s> at the same step), the GEMM-family launches of one call do not
    grow with B."""
    lib = model.lib
    encs = [_enc(model, 70 + i, 64) for i in range(32)]
    per = []
    lib.ss_prof_shape_log(1)
    try:
        for B in (1, 8, 32):
            rows = [(encs[i], list(range(10, 10 + i % 5)), i % 5 + 4) for i in range(B)]
            torch.cuda.synchronize()
            d0 = _gemm_dispatch(lib)
            _continue(model, rows, 4)                    # min_len 4: no early </s>, every row stops at its forced position
            d1 = _gemm_dispatch(lib)
            per.append(sum(v - d0.get(k, 0) for k, v in d1.items()))
    finally:
        lib.ss_prof_shape_log(0)
    assert per[0] == per[1] == per[2], per


def test_lifecycle(model, synth_weights):
    """A finished session frees its slot and the same id starts a fresh utterance; a push past max_rows raises ValueError naming the
    session, and the others' step proceeds."""
    from streamspeech_amd import synth
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.text_pool import TextSessionPool
    cfg = synth_weights[0]
    d = RF.dictionaries(cfg)
    pool = TextSessionPool(model, 2, 40)
    _, args = _text_args("s2tt", 320, 16000)
    a, b = pool.open("s2tt", args, dicts=d), pool.open("asr", args, dicts=d)
    pcm = synth.synth_pcm(5, 16000)
    first = pool.step({a: SpeechSegment(content=pcm[:5120].tolist(), sample_rate=16000, finished=False),
                       b: SpeechSegment(content=pcm[:5120].tolist(), sample_rate=16000, finished=True)})
    assert set(first) == {a, b}
    assert pool.sessions[b].slot is None and len(pool.free) == 1          # b finished: its slot is back
    with pytest.raises(ValueError, match=f"session {a}"):
        pool.push(a, SpeechSegment(content=[0.0] * 16000 * 2, sample_rate=16000, finished=False))
    again = pool.step({b: SpeechSegment(content=pcm[:5120].tolist(), sample_rate=16000, finished=True)})
    assert again[b].content == first[b].content                           # a fresh utterance of the same audio
    assert pool.sessions[a].states.source == pcm[:5120].tolist()          # the refused push changed nothing
    pool.close(a)
    pool.close(b)
    assert sorted(pool.free) == [0, 1]


def test_more_sessions_than_slots(model, synth_weights):
    """Slots are taken when a session first has frames, so more sessions than slots may be open.  A step whose sessions would need
    more slots than are free is refused whole before anything moves; push() refuses the session that does not fit and the others
    step as usual."""
    from streamspeech_amd import synth
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.text_pool import TextSessionPool
    d = RF.dictionaries(synth_weights[0])
    pool = TextSessionPool(model, 2, 64)
    _, args = _text_args("s2tt", 320, 16000)
    sids = [pool.open("s2tt" if i % 2 == 0 else "asr", args, dicts=d) for i in range(3)]
    pcm = synth.synth_pcm(11, 16000)
    seg = lambda: SpeechSegment(content=pcm[:5120].tolist(), sample_rate=16000, finished=False)    # noqa: E731
    with pytest.raises(ValueError, match=f"session {sids[2]}"):
        pool.step({s: seg() for s in sids})
    for s in sids:                                    # nothing moved
        assert pool.sessions[s].states.source == [] and not pool.sessions[s].pending and pool.sessions[s].slot is None
    assert sorted(pool.free) == [0, 1]
    pool.push(sids[0], seg())
    pool.push(sids[1], seg())
    with pytest.raises(ValueError, match=f"session {sids[2]}"):
        pool.push(sids[2], seg())
    out = pool.step()
    assert set(out) == {sids[0], sids[1]} and pool.sessions[sids[2]].states.source == []
    assert pool.free == [] and not any(pool.sessions[s].pending for s in sids)
    # the next step: every stepped session again one push for one pop
    out = pool.step({sids[0]: seg(), sids[1]: seg()})
    assert set(out) == {sids[0], sids[1]}
    pool.close(sids[1])                               # its slot goes back: the third session fits now
    out = pool.step({sids[2]: seg()})
    assert set(out) == {sids[2]} and pool.sessions[sids[2]].slot is not None


def test_finished_without_new_subword_frees_the_slot(model, synth_weights):
    """An S2TT session whose final search adds no subword answers ('', finished=True) and stays finished, as the agent does (no
    reset()); its slot goes back to the pool at once, later pushes get EmptySegment(finished=True), reset(sid) starts afresh."""
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.text_pool import TextSessionPool
    cfg = synth_weights[0]
    g, cases = RF.traces_gold()
    c = cases["s2tt_320_a"]
    pcm = RF.trace_pcm(c["seed"], c["sr"], c["seconds"])
    _, args = _text_args("s2tt", c["segment_ms"], c["sr"], c["over"])
    pool = TextSessionPool(model, 1, 512)
    sid = pool.open("s2tt", args, dicts=RF.dictionaries(cfg))
    step, pos = c["sr"] * c["segment_ms"] // 1000, 0
    while pool.sessions[sid].tgt_subwords is None:    # up to the first write
        pool.step({sid: SpeechSegment(content=pcm[pos:pos + step].tolist(), sample_rate=c["sr"], finished=False)})
        pos += step
        assert pos + step < len(pcm), "no write before the end of the trace"
    real = model.batch_mt_continue

    def no_new_subword(enc, Tp, prefixes, max_len, min_len=1):     # the real call with </s> forced right after each prefix
        return real(enc, Tp, prefixes, [len(p) for p in prefixes], 0)
    model.batch_mt_continue = no_new_subword
    try:
        out = pool.step({sid: SpeechSegment(content=pcm[pos:].tolist(), sample_rate=c["sr"], finished=True)})
    finally:
        del model.batch_mt_continue
    assert out[sid].content == "" and out[sid].finished
    s = pool.sessions[sid]
    assert s.states.target_finished and s.slot is None and pool.free == [0]
    again = pool.step({sid: SpeechSegment(content=pcm[:step].tolist(), sample_rate=c["sr"], finished=False)})
    assert again[sid].is_empty and again[sid].finished
    pool.reset(sid)
    fresh = pool.step({sid: SpeechSegment(content=pcm[:step].tolist(), sample_rate=c["sr"], finished=False)})
    assert not fresh[sid].finished and pool.sessions[sid].states.source == pcm[:step].tolist()
