"""Concurrent S2ST sessions over the session pool (streamspeech_amd/speech_pool.py) and the batched write side they share, on the GPU:
reference traces served concurrently, agreement with single-session S2ST agents, the tail-pad masks of the ragged unit decoder
(ss_batch_t2u_units_pad), the features-only MT pass (ss_batch_mt_features), the receptive-field vocoder tail (ss_batch_vocoder_tail),
refusals before any launch, and a write-side launch count flat in the number of writers."""
import ctypes as C
import random

import numpy as np
import pytest
import torch

from tests import ref_fixtures as RF

pytestmark = pytest.mark.gpu

WAV_RMS_TOL = 1e-3          # against the reference agent's fixtures (tests/test_reference_agent_gpu.py)
BATCH_RMS_TOL = 1e-5        # batched against single-utterance vocoder (tests/test_batch_gpu.py)
STATE_TOL = 5e-5            # decoder states, batched against the single-utterance path


@pytest.fixture(scope="module")
def model(hip_model):
    return hip_model


class HipVocSurface:
    """CodeHiFiGANVocoderWithDur call surface over the shared fixture handle (as tests/test_reference_agent_gpu.py)."""

    def __init__(self, hv):
        self.hip = hv

    def __call__(self, x, dur_prediction=False):
        from streamspeech_amd.modules import CodeHiFiGANVocoderWithDur
        return CodeHiFiGANVocoderWithDur.__call__(self, x, dur_prediction)


def _enc(model, seed, T):
    from streamspeech_amd import synth
    fb = torch.from_numpy(synth.synth_fbank(seed, T)).to(model.device)
    return model.encoder_forward(fb, 8, 8)


def _s2st_args(segment_ms, sr, over=None):
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    return RF.agent_args(StreamSpeechS2STAgent, segment_ms, sr, over)


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


S2ST_TRACES = ("s2st_320_a", "s2st_320_b", "s2st_320_k3", "s2st_640_a", "s2st_640_b", "s2st_960_a", "s2st_320_48k")


def test_reference_traces_concurrently(model, hip_vocoder, synth_weights):
    """The seven S2ST reference traces in ONE pool (whole-word mode at 640 / 960 ms with a tail-padded final write, the 48-kHz
    front-end), plus a second copy of each started a few steps later: every session passes the reference agent's trace check."""
    from streamspeech_amd.speech_pool import SpeechSessionPool
    cfg = synth_weights[0]
    g, cases = RF.traces_gold()
    pool = SpeechSessionPool(model, 16, 512, vocoder=hip_vocoder)
    plan = {}
    for name in S2ST_TRACES:
        c = cases[name]
        args = _s2st_args(c["segment_ms"], c["sr"], c["over"])
        pcm = RF.trace_pcm(c["seed"], c["sr"], c["seconds"])
        for copy, start in (("", 0), ("#2", 3)):
            plan[name + copy] = ("s2st", args, pcm, c["sr"], c["segment_ms"], start)
    recs = _drive(pool, plan, cfg)
    for name in plan:
        RF.check_s2st_trace(g, name.split("#")[0], recs[name], WAV_RMS_TOL)


def _sessions(n=16, seed=11):
    from streamspeech_amd import synth
    rng = random.Random(seed)
    out = {}
    for i in range(n):
        ms = (320, 640, 960)[i % 3]
        sr = 48000 if i == 4 else 16000
        over = {"lagging_k1": (0, 1, 2)[(i // 3) % 3], "stride_n": (1, 2)[(i // 2) % 2]}
        secs = 1.0 + 7.0 * rng.random()
        pcm = synth.synth_pcm(2000 + i, int(16000 * secs))
        if sr != 16000:
            pcm = np.repeat(pcm, 3)
        out[f"s2st{i}"] = (ms, sr, over, pcm, i % 4)
    return out


def test_against_single_session_agents(model, hip_vocoder, synth_weights):
    """16 seeded sessions (1-8 s, 320 / 640 / 960 ms, lagging / stride variants, one 48-kHz source) with 4 S2TT sessions in the
    same pool: each S2ST session's READ / WRITE sequence, finished flags and per-write sample counts equal its own
    StreamSpeechS2STAgent's, and its speech is within the batched-vocoder bar of the agent's."""
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.agent_text import StreamSpeechS2TTAgent
    from streamspeech_amd.modules import StreamSpeechModel
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.speech_pool import SpeechSessionPool
    from streamspeech_amd import synth
    cfg = synth_weights[0]
    sess = _sessions()
    plan = {name: ("s2st", _s2st_args(ms, sr, over), pcm, sr, ms, start) for name, (ms, sr, over, pcm, start) in sess.items()}
    for i in range(4):                                   # text writers share the step's MT call
        plan[f"s2tt{i}"] = ("s2tt", RF.agent_args(StreamSpeechS2TTAgent, 320, 16000), synth.synth_pcm(3000 + i, 16000 * (2 + i)),
                            16000, 320, i)
    pool = SpeechSessionPool(model, 32, 256, vocoder=hip_vocoder)
    got = _drive(pool, plan, cfg)
    n_writes = 0
    for name, (ms, sr, over, pcm, start) in sess.items():
        agent = RF.set_dicts(StreamSpeechS2STAgent(_s2st_args(ms, sr, over), model=StreamSpeechModel.from_engine(model),
                                                   vocoder=HipVocSurface(hip_vocoder)), cfg)
        step, pos, want = sr * ms // 1000, 0, []
        while True:
            chunk = pcm[pos:pos + step]
            pos += step
            fin = pos >= len(pcm)
            o = agent.pushpop(SpeechSegment(content=chunk.tolist(), sample_rate=sr, finished=fin))
            want.append((not o.is_empty, None if o.is_empty else o.content, bool(o.finished)))
            if fin:
                break
        g = got[name]
        assert [(w, f) for w, _, f in g] == [(w, f) for w, _, f in want], name
        assert [len(c or []) for _, c, _ in g] == [len(c or []) for _, c, _ in want], name
        for (_, a, _), (_, b, _) in zip(g, want):
            if a:
                n_writes += 1
                rms = float(np.sqrt(np.mean((np.asarray(a, np.float32) - np.asarray(b, np.float32)) ** 2)))
                assert rms < BATCH_RMS_TOL, (name, rms)
    assert n_writes > len(sess)                          # speech was written, more than once per session on the whole
    model.encoder_stream_set_tail(0)


def _mt_rows(model, n=8):
    """(encoder rows, hypothesis tokens without </s>) of n utterances: greedy searches of the single-utterance path."""
    rows = []
    for i in range(n):
        enc = _enc(model, 300 + i, 70 + 19 * i)
        toks, _ = model.mt_greedy(enc, [], 4 + 3 * i, 1)
        rows.append((enc, [t for t in toks if t != model.cfg.eos]))
    return rows


def test_mt_features_match_truncate_append(model):
    """ss_batch_mt_features against ss_mt_truncate + ss_mt_append(n_tail_pad = 1) row by row, tail pads 0 / 1 mixed in one pack."""
    rows = _mt_rows(model)
    pads = [i % 2 for i in range(len(rows))]
    enc = torch.cat([e for e, _ in rows], 0)
    got = model.batch_mt_features(enc, [e.shape[0] for e, _ in rows], [t for _, t in rows], pads)
    for (e, toks), p, f in zip(rows, pads, got):
        n = len(toks) + 1
        _, ref = model.mt_greedy(e, toks, n, 1)            # states of [</s>, toks...] (and the forced </s> step)
        ref = ref[:n]
        if p:
            model.mt_truncate(n)
            pf, _ = model.mt_append([model.cfg.pad], n, False, False, want_next=False, n_tail_pad=1)
            ref = torch.cat((ref, pf), 0)
        assert f.shape == ref.shape
        assert float((f - ref).abs().max()) < STATE_TOL


def _t2u_pack(model):
    rows = _mt_rows(model)
    feats = []
    for e, toks in rows:
        _, f = model.mt_greedy(e, toks, len(toks) + 1, 1)
        feats.append(f[:len(toks) + 1])
    return feats


def _pack(model, feats):
    D = model.cfg.dec_dim
    out = torch.zeros((len(feats), max(f.shape[0] for f in feats), D), device=model.device)
    for i, f in enumerate(feats):
        out[i, :f.shape[0]] = f
    return out


def _t2u_logits(model, feats, pads):
    n = [f.shape[0] for f in feats]
    toks = model.batch_t2u_units_pad(_pack(model, feats), n, pads) if pads is not None else \
        model.batch_t2u_units(_pack(model, feats), n)
    lg = model.last_logits().clone()
    up, off, per = model.cfg.ctc_upsample, 0, []
    for k in n:
        per.append(lg[off:off + k * up])
        off += k * up
    return toks, per


def test_t2u_units_pad(model):
    """Mixed tail pads in one pack: tokens equal ss_t2u_units(n_tail_pad) row by row; pad-0 rows carry the bits of
    ss_batch_t2u_units; every row has the same bits alone, in the pack and in the reversed pack."""
    feats = _t2u_pack(model)
    pads = [(i + 1) % 2 for i in range(len(feats))]
    toks, lg = _t2u_logits(model, feats, pads)
    for f, p, t in zip(feats, pads, toks):
        want, _, _ = model.t2u_units(f, n_tail_pad=p)
        assert t == want
    plain_toks, plain_lg = _t2u_logits(model, feats, None)
    for i, p in enumerate(pads):
        if p == 0:
            assert plain_toks[i] == toks[i] and torch.equal(plain_lg[i], lg[i]), i
    rtoks, rlg = _t2u_logits(model, feats[::-1], pads[::-1])
    R = len(feats)
    for i in range(R):
        atoks, alg = _t2u_logits(model, [feats[i]], [pads[i]])
        assert atoks[0] == toks[i] == rtoks[R - 1 - i]
        assert torch.equal(alg[0], lg[i]) and torch.equal(rlg[R - 1 - i], lg[i]), i


def test_vocoder_tail_matches_synthesize_tail(hip_vocoder):
    """ss_batch_vocoder_tail against the agent's synthesize_tail on the same units: a pack of rows whose window covers the
    receptive field, rows that must fall back to all units, and rows shorter than a window.  Durations and sample counts equal,
    tails within the batched-vocoder bar."""
    from streamspeech_amd.agent import synthesize_tail
    v = hip_vocoder
    rf = v.cfg.receptive_field_frames()
    rng = random.Random(5)
    rows = []
    for i in range(9):
        K = [60, 80, 12, 45, 100, 30, 70, 9, 55][i]
        n_new = [3, 7, 4, 1, 10, 5, 2, 9, 6][i]
        ctx = [rf + 8, 3, rf + 8, 4, rf + 8, 2, 5, rf + 8, rf + 8][i]
        rows.append(([rng.randrange(0, 1000) for _ in range(K)], n_new, ctx))
    tails, info = v.batch_tail([u for u, _, _ in rows], [n for _, n, _ in rows], [c for _, _, c in rows], [rf] * len(rows))
    surf = HipVocSurface(v)
    kinds = set()
    for (units, n_new, ctx), t, (first, dur) in zip(rows, tails, info):
        windowed = len(units) > n_new + ctx
        want, _ = synthesize_tail(surf, units, n_new, True, ctx, rf)
        _, wdur = v.forward(units[first:], True)
        assert dur == wdur.cpu().tolist()
        kinds.add("short" if not windowed else "window" if first > 0 else "fallback")
        if windowed and first > 0:
            assert first == len(units) - (n_new + ctx) and sum(dur[2:ctx]) >= rf + 2
        if windowed and first == 0:
            _, d = v.forward(units[-(n_new + ctx):], True)
            assert int(d[2:ctx].sum()) < rf + 2
        assert t.numel() == want.numel() == sum(dur[-n_new:]) * v.hop
        assert float(torch.sqrt(torch.mean((t - want) ** 2))) < BATCH_RMS_TOL
    assert kinds == {"short", "window", "fallback"}, kinds


def test_refusals_before_any_launch(model, hip_vocoder, synth_weights):
    """An s2st session without a vocoder, with --full-recompute-encoder, over-capacity pushes and bad arguments of the new entry
    points are refused before anything runs, and no session or output changes."""
    from streamspeech_amd import lib as L
    from streamspeech_amd.engine import _i32, _ptr, _stream
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.speech_pool import SpeechSessionPool
    from streamspeech_amd import synth
    cfg = synth_weights[0]
    d = RF.dictionaries(cfg)
    with pytest.raises(ValueError):
        SpeechSessionPool(model, 2, 64).open("s2st", _s2st_args(320, 16000), dicts=d)
    pool = SpeechSessionPool(model, 2, 64, vocoder=hip_vocoder)
    with pytest.raises(ValueError):
        pool.open("s2st", _s2st_args(320, 16000, {"full_recompute_encoder": True}), dicts=d)
    a, b = pool.open("s2st", _s2st_args(320, 16000), dicts=d), pool.open("s2st", _s2st_args(320, 16000), dicts=d)
    ok = SpeechSegment(content=synth.synth_pcm(1, 5120).tolist(), sample_rate=16000, finished=False)
    big = SpeechSegment(content=synth.synth_pcm(2, 16000 * 4).tolist(), sample_rate=16000, finished=False)   # > 64 rows
    with pytest.raises(ValueError):
        pool.step({a: ok, b: big})
    assert len(pool.sessions[a].states.source) == 0 and len(pool.sessions[b].states.source) == 0
    assert len(pool.free) == 2
    pool.step({a: ok, b: ok})                             # the same pool steps as usual afterwards
    # C ABI arguments
    lib, D = model.lib, model.cfg.dec_dim
    feats = torch.zeros((2, 8, D), device=model.device)
    ibuf = torch.full((64,), -7, dtype=torch.int32, device=model.device)
    enc = _enc(model, 9, 80)
    torch.cuda.synchronize()
    assert lib.ss_batch_t2u_units_pad(model.h, _stream(), 2, _ptr(feats), 8, _i32([3, 2]), _i32([0, 2]), 0, 0, _ptr(ibuf),
                                      _ptr(ibuf), _ptr(ibuf)) == L.SS_ERR_ARG                 # every state padding
    assert lib.ss_batch_t2u_units_pad(model.h, _stream(), 2, _ptr(feats), 8, _i32([3, 2]), None, 0, 0, _ptr(ibuf),
                                      _ptr(ibuf), _ptr(ibuf)) == L.SS_ERR_ARG
    Tp = enc.shape[0]
    assert lib.ss_batch_mt_features(model.h, _stream(), 1, _ptr(enc), _i32([Tp]), _i32([999999]), _i32([1]), _i32([0]),
                                    _ptr(feats), 8) == L.SS_ERR_ARG                           # id outside the vocabulary
    assert lib.ss_batch_mt_features(model.h, _stream(), 1, _ptr(enc), _i32([Tp]), _i32([5] * 8), _i32([8]), _i32([1]),
                                    _ptr(feats), 8) == L.SS_ERR_CAPACITY                      # 10 rows past feat_rows 8
    assert lib.ss_batch_mt_features(model.h, _stream(), 1, _ptr(enc), _i32([0]), _i32([5]), _i32([1]), _i32([0]),
                                    _ptr(feats), 8) == L.SS_ERR_ARG                           # no encoder rows
    codes = torch.arange(10, dtype=torch.int32, device=model.device)
    wav = torch.full((64,), 7.0, device=model.device)
    first, dur = (C.c_int32 * 2)(), (C.c_int32 * 20)()
    st, ns = (C.c_int64 * 2)(), (C.c_int64 * 2)()
    vl = hip_vocoder.lib
    assert vl.ss_batch_vocoder_tail(hip_vocoder.h, _stream(), 2, _ptr(codes), _i32([5, 5]), _i32([6, 1]), _i32([0, 0]),
                                    _i32([0, 0]), 1, _ptr(wav), 64, first, dur, st, ns) == L.SS_ERR_ARG   # n_new > K
    assert vl.ss_batch_vocoder_tail(hip_vocoder.h, _stream(), 2, _ptr(codes), _i32([5, 5]), _i32([1, 1]), _i32([2, 0]),
                                    _i32([-1, 0]), 1, _ptr(wav), 64, first, dur, st, ns) == L.SS_ERR_ARG  # window without rf
    assert vl.ss_batch_vocoder_tail(hip_vocoder.h, _stream(), 2, _ptr(codes), _i32([5, 5]), _i32([1, 1]), _i32([0, 0]),
                                    _i32([0, 0]), 1, _ptr(wav), 64, first, dur, st, ns) == L.SS_ERR_CAPACITY  # tail > 64 samples
    torch.cuda.synchronize()
    assert torch.equal(feats, torch.zeros_like(feats)) and bool((ibuf == -7).all()) and bool((wav == 7.0).all())


def _gemm_dispatch(lib):
    n = lib.ss_prof_shape_dump(None, 0)
    buf = C.create_string_buffer(n)
    lib.ss_prof_shape_dump(buf, n)
    out = {}
    for line in buf.value.decode().splitlines()[1:]:
        f = [int(v) for v in line.split()[:6]]
        out[tuple(f[1:5])] = out.get(tuple(f[1:5]), 0) + f[5]
    return out


def test_write_side_launch_count_flat(model, hip_vocoder):
    """The GEMM-family launches of the unit side of a step (MT feature pass, T2U + unit decoder) do not grow with the number of
    writers; the vocoder tail launches exactly the GEMMs of ss_batch_vocoder_forward over the windows it synthesises (the generator's
    kernel choice follows the pack's frame count there as well)."""
    lib = model.lib
    rf = hip_vocoder.cfg.receptive_field_frames()
    feats = _t2u_pack(model)
    rows = _mt_rows(model)
    rng = random.Random(9)
    units = [[rng.randrange(0, 1000) for _ in range(40 + 3 * i)] for i in range(8)]

    def census(fn):
        torch.cuda.synchronize()
        d0 = _gemm_dispatch(lib)
        fn()
        torch.cuda.synchronize()
        d1 = _gemm_dispatch(lib)
        return sum(v - d0.get(k, 0) for k, v in d1.items())

    per = []
    lib.ss_prof_shape_log(1)
    try:
        for B in (1, 4, 8):
            enc = torch.cat([e for e, _ in rows[:B]], 0)
            per.append(census(lambda: (
                model.batch_mt_features(enc, [e.shape[0] for e, _ in rows[:B]], [t for _, t in rows[:B]], [1] * B),
                model.batch_t2u_units_pad(_pack(model, feats[:B]), [f.shape[0] for f in feats[:B]], [1] * B))))
            ctx = rf + 8
            tail = census(lambda: hip_vocoder.batch_tail(units[:B], [4] * B, [ctx] * B, [rf] * B))
            whole = census(lambda: hip_vocoder.batch_forward([u[-(4 + ctx):] for u in units[:B]]))
            assert tail == whole, (B, tail, whole)
    finally:
        lib.ss_prof_shape_log(0)
    assert per[0] == per[1] == per[2], per
