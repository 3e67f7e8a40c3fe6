"""Multi-speaker unit vocoder on the GPU: the speaker add kernel bit for bit against its NumPy restatement, the three entry points
against the reference class's recorded outputs and against each other, the refusals, and the voice per session / agent."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest
import torch

from tests import multispkr_ref as MR
from tests import ref_fixtures as RF

pytestmark = pytest.mark.gpu

WAV_RMS_TOL = 1e-3          # tests/test_stages_gpu.py: waveform against the reference's golden (max 5e-3)
BATCH_RMS_TOL = 1e-5        # tests/test_speech_pool_gpu.py: batched against single-utterance vocoder
TAIL_RMS_TOL = 1e-5         # tests/test_stages_gpu.py test_incremental_vocoder_tail_on_hip
FP16_RMS_TOL = 1e-3         # tests/test_vocoder_f16_gpu.py: FP16 against the f32 path
NUM_SPEAKERS = 5


@pytest.fixture(scope="module")
def multi_voc():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import synth
    from streamspeech_amd.engine import HipVocoder
    vcfg = MR.multispkr_config(NUM_SPEAKERS)
    v = HipVocoder(synth.make_vocoder_state_dict(0, vcfg), vcfg)
    assert v.num_speakers == NUM_SPEAKERS
    return v


@pytest.fixture(scope="module")
def gold(golden_dir):
    return np.load(os.path.join(golden_dir, "vocoder_multispkr.npz"))


class VocSurface:
    """CodeHiFiGANVocoderWithDur call surface over a HipVocoder handle (as tests/test_speech_pool_gpu.py)."""

    def __init__(self, hv):
        self.hip = hv

    def __call__(self, x, dur_prediction=False):
        from streamspeech_amd.modules import CodeHiFiGANVocoderWithDur
        return CodeHiFiGANVocoderWithDur.__call__(self, x, dur_prediction)


def _rms(a, b):
    return float(torch.sqrt(torch.mean((a.float().cpu() - b.float().cpu()) ** 2)))


# ---- op level ---------------------------------------------------------------------------------------------------------------
OP_SPEAKERS = (0, 4, 2, 2, 0, 1, 3, 4)


def _op_pack():
    """8 segments of MR.SEG_LENGTHS with gaps before, between and after them -> (segs [(start, L)], M)."""
    segs, at = [], 2
    for i, L in enumerate(MR.SEG_LENGTHS):
        segs.append((at, L))
        at += L + (3 if i % 3 == 1 else 0)
    return segs, at + 5


@pytest.mark.parametrize("C0,ld", [(512, 512), (32, 48)])
@pytest.mark.parametrize("act", [0, 1])
def test_op_spkr_pre_add_bit_exact(C0, ld, act):
    from streamspeech_amd import lib as L
    from streamspeech_amd.engine import _ptr, _stream
    lib = L.load()
    segs, M = _op_pack()
    rng = np.random.default_rng(100 + C0 + act)
    x = rng.standard_normal((M, ld)).astype(np.float32)
    table = rng.standard_normal((NUM_SPEAKERS, 16, C0)).astype(np.float32)
    want_rows = MR.spkr_pre_add_np(x, C0, table, OP_SPEAKERS, segs, act)
    dev = "cuda:0"
    dx, dt = torch.from_numpy(x).to(dev), torch.from_numpy(table).to(dev)
    dsegs = torch.tensor([[s, n, s, n] for s, n in segs], dtype=torch.int32, device=dev)
    dspk = torch.tensor(OP_SPEAKERS, dtype=torch.int32, device=dev)
    if act:
        # the activated output goes to a second tensor (what the first up-conv reads); x stays as conv_pre left it
        sentinel = np.float32(-77.0)
        dy = torch.full((M, ld), float(sentinel), device=dev)
        want = np.full((M, ld), sentinel, np.float32)
        for s, n in segs:
            want[s:s + n, :C0] = want_rows[s:s + n, :C0]
    else:
        dy, want = dx, want_rows                             # in place; rows outside the segments and columns past C0 keep x
    L.check(lib.ss_op_spkr_pre_add(_stream(), _ptr(dx), _ptr(dy), ld, C0, _ptr(dt), _ptr(dspk), 0, _ptr(dsegs), len(segs),
                                   max(MR.SEG_LENGTHS), M, act, 0.1), "ss_op_spkr_pre_add")
    torch.cuda.synchronize()
    got = dy.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    if act:
        assert np.array_equal(dx.cpu().numpy().view(np.uint32), x.view(np.uint32))
    # the single-utterance form: one segment of all M rows, the speaker by value
    dx1 = torch.from_numpy(x).to(dev)
    L.check(lib.ss_op_spkr_pre_add(_stream(), _ptr(dx1), _ptr(dx1), ld, C0, _ptr(dt), None, 3, None, 0, 0, M, act, 0.1),
            "ss_op_spkr_pre_add")
    torch.cuda.synchronize()
    want1 = MR.spkr_pre_add_np(x, C0, table, [3], [(0, M)], act)
    assert np.array_equal(dx1.cpu().numpy().view(np.uint32), want1.view(np.uint32))


# ---- against the reference class ----------------------------------------------------------------------------------------------
def test_forward_vs_reference_golden(multi_voc, gold):
    for name in gold["names"].tolist():
        codes = gold[f"{name}/codes"].tolist()
        for s in gold["speakers"].tolist():
            for dp, tag in ((True, "dur"), (False, "nodur")):
                wav, dur = multi_voc.forward(codes, dur_prediction=dp, speaker=s)
                ref = gold[f"{name}/s{s}/{tag}/wav"]
                assert dur.cpu().tolist() == gold[f"{name}/s{s}/{tag}/dur"].tolist(), (name, s, tag)
                w = wav.cpu().numpy()
                assert w.shape == ref.shape
                rms, mx = float(np.sqrt(np.mean((w - ref) ** 2))), float(np.abs(w - ref).max())
                print(f"{name} speaker {s} {tag}: rms {rms:.3e} max {mx:.3e}")
                assert rms < WAV_RMS_TOL and mx < 5e-3, (name, s, tag, rms, mx)
    codes = gold["six/codes"].tolist()
    w0, _ = multi_voc.forward(codes, True, speaker=0)
    other = float(np.sqrt(np.mean((w0.cpu().numpy() - gold["six/s2/dur/wav"]) ** 2)))
    assert other > 0.05, other                               # an ignored speaker id would pass the bars above


# ---- pack equals single ---------------------------------------------------------------------------------------------------------
def _sequences(gold):
    rng = random.Random(21)
    seqs = [gold[f"{n}/codes"].tolist() for n in ("six", "one", "two")]
    return seqs + [[rng.randrange(0, 1000) for _ in range(k)] for k in (23, 9)]


def test_batch_forward_equals_single(multi_voc, gold):
    seqs = _sequences(gold)
    speakers = [0, 4, 2, 2, NUM_SPEAKERS - 1]                # the same speaker twice, both ends of the id range
    for dp in (True, False):
        singles = [multi_voc.forward(c, dp, speaker=s) for c, s in zip(seqs, speakers)]
        singles = [(w.clone(), d.cpu().tolist()) for w, d in singles]
        wavs, dur, K = multi_voc.batch_forward(seqs, dur_prediction=dp, speakers=speakers)
        dur, off = dur.cpu().tolist(), 0
        for (w1, d1), w, k in zip(singles, wavs, K):
            assert dur[off:off + k] == d1
            off += k
            assert w.shape == w1.shape and _rms(w, w1) < BATCH_RMS_TOL
        wavs = [w.clone() for w in wavs]
        perm = [3, 0, 4, 2, 1]
        pw, pdur, _ = multi_voc.batch_forward([seqs[i] for i in perm], dur_prediction=dp, speakers=[speakers[i] for i in perm])
        for j, i in enumerate(perm):
            assert pw[j].shape == wavs[i].shape and _rms(pw[j], wavs[i]) < BATCH_RMS_TOL
    # the voices are per row: swapping two rows' speakers changes both rows
    sw, _, _ = multi_voc.batch_forward(seqs[:2], speakers=[4, 0])
    ow, _, _ = multi_voc.batch_forward(seqs[:2], speakers=[0, 4])
    assert _rms(sw[0], ow[0]) > 0.05 and _rms(sw[1], ow[1]) > 0.05


# ---- tail ---------------------------------------------------------------------------------------------------------------------
def test_batch_tail_with_speakers(multi_voc):
    from streamspeech_amd.agent import synthesize_tail
    v = multi_voc
    rf = v.cfg.receptive_field_frames()
    rng = random.Random(5)
    # a windowed row, a row whose 3-unit context cannot cover the receptive field (falls back to all units), a row shorter than its window
    rows = [([rng.randrange(0, 1000) for _ in range(K)], n_new, ctx) for K, n_new, ctx in ((60, 3, rf + 8), (80, 7, 3), (12, 4, rf + 8))]
    speakers = [4, 0, 2]
    tails, info = v.batch_tail([u for u, _, _ in rows], [n for _, n, _ in rows], [c for _, _, c in rows], [rf] * 3, speakers=speakers)
    tails = [t.clone() for t in tails]
    surf, kinds = VocSurface(v), []
    for (units, n_new, ctx), s, t, (first, dur) in zip(rows, speakers, tails, info):
        windowed = len(units) > n_new + ctx
        kinds.append("short" if not windowed else "window" if first > 0 else "fallback")
        want, _ = synthesize_tail(surf, units, n_new, True, ctx, rf, spkr=s)
        assert t.shape == want.shape and _rms(t, want) < BATCH_RMS_TOL, (kinds[-1], _rms(t, want))
        full, fdur = v.forward(units, True, speaker=s)
        keep = int(fdur[-n_new:].sum()) * v.hop
        assert dur[-n_new:] == fdur[-n_new:].cpu().tolist()
        assert t.numel() == keep and _rms(t, full[-keep:]) < TAIL_RMS_TOL, (kinds[-1], _rms(t, full[-keep:]))
        wrong, _ = v.forward(units, True, speaker=(s + 1) % NUM_SPEAKERS)
        assert _rms(t, wrong[-keep:]) > 0.05                 # the row kept ITS voice through the reordering of the generator rows
    assert kinds == ["window", "fallback", "short"], kinds


# ---- FP16 ------------------------------------------------------------------------------------------------------------------------
def test_fp16_speaker_path(multi_voc, gold):
    codes = _sequences(gold)[3]
    w32, d32 = multi_voc.forward(codes, True, speaker=3)
    w32, d32 = w32.clone(), d32.cpu().tolist()
    multi_voc.set_fp16(True)
    try:
        w16, d16 = multi_voc.forward(codes, True, speaker=3)
        assert d16.cpu().tolist() == d32
        assert w16.shape == w32.shape and _rms(w16, w32) < FP16_RMS_TOL
        bw, _, _ = multi_voc.batch_forward([codes, codes[:5]], speakers=[3, 1])
        assert _rms(bw[0], w16) < BATCH_RMS_TOL
    finally:
        multi_voc.set_fp16(False)
    back, _ = multi_voc.forward(codes, True, speaker=3)
    assert torch.equal(back, w32)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals(multi_voc, hip_vocoder):
    from streamspeech_amd import lib as L
    from streamspeech_amd.engine import _i32, _ptr, _stream
    dev = multi_voc.device
    codes = torch.arange(10, dtype=torch.int32, device=dev)
    wav = torch.full((10 * 64 * 320,), 7.0, device=dev)
    dur = torch.full((10,), -7, dtype=torch.int32, device=dev)
    ns, st2, ns2 = C.c_int64(-1), (C.c_int64 * 2)(), (C.c_int64 * 2)()
    first, hdur = (C.c_int32 * 2)(), (C.c_int32 * 10)()
    cap = wav.numel()
    torch.cuda.synchronize()
    for v in (multi_voc, hip_vocoder):
        lib, h = v.lib, v.h
        bad = (-1, NUM_SPEAKERS) if v is multi_voc else (0,)   # an id outside the range; any speaker on a single-speaker handle
        for s in bad:
            assert lib.ss_vocoder_forward_spkr(h, _stream(), _ptr(codes), 10, 1, None, _ptr(wav), cap, _ptr(dur), C.byref(ns), s) \
                == L.SS_ERR_ARG
            assert lib.ss_batch_vocoder_forward_spkr(h, _stream(), 2, _ptr(codes), _i32([5, 5]), 1, None, _ptr(wav), cap, _ptr(dur),
                                                     st2, ns2, _i32([0, s])) == L.SS_ERR_ARG
            assert lib.ss_batch_vocoder_tail_spkr(h, _stream(), 2, _ptr(codes), _i32([5, 5]), _i32([1, 1]), _i32([0, 0]),
                                                  _i32([0, 0]), 1, _ptr(wav), cap, first, hdur, st2, ns2, _i32([s, 0])) == L.SS_ERR_ARG
        if v is multi_voc:                                    # the no-speaker forms on a multi-speaker handle
            assert lib.ss_vocoder_forward(h, _stream(), _ptr(codes), 10, 1, None, _ptr(wav), cap, _ptr(dur), C.byref(ns)) == L.SS_ERR_ARG
            assert lib.ss_batch_vocoder_forward(h, _stream(), 2, _ptr(codes), _i32([5, 5]), 1, None, _ptr(wav), cap, _ptr(dur),
                                                st2, ns2) == L.SS_ERR_ARG
            assert lib.ss_batch_vocoder_tail(h, _stream(), 2, _ptr(codes), _i32([5, 5]), _i32([1, 1]), _i32([0, 0]), _i32([0, 0]), 1,
                                             _ptr(wav), cap, first, hdur, st2, ns2) == L.SS_ERR_ARG
            assert lib.ss_batch_vocoder_forward_spkr(h, _stream(), 2, _ptr(codes), _i32([5, 5]), 1, None, _ptr(wav), cap, _ptr(dur),
                                                     st2, ns2, None) == L.SS_ERR_ARG
    torch.cuda.synchronize()
    assert bool((wav == 7.0).all()) and bool((dur == -7).all()) and ns.value == -1       # refused before anything ran
    assert multi_voc.lib.ss_vocoder_num_speakers(multi_voc.h) == NUM_SPEAKERS and hip_vocoder.num_speakers == 0
    # the Python surface
    with pytest.raises(ValueError):
        multi_voc.forward([1, 2, 3])
    with pytest.raises(ValueError):
        multi_voc.batch_forward([[1, 2], [3]])
    with pytest.raises(ValueError):
        multi_voc.batch_tail([[1, 2]], [1], [0], [0])
    with pytest.raises(ValueError):
        multi_voc.batch_forward([[1, 2], [3]], speakers=[1])
    for s in (-1, NUM_SPEAKERS):
        with pytest.raises(IndexError):
            multi_voc.forward([1, 2, 3], speaker=s)
        with pytest.raises(IndexError):
            multi_voc.batch_forward([[1, 2], [3]], speakers=[0, s])
        with pytest.raises(IndexError):
            multi_voc.batch_tail([[1, 2]], [1], [0], [0], speakers=[s])
    with pytest.raises(ValueError):
        hip_vocoder.forward([1, 2, 3], speaker=0)
    with pytest.raises(ValueError):
        hip_vocoder.batch_forward([[1, 2]], speakers=[0])
    # correct calls afterwards still work, on both handles and on a second context over the same blob (same table)
    a, _ = multi_voc.forward([1, 2, 3], True, speaker=1)
    ctx2 = multi_voc.new_context()
    assert ctx2.num_speakers == NUM_SPEAKERS
    b, _ = ctx2.forward([1, 2, 3], True, speaker=1)
    assert a.numel() > 0 and torch.equal(a, b)
    w, _ = hip_vocoder.forward([1, 2, 3], True)
    assert w.numel() > 0


# ---- pool and agent -------------------------------------------------------------------------------------------------------------------
def _s2st_args(extra=()):
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    return RF.agent_args(StreamSpeechS2STAgent, 320, 16000, None, extra)


def _run_agent(agent, pcm, step=5120):
    from streamspeech_amd.simuleval_shim import SpeechSegment
    out = []
    for pos in range(0, len(pcm), step):
        fin = pos + step >= len(pcm)
        o = agent.pushpop(SpeechSegment(content=pcm[pos:pos + step].tolist(), sample_rate=16000, finished=fin))
        out.append((not o.is_empty, None if o.is_empty else o.content, bool(o.finished)))
    return out


def test_pool_sessions_with_their_own_voices(hip_model, multi_voc, synth_weights):
    from streamspeech_amd import synth
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.modules import StreamSpeechModel
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.speech_pool import SpeechSessionPool
    cfg = synth_weights[0]
    d = RF.dictionaries(cfg)
    voices = (0, 2, 4)
    pcm = synth.synth_pcm(2003, 16000 * 2)
    pool = SpeechSessionPool(hip_model, 4, 256, vocoder=multi_voc)
    with pytest.raises(ValueError):
        pool.open("s2st", _s2st_args(), dicts=d)             # no voice: refused at open()
    sids = [pool.open("s2st", _s2st_args(("--speaker-id", str(k))), dicts=d) for k in voices]
    got = {s: [] for s in sids}
    steps_with_writers = 0
    for pos in range(0, len(pcm), 5120):
        fin = pos + 5120 >= len(pcm)
        out = pool.step({s: SpeechSegment(content=pcm[pos:pos + 5120].tolist(), sample_rate=16000, finished=fin) for s in sids})
        ls = pool.last_step
        assert ls["vocoder_tail_calls"] == (1 if ls["speech_writers"] else 0)   # three voices, ONE tail call
        steps_with_writers += 1 if ls["speech_writers"] else 0
        for s in sids:
            got[s].append((not out[s].is_empty, None if out[s].is_empty else out[s].content, bool(out[s].finished)))
    assert steps_with_writers >= 1
    speech = {}
    for k, s in zip(voices, sids):
        agent = RF.set_dicts(StreamSpeechS2STAgent(_s2st_args(("--speaker-id", str(k))), model=StreamSpeechModel.from_engine(hip_model),
                                                   vocoder=VocSurface(multi_voc)), cfg)
        want = _run_agent(agent, pcm)
        assert [(w, f) for w, _, f in got[s]] == [(w, f) for w, _, f in want]
        assert [len(c or []) for _, c, _ in got[s]] == [len(c or []) for _, c, _ in want]
        a = np.concatenate([np.asarray(c, np.float32) for _, c, _ in got[s] if c])
        b = np.concatenate([np.asarray(c, np.float32) for _, c, _ in want if c])
        assert a.size > 0 and float(np.sqrt(np.mean((a - b) ** 2))) < BATCH_RMS_TOL
        speech[k] = a
    assert float(np.sqrt(np.mean((speech[0] - speech[2]) ** 2))) > 0.05       # the same units in different voices
    hip_model.encoder_stream_set_tail(0)


def test_agent_with_speaker_id(hip_model, synth_weights, tmp_path):
    from streamspeech_amd import synth
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.modules import StreamSpeechModel
    cfg = synth_weights[0]
    cfg_path = tmp_path / "vocoder_cfg.json"
    cfg_path.write_text(json.dumps(MR.multispkr_config(NUM_SPEAKERS).as_dict()))
    model = StreamSpeechModel.from_engine(hip_model)
    with pytest.raises(ValueError, match="--speaker-id"):
        StreamSpeechS2STAgent(_s2st_args(("--vocoder-cfg", str(cfg_path))), model=model)
    agent = RF.set_dicts(StreamSpeechS2STAgent(_s2st_args(("--vocoder-cfg", str(cfg_path), "--speaker-id", "2")), model=model), cfg)
    assert agent.vocoder.hip.num_speakers == NUM_SPEAKERS and agent.speaker_id == 2
    recs = _run_agent(agent, synth.synth_pcm(2003, 16000 * 2))
    wav = np.concatenate([np.asarray(c, np.float32) for w, c, _ in recs if w and c])
    assert wav.size > 0 and wav.size % 320 == 0 and np.isfinite(wav).all()
    hip_model.encoder_stream_set_tail(0)
