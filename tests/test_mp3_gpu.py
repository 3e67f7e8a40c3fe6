"""GPU checks of the MP3 ingest: the device stage (csrc/mp3.hip, ss_mp3_synthesize) against the float64 restatement
tests/mp3_ref.py on the example streams and every writer stream, batch invariance, a refused file inside a batch, and the
offline driver on the example MP3s."""
import argparse
import os

import numpy as np
import pytest
import torch

import mp3_ref as R
import mp3_writer as Wr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "mp3")
EXAMPLES = ["common_voice_fr_17301936.mp3", "common_voice_fr_17767732.mp3"]
RMS_BAR = 2.0 ** -15 / np.sqrt(12.0)          # ISO/IEC 11172-4 "full accuracy" limits, here against our float64 restatement
MAX_BAR = 2.0 ** -14


def _streams():
    out = {n: open(os.path.join(GOLD, n), "rb").read() for n in EXAMPLES}
    out.update({n: v[0] for n, v in Wr.catalogue().items()})
    return out


STREAMS = _streams()


@pytest.mark.parametrize("name", sorted(STREAMS))
@pytest.mark.parametrize("mono", [True, False])
def test_device_synthesis_matches_float64_restatement(name, mono):
    from streamspeech_amd import mp3
    data = STREAMS[name]
    info, q, rec, _ = mp3.unpack(data)
    (y, sr), = mp3.decode_batch([data], "cuda:0", mono=mono)
    ref = R.synthesize(info, q, rec, mono=mono)
    got = y.cpu().numpy().astype(np.float64)
    assert sr == info["sample_rate"] and got.shape == ref.shape
    err = got - ref
    rms, mx = float(np.sqrt(np.mean(err ** 2))), float(np.abs(err).max())
    assert rms <= RMS_BAR and mx <= MAX_BAR, (name, rms, mx)


def test_batch_invariance():
    from streamspeech_amd import mp3
    names = sorted(STREAMS)
    alone = {n: mp3.decode_batch([STREAMS[n]], "cuda:0")[0][0].clone() for n in names}
    for order in (names, names[::-1]):
        got = mp3.decode_batch([STREAMS[n] for n in order], "cuda:0", threads=3)
        for n, (y, _) in zip(order, got):
            assert torch.equal(y, alone[n]), n
    # bounded groups (several ss_mp3_synthesize calls): the same bits
    got = mp3.decode_batch([STREAMS[n] for n in names], "cuda:0", max_seconds=5.0)
    for n, (y, _) in zip(names, got):
        assert torch.equal(y, alone[n]), n
    stereo = mp3.decode_batch([STREAMS["mpeg1_stereo_ms"], STREAMS[EXAMPLES[0]]], "cuda:0", mono=False)
    assert stereo[0][0].shape[0] == 2 and stereo[1][0].shape[0] == 1
    assert torch.equal((stereo[0][0][0] + stereo[0][0][1]) * 0.5, alone["mpeg1_stereo_ms"])


def test_bad_file_in_batch_names_it():
    from streamspeech_amd import lib as L, mp3
    good = STREAMS[EXAMPLES[0]]
    bad = b"ID3\x03\x00\x00\x00\x00\x7f\x7f" + good[10:3000]          # the tag claims more bytes than the file has
    with pytest.raises(L.StreamSpeechHipError) as e:
        mp3.decode_batch([good, bad, good], "cuda:0", names=["a.mp3", "broken.mp3", "c.mp3"])
    assert "broken.mp3" in str(e.value) and "a.mp3" not in str(e.value) and e.value.code == mp3.SS_ERR_BITSTREAM
    with pytest.raises(L.StreamSpeechHipError) as e:
        mp3.decode_batch([good, Wr.raw_header(layer=2) + bytes(400)], "cuda:0", names=["a.mp3", "layer2.mp3"])
    assert "layer2.mp3" in str(e.value) and e.value.code == mp3.SS_ERR_UNSUPPORTED


def test_load_audio_batch_and_read_audio():
    from streamspeech_amd import frontend
    paths = [os.path.join(GOLD, n) for n in EXAMPLES]
    got = frontend.load_audio_batch(paths, "cuda:0")
    for (y, sr), p in zip(got, paths):
        assert sr == 48000 and y.is_cuda and y.dtype == torch.float32
        x, sr2 = frontend.read_audio(p)
        assert sr2 == 48000 and x.dtype == np.float32 and np.array_equal(x, y.cpu().numpy())


def test_offline_driver_on_example_mp3s(tmp_path):
    """`python -m streamspeech_amd.offline --wav-list` over the two example MP3s: A-/S-/D- and H- lines and pred_wav dumps for
    both ids, and the ASR text equals the pipeline's on load_audio_batch tensors resampled by model.resample."""
    from streamspeech_amd import frontend, offline
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.modules import CodeHiFiGANVocoderWithDur
    paths = [os.path.join(GOLD, n) for n in EXAMPLES]
    lst = tmp_path / "wav_list.txt"
    lst.write_text("\n".join(paths) + "\n")
    res = tmp_path / "res"
    offline.main(["--wav-list", str(lst), "--path", "synthetic:0", "--vocoder", "synthetic:0", "--results-path", str(res),
                  "--device", "cuda:0"])
    log = (res / "generate-test.log").read_text().splitlines()
    assert sorted(ln.split("\t")[0] for ln in log) == sorted(f"{p}-{i}" for p in "ASD" for i in range(2))
    txt = (res / "generate-test.txt").read_text().splitlines()
    assert sorted(ln.split("\t")[0] for ln in txt) == sorted(f"{p}-{i}" for p in "HD" for i in range(2))
    assert sorted(os.listdir(res / "pred_wav")) == ["0_pred.wav", "1_pred.wav"]
    asr_main = {int(ln.split("\t")[0][2:]): ln.split("\t", 1)[1] for ln in log if ln.startswith("A-")}
    # the same model the driver loads, run on the decoded tensors directly
    ns = argparse.Namespace(config_yaml=None, multitask_config_yaml=None, data_bin=".", model_path="synthetic:0",
                            global_stats=None, source_segment_size=999999 * 40, shift_size=10, window_size=25,
                            sample_rate=16000, feature_dim=80, full_recompute_encoder=True)
    holder = argparse.Namespace(device="cuda:0")
    StreamSpeechS2STAgent.load_model_vocab(holder, ns)
    model = holder.model.hip
    voc = CodeHiFiGANVocoderWithDur("synthetic:0", None, device="cuda:0").hip
    items = [(i, model.resample(y, sr, 16000)) for i, (y, sr) in enumerate(frontend.load_audio_batch(paths, "cuda:0"))]
    hyps = offline.generate(model, voc, items, holder.dict, str(tmp_path / "direct"), "test", dur_prediction=False,
                            dump_wav=False, t2u_causal=getattr(holder.model, "uni_encoder", False))
    assert {i: hyps[i]["asr"] for i in range(2)} == asr_main


def test_streaming_agent_on_decoded_real_speech(hip_model, hip_vocoder):
    """One example clip, decoded on the device (48 kHz), through the S2ST agent's resampling front end and
    streaming_eval.run_utterance at 320 ms to the end.  Every incremental encoder call is compared with a full recompute of the
    same fbank prefix (the bar of test_stages_gpu.py's incremental-encoder tests: max |diff| < 5e-5), and the CTC ids of both
    heads of the final prefix are equal.  Traces are not compared: with random weights a near-tie may flip them."""
    from streamspeech_amd import frontend, streaming_eval
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.modules import CodeHiFiGANVocoderWithDur, StreamSpeechModel
    from tests.test_agent_cpu import make_args

    class HipVocSurface:  # CodeHiFiGANVocoderWithDur call surface over the shared fixture handle
        def __init__(self, hv):
            self.hip = hv
        __call__ = CodeHiFiGANVocoderWithDur.__call__

    (y, sr), = frontend.load_audio_batch([os.path.join(GOLD, EXAMPLES[0])], hip_model.device)
    assert sr == 48000
    pcm = y.cpu().numpy()
    agent = StreamSpeechS2STAgent(make_args(320, sample_rate=48000, full_recompute_encoder=False),
                                  model=StreamSpeechModel.from_engine(hip_model), vocoder=HipVocSurface(hip_vocoder))
    inc_fn = hip_model.encoder_stream_forward
    seen = {"calls": 0, "worst": 0.0, "last": None}

    def checked(fb, attn_chunk, conv_chunk, *a, **k):
        inc = inc_fn(fb, attn_chunk, conv_chunk, *a, **k)
        full = hip_model.encoder_forward(fb, attn_chunk, conv_chunk)
        assert inc.shape == full.shape
        err = (inc - full).abs().max().item() if inc.numel() else 0.0
        assert err < 5e-5, f"call {seen['calls']}: {err}"
        seen["calls"] += 1
        seen["worst"] = max(seen["worst"], err)
        seen["last"] = (inc.clone(), full.clone())
        return inc

    hip_model.encoder_stream_forward = checked
    try:
        agent.reset()
        r = streaming_eval.run_utterance(agent, pcm, 320, sr=48000)
    finally:
        del hip_model.encoder_stream_forward
        hip_model.encoder_stream_reset()
    step = 48000 * 320 // 1000
    assert r["calls"] == -(-len(pcm) // step) and r["source_ms"] > 4000
    assert seen["calls"] >= 10, seen["calls"]
    inc, full = seen["last"]
    for head in (0, 1):
        assert hip_model.ctc_greedy(head, inc)[0] == hip_model.ctc_greedy(head, full)[0]
    print(f"streaming on decoded speech: {r['calls']} calls, {seen['calls']} encoder calls, worst |inc - full| {seen['worst']:.2e}, "
          f"actions {r['actions']}")
