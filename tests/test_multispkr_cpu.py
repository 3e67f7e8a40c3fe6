"""Multi-speaker unit vocoder, host side: the config fields and refusals, the seeded checkpoint, the speaker table of the weight
packer against a float64 restatement of the reference's concatenated conv_pre, the exported symbols, and the --speaker-id plumbing
of the S2ST agent, the offline driver and the session pool with stub vocoders.  No GPU."""
import argparse
import hashlib
import os
import re

import numpy as np
import pytest
import torch

from streamspeech_amd import synth
from streamspeech_amd.config import VocoderConfig
from tests import multispkr_ref as MR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# sha256 over the sorted (key, bytes) pairs of synth.make_vocoder_state_dict(0) on the commit before the speaker embedding existed
SINGLE_SPEAKER_SD_SHA256 = "29ee8de667811e031d2950e3b74926bd654d3cd8c6f9faa14629345567c1a628"
SINGLE_SPEAKER_SD_KEYS = 302
NEW_SYMBOLS = ("ss_vocoder_num_speakers", "ss_vocoder_forward_spkr", "ss_batch_vocoder_forward_spkr", "ss_batch_vocoder_tail_spkr",
               "ss_op_spkr_pre_add")


@pytest.fixture(scope="module")
def multi():
    """(config, state dict, folded conv_pre weight f64, bias f64, speaker embeddings, packed slots by name)."""
    from streamspeech_amd.weights import pack_vocoder
    vcfg = MR.multispkr_config(5)
    vsd = synth.make_vocoder_state_dict(0, vcfg)
    w, b = MR.folded_pre(vsd)
    names, offsets, numels, blob = pack_vocoder(vsd, vcfg)
    slots = {n: blob[o:o + k] for n, o, k in zip(names, offsets, numels)}
    return vcfg, vsd, w, b, torch.from_numpy(vsd["spkr.weight"]), slots


def test_config_fields_and_dict():
    d = VocoderConfig().as_dict()
    assert list(d) == ["num_embeddings", "embedding_dim", "model_in_dim", "upsample_rates", "upsample_kernel_sizes",
                       "upsample_initial_channel", "resblock_kernel_sizes", "resblock_dilation_sizes", "dur_predictor_params",
                       "code_hop_size"]                                    # the single-speaker dict is what it was
    assert d["model_in_dim"] == 128 and not VocoderConfig().multispkr and VocoderConfig().num_speakers == 200
    m = MR.multispkr_config(5).as_dict()
    assert m["multispkr"] is True and m["num_speakers"] == 5 and m["model_in_dim"] == 256
    assert {k: v for k, v in m.items() if k not in ("multispkr", "num_speakers", "model_in_dim")} == \
        {k: v for k, v in d.items() if k != "model_in_dim"}


def test_config_json_round_trip_and_refusals():
    from streamspeech_amd.modules import vocoder_config_from_json
    for cfg in (VocoderConfig(), MR.multispkr_config(5), MR.multispkr_config(200)):
        assert vocoder_config_from_json(cfg.as_dict()) == cfg
    base = MR.multispkr_config(5).as_dict()
    with pytest.raises(ValueError, match="model_in_dim"):
        vocoder_config_from_json({**base, "model_in_dim": 128})            # multi-speaker needs 2 x embedding_dim
    with pytest.raises(ValueError, match="model_in_dim"):
        vocoder_config_from_json({**VocoderConfig().as_dict(), "model_in_dim": 256})
    with pytest.raises(ValueError, match="model_in_dim"):
        VocoderConfig(multispkr=True)
    with pytest.raises(ValueError, match="f0"):
        vocoder_config_from_json({**base, "f0": True})
    with pytest.raises(ValueError, match="f0_quant_num_bin"):
        vocoder_config_from_json({**base, "f0_quant_num_bin": 32})
    with pytest.raises(ValueError, match="embedder_params"):
        vocoder_config_from_json({**base, "embedder_params": {"embedder_dim": 256}})
    assert vocoder_config_from_json({**base, "f0": False, "f0_quant_num_bin": 0, "embedder_params": None}) == MR.multispkr_config(5)


def _sd_hash(sd):
    h = hashlib.sha256()
    for k in sorted(sd):
        h.update(k.encode())
        h.update(np.ascontiguousarray(sd[k]).tobytes())
    return h.hexdigest()


def test_single_speaker_state_dict_unchanged(multi):
    sd = synth.make_vocoder_state_dict(0)
    assert len(sd) == SINGLE_SPEAKER_SD_KEYS and "spkr.weight" not in sd
    assert _sd_hash(sd) == SINGLE_SPEAKER_SD_SHA256
    vcfg, vsd = multi[0], multi[1]
    assert vsd["spkr.weight"].shape == (5, vcfg.embedding_dim) and vsd["spkr.weight"].dtype == np.float32
    assert vsd["conv_pre.weight_v"].shape == (512, 256, 7)
    # name-keyed generator: every tensor whose shape does not depend on model_in_dim is the single-speaker one, bit for bit
    same = [k for k in sd if not k.startswith("conv_pre.weight")]
    assert set(vsd) == set(sd) | {"spkr.weight"} and all(np.array_equal(sd[k], vsd[k]) for k in same)


def test_packed_table_is_the_rounded_float64_sums(multi):
    vcfg, vsd, w, b, spk, slots = multi
    C0, E = vcfg.upsample_initial_channel, vcfg.embedding_dim
    tab = slots["voc.spkr.table"].reshape(5, 16, C0)
    want = MR.table64(w, spk)
    assert tab.dtype == torch.float32 and torch.equal(tab, want.float())
    # the code half keeps the tap-major layout of voc.pre.w; the fold runs over the whole [C0, 2E, 7] tensor
    from streamspeech_amd.weights import conv_tap_major
    assert torch.equal(slots["voc.pre.w"].reshape(C0, 7 * E), conv_tap_major(w[:, :E, :].float()))
    assert "voc.spkr.table" not in _single_slots()


def _single_slots():
    from streamspeech_amd.weights import pack_vocoder
    return pack_vocoder(synth.make_vocoder_state_dict(0), VocoderConfig())[0]


@pytest.mark.parametrize("L", MR.SEG_LENGTHS)
def test_split_form_equals_concatenated_form(multi, L):
    """Code-half conv + table entry == conv over [code ; speaker] in float64, within 1e-12, for every speaker."""
    vcfg, vsd, w, b, spk, _ = multi
    codes = torch.from_numpy(synth.uniform(L, "multispkr_codes", (L,), 0, vcfg.num_embeddings).astype(np.int64))
    emb = torch.from_numpy(vsd["dict.weight"])[codes]
    tab = MR.table64(w, spk)
    for s in range(spk.shape[0]):
        want = MR.concat_conv_pre(w, b, emb, spk[s])
        got = MR.split_conv_pre(w, b, emb, tab[s])
        assert want.shape == got.shape == (L, vcfg.upsample_initial_channel)
        assert float((want - got).abs().max()) < 1e-12
    assert float((MR.concat_conv_pre(w, b, emb, spk[0]) - MR.concat_conv_pre(w, b, emb, spk[2])).abs().max()) > 0.1


def test_pack_refuses_mismatched_checkpoints(multi):
    from streamspeech_amd.weights import pack_vocoder
    vcfg, vsd = multi[0], multi[1]
    with pytest.raises(ValueError):
        pack_vocoder(vsd, VocoderConfig())                                # spkr.weight without multispkr
    with pytest.raises(ValueError):
        pack_vocoder(synth.make_vocoder_state_dict(0), vcfg)              # multispkr without spkr.weight
    with pytest.raises(ValueError):
        pack_vocoder(vsd, MR.multispkr_config(7))                         # another speaker count
    with pytest.raises(ValueError, match="embedder_params"):
        pack_vocoder({**vsd, "spkr.bias": np.zeros(128, np.float32)}, vcfg)


def test_new_symbols_exported_and_prototyped():
    from streamspeech_amd import lib as L
    header = open(os.path.join(ROOT, "include", "streamspeech_hip.h")).read()
    for name in NEW_SYMBOLS:
        assert name in L.SIGNATURES, name
        assert re.search(r"\bint %s\(" % name, header), name
    lib = L.load()                                                        # dlopen binds every declared symbol or raises
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name)
    assert lib.ss_vocoder_num_speakers(None) == 0
    # the _spkr forms are the existing argument lists plus the speaker(s)
    for old, new in (("ss_vocoder_forward", "ss_vocoder_forward_spkr"), ("ss_batch_vocoder_forward", "ss_batch_vocoder_forward_spkr"),
                     ("ss_batch_vocoder_tail", "ss_batch_vocoder_tail_spkr")):
        assert L.SIGNATURES[new][1][:-1] == L.SIGNATURES[old][1] and len(L.SIGNATURES[new][1]) == len(L.SIGNATURES[old][1]) + 1


# ---- flag plumbing with stub vocoders -------------------------------------------------------------------------------------------
class _StubVoc:
    """CodeHiFiGANVocoderWithDur call surface that records what it is asked; num_speakers as HipVocoder reports it."""

    def __init__(self, num_speakers):
        self.num_speakers = num_speakers
        self.cfg = VocoderConfig()
        self.calls = []

    def __call__(self, x, dur_prediction=False):
        self.calls.append({k: v.clone() for k, v in x.items()})
        K = x["code"].numel()
        return torch.zeros(K * 320), torch.ones((1, K), dtype=torch.long)

    def batch_forward(self, codes, dur_prediction=True, **kw):
        self.calls.append(("batch_forward", [list(c) for c in codes], kw))
        return [torch.zeros(len(c) * 320) for c in codes], None, [len(c) for c in codes]

    def batch_tail(self, codes, n_new, ctx, rf, dur_prediction=True, **kw):
        self.calls.append(("batch_tail", [list(c) for c in codes], kw))
        return [torch.zeros(n * 320) for n in n_new], [(0, [1] * len(c)) for c in codes]


def _agent_args(extra=(), segment_ms=320):
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    p = argparse.ArgumentParser()
    StreamSpeechS2STAgent.add_args(p)
    a = p.parse_args(["--model-path", "synthetic:0", "--data-bin", "/nonexistent", "--vocoder", "synthetic:0", "--dur-prediction",
                      "--sample-rate", "16000", *extra])
    a.source_segment_size, a.device = segment_ms, "cpu"
    return a


def test_synthesize_tail_passes_the_speaker_on_both_calls():
    from streamspeech_amd.agent import synthesize_tail
    v = _StubVoc(5)
    units = list(range(40))
    synthesize_tail(v, units, 2, True, ctx=10, rf=200, spkr=3)            # window first, then (durations of 1 < rf) all units
    assert len(v.calls) == 2 and [c["code"].numel() for c in v.calls] == [12, 40]
    for c in v.calls:
        assert c["spkr"].dtype == torch.long and c["spkr"].tolist() == [[3]]
    v.calls.clear()
    synthesize_tail(v, units, 2, True, ctx=10, rf=200)
    assert all("spkr" not in c for c in v.calls)


def test_agent_flag(synth_weights):
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.modules import StreamSpeechModel
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from tests.oracle_engine import OracleEngine
    cfg, _, sd, _ = synth_weights
    assert _agent_args().speaker_id is None and _agent_args(["--speaker-id", "2"]).speaker_id == 2
    model = StreamSpeechModel.from_engine(OracleEngine(sd, cfg))
    with pytest.raises(ValueError, match="--speaker-id"):                 # required on a multi-speaker vocoder, at construction
        StreamSpeechS2STAgent(_agent_args(), model=model, vocoder=_StubVoc(5))
    with pytest.raises(ValueError, match="--speaker-id"):
        StreamSpeechS2STAgent(_agent_args(["--speaker-id", "5"]), model=model, vocoder=_StubVoc(5))
    assert StreamSpeechS2STAgent(_agent_args(["--speaker-id", "7"]), model=model, vocoder=_StubVoc(0)).speaker_id is None   # ignored
    voc = _StubVoc(5)
    agent = StreamSpeechS2STAgent(_agent_args(["--speaker-id", "2"]), model=model, vocoder=voc)
    assert agent.speaker_id == 2
    pcm = synth.synth_pcm(3, 16000 * 2)
    for pos in range(0, len(pcm), 5120):
        agent.pushpop(SpeechSegment(content=pcm[pos:pos + 5120].tolist(), sample_rate=16000, finished=pos + 5120 >= len(pcm)))
    assert voc.calls and all(c["spkr"].tolist() == [[2]] for c in voc.calls)


def test_vocoder_class_reads_spkr():
    from streamspeech_amd.modules import CodeHiFiGANVocoderWithDur

    class Hip:
        def __init__(self, n):
            self.num_speakers, self.seen = n, []

        def forward(self, code, dur_prediction, speaker=None):
            self.seen.append(speaker)
            return torch.zeros(code.numel() * 320), torch.ones(code.numel(), dtype=torch.int32)

    v = CodeHiFiGANVocoderWithDur.__new__(CodeHiFiGANVocoderWithDur)
    v.hip = Hip(5)
    x = {"code": torch.tensor([[4, 5, -1]]), "spkr": torch.tensor([[3]])}
    wav, dur = v(x, True)
    assert v.hip.seen == [3] and dur.shape == (1, 2)
    with pytest.raises(AssertionError, match="spkr"):
        v({"code": torch.tensor([[4, 5]])}, True)
    v.hip = Hip(0)                                                        # single-speaker: the key is ignored (codehifigan.py:88-90)
    v(x, True)
    assert v.hip.seen == [None]


class _OffModel:
    """The offline driver's model calls, canned: two utterances, three and zero units."""
    class cfg:
        max_target_positions, eos = 1024, 2

    def batch_fbank_cmvn(self, pcm, n):
        return None, [10] * len(n)

    def batch_encoder_forward(self, feat, T):
        return None, [3] * len(T)

    def batch_ctc_greedy(self, head, enc, Tp):
        return [([], None)] * len(Tp)

    def batch_mt_greedy(self, enc, Tp, mx):
        return [[2]] * len(Tp), None, [1] * len(Tp)

    def batch_t2u_units(self, feats, n, t2u_causal=False, mask_eos=True):
        return [[4 + 7, 4 + 8, 4 + 9] for _ in n]


def test_offline_driver_flag(tmp_path, monkeypatch):
    from streamspeech_amd import offline
    from streamspeech_amd.modules import Dictionary
    assert offline.build_parser().parse_args(["--path", "p", "--vocoder", "v", "--results-path", "r"]).speaker_id == -1
    monkeypatch.setattr(offline, "units_from_tokens", lambda t, cfg: [c - 4 for c in t])
    d = Dictionary.placeholder(20)
    dicts = {"source_unigram": d, "ctc_target_unigram": d, "target_unigram": d}
    items = [(i, torch.zeros(800 + i)) for i in range(3)]
    voc = _StubVoc(5)
    offline.generate(_OffModel(), voc, items, dicts, str(tmp_path / "a"), speaker_id=3)
    assert [c[2] for c in voc.calls] == [{"speakers": [3, 3, 3]}]         # one batch_forward per batch, a voice per row
    voc.calls.clear()
    import random
    random.seed(1)
    offline.generate(_OffModel(), voc, items, dicts, str(tmp_path / "b"))  # -1: a random speaker per utterance, logged
    drawn = voc.calls[0][2]["speakers"]
    assert len(voc.calls) == 1 and len(drawn) == 3 and all(0 <= s < 5 for s in drawn)
    log = open(tmp_path / "b" / "generate-test.log").read().splitlines()
    order = [int(ln.split("\t")[0][2:]) for ln in log if ln.startswith("A-")]
    assert {int(ln.split("\t")[0][2:]): int(ln.split("\t")[1]) for ln in log if ln.startswith("K-")} == dict(zip(order, drawn))
    with pytest.raises(ValueError, match="--speaker-id"):
        offline.generate(_OffModel(), voc, items, dicts, str(tmp_path / "c"), speaker_id=5)
    single = _StubVoc(0)
    offline.generate(_OffModel(), single, items, dicts, str(tmp_path / "d"), speaker_id=3)
    assert [c[2] for c in single.calls] == [{}]                           # a single-speaker vocoder is called as before


def test_pool_open_takes_and_refuses_the_voice():
    from streamspeech_amd.speech_pool import SpeechSessionPool
    from tests.test_speech_pool_cpu import _StubEngine, _dicts
    pool = SpeechSessionPool(_StubEngine(), 4, 64, vocoder=_StubVoc(5))
    with pytest.raises(ValueError, match="speaker"):                      # at open(), not at the first write
        pool.open("s2st", _agent_args(), dicts=_dicts())
    with pytest.raises(ValueError, match="speaker"):
        pool.open("s2st", _agent_args(["--speaker-id", "9"]), dicts=_dicts())
    assert pool.sessions == {}
    sids = [pool.open("s2st", _agent_args(["--speaker-id", str(k)]), dicts=_dicts()) for k in (0, 4)]
    assert [pool.sessions[s].speaker_id for s in sids] == [0, 4]
    pool.open("s2tt", _agent_args(), dicts=_dicts())                      # text sessions have no voice
    single = SpeechSessionPool(_StubEngine(), 2, 64, vocoder=_StubVoc(0))
    assert single.sessions[single.open("s2st", _agent_args(["--speaker-id", "3"]), dicts=_dicts())].speaker_id is None
