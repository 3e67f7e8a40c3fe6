"""GPU checks of the precomputed-feature route (the recipe's src_fbank80.zip): ss_batch_cmvn against numpy, and the offline driver
on a manifest of `.npy` stored-zip cells against the PCM route of the same model, byte for byte."""
import io
import os
import wave

import numpy as np
import pytest
import torch

from test_flac_cpu import stored_zip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = os.path.join(ROOT, "tests", "golden", "gcmvn_fr-en.npz")
DEV = "cuda:0"
FRAMES = (1, 57, 131, 90)                              # T = 1, and a ragged pack


def _samples(T):
    return 400 + 160 * (T - 1)


def _clips():
    from streamspeech_amd import synth
    return {f"utt{k}": np.round(synth.synth_pcm(70 + k, _samples(T)) * 32767.0).astype(np.int16) for k, T in enumerate(FRAMES)}


@pytest.fixture(scope="module")
def plain_model(synth_weights):
    """The synthetic checkpoint WITHOUT CMVN statistics: its fbank rows are the raw log-mel values, (lg - 0) / 1."""
    from streamspeech_amd.engine import HipModel
    cfg, _, sd, _ = synth_weights
    return HipModel(sd, cfg)


def test_batch_cmvn_is_numpy_float32(hip_model, plain_model):
    g = np.load(STATS)
    mean, std = g["mean"].astype(np.float32), g["std"].astype(np.float32)
    rng = np.random.default_rng(5)
    for rows in (1, 3, 57 + 131 + 90, 4097):
        x = (rng.standard_normal((rows, 80)) * 4.0 + 5.0).astype(np.float32)
        x[0, :4] = [0.0, -0.0, np.float32(-15.9424), np.finfo(np.float32).tiny]
        got = hip_model.batch_cmvn(torch.from_numpy(x).to(DEV)).cpu().numpy()
        assert got.dtype == np.float32 and np.array_equal(got, (x - mean) / std), rows
        assert np.array_equal(plain_model.batch_cmvn(torch.from_numpy(x).to(DEV)).cpu().numpy(), x)      # no stats: (x - 0) / 1
    assert hip_model.batch_cmvn(torch.empty((0, 80), device=DEV)).shape == (0, 80)
    with pytest.raises(ValueError):
        hip_model.batch_cmvn(torch.zeros((4, 40), device=DEV))


def test_cmvn_of_raw_rows_is_the_fused_front_end(hip_model, plain_model):
    """Raw rows from the stats-less model, normalised by ss_batch_cmvn of the model with stats == that model's fused fbank + CMVN."""
    clips = _clips()
    pcm = torch.cat([torch.from_numpy(x.astype(np.float32) / 32768.0) for x in clips.values()]).to(DEV)
    n = [len(x) for x in clips.values()]
    raw, T = plain_model.batch_fbank_cmvn(pcm, n)
    fused, T2 = hip_model.batch_fbank_cmvn(pcm, n)
    assert T == T2 == list(FRAMES)
    assert torch.equal(hip_model.batch_cmvn(raw), fused)


def _wav(path, x):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(np.asarray(x, "<i2").tobytes())


def _tree(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            out[os.path.relpath(os.path.join(d, f), root)] = open(os.path.join(d, f), "rb").read()
    return out


def _data_root(tmp_path, plain_model):
    clips = _clips()
    data = tmp_path / "data"
    data.mkdir()
    members = {}
    for name, x in clips.items():
        _wav(data / (name + ".wav"), x)
        raw, _ = plain_model.batch_fbank_cmvn(torch.from_numpy(x.astype(np.float32) / 32768.0).to(DEV), [len(x)])
        bio = io.BytesIO()
        np.save(bio, raw.cpu().numpy())
        members[name + ".npy"] = bio.getvalue()
    cells = stored_zip(str(data / "src_fbank80.zip"), members)
    (data / "config_gcmvn.yaml").write_text(
        "global_cmvn:\n  stats_npz_path: %s\ninput_channels: 1\ninput_feat_per_channel: 80\n"
        "transforms:\n  '*':\n  - global_cmvn\n  _train:\n  - global_cmvn\n  - specaugment\nvocoder:\n  type: code_hifigan\n" % STATS)

    def manifest(sub, cell_of):
        with open(data / (sub + ".tsv"), "w") as f:
            f.write("id\tsrc_audio\tsrc_n_frames\ttgt_audio\ttgt_n_frames\n")
            for name, x in clips.items():
                f.write(f"{name}\t{cell_of(name)}\t{len(x)}\t4 5\t2\n")
    manifest("test", lambda n: cells[n + ".npy"])
    manifest("testwav", lambda n: str(data / (n + ".wav")))
    return data, clips, cells


def test_offline_driver_feature_cells_equal_the_pcm_route(tmp_path, plain_model):
    from streamspeech_amd import offline
    data, clips, cells = _data_root(tmp_path, plain_model)
    common = ["--path", "synthetic:0", "--vocoder", "synthetic:0", "--device", DEV, "--config-yaml", "config_gcmvn.yaml",
              "--dur-prediction"]
    offline.main([str(data), "--gen-subset", "test", "--results-path", str(tmp_path / "feat")] + common)
    offline.main([str(data), "--gen-subset", "testwav", "--results-path", str(tmp_path / "pcm")] + common)
    a, b = _tree(tmp_path / "feat"), _tree(tmp_path / "pcm")
    assert sorted(k.replace("testwav", "test") for k in b) == sorted(a) and "generate-test.unit" in a
    for k in a:
        assert a[k] == b[k.replace("generate-test", "generate-testwav")], k
    log = (tmp_path / "feat" / "generate-test.log").read_text().splitlines()
    assert sorted(ln.split("\t")[0] for ln in log) == sorted(f"{p}-{i}" for p in "ASD" for i in range(len(FRAMES)))
    # a manifest that mixes the two kinds is refused, naming the row
    with open(data / "mixed.tsv", "w") as f:
        f.write("id\tsrc_audio\n")
        f.write(f"utt0\t{cells['utt0.npy']}\n")
        f.write(f"utt1\t{data / 'utt1.wav'}\n")
    with pytest.raises(ValueError, match="mixes precomputed feature rows and audio rows"):
        offline.main([str(data), "--gen-subset", "mixed", "--results-path", str(tmp_path / "mixed")] + common)
    # a plain .npy path is a feature row as well
    from streamspeech_amd import frontend
    np.save(data / "utt2.npy", np.load(io.BytesIO(frontend.read_cell_bytes(cells["utt2.npy"]))))
    with open(data / "plain.tsv", "w") as f:
        f.write("id\tsrc_audio\n")
        f.write(f"utt2\t{data / 'utt2.npy'}\n")
    offline.main([str(data), "--gen-subset", "plain", "--results-path", str(tmp_path / "plain"), "--no-wav"] + common)
    txt = (tmp_path / "plain" / "generate-plain.txt").read_text().splitlines()
    assert [ln.split("\t")[0] for ln in txt] == ["H-0", "D-0"]


def test_generate_feature_items_keyword(hip_model, hip_vocoder, plain_model, tmp_path):
    """offline.generate(features=True) on (id, [T, 80]) items == generate on the PCM the rows were made from; the PCM call
    signature is unchanged."""
    from streamspeech_amd import offline
    from ref_fixtures import dictionaries
    clips = _clips()
    dicts = dictionaries(hip_model.cfg)
    pcm_items = [(k, torch.from_numpy(x.astype(np.float32) / 32768.0).to(DEV)) for k, x in enumerate(clips.values())]
    feat_items = [(k, plain_model.batch_fbank_cmvn(p, [p.numel()])[0]) for k, p in pcm_items]
    h_pcm = offline.generate(hip_model, hip_vocoder, pcm_items, dicts, str(tmp_path / "pcm"), "test")
    h_feat = offline.generate(hip_model, hip_vocoder, feat_items, dicts, str(tmp_path / "feat"), "test", features=True)
    assert _tree(tmp_path / "pcm") == _tree(tmp_path / "feat")
    for k in h_pcm:
        assert h_pcm[k]["units"] == h_feat[k]["units"] and h_pcm[k]["asr"] == h_feat[k]["asr"]
    with pytest.raises(ValueError, match="float32"):
        offline.generate(hip_model, hip_vocoder, [(0, torch.zeros((5, 40), device=DEV))], dicts, str(tmp_path / "bad"), "test", features=True)
