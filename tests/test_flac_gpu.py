"""GPU checks of the FLAC ingest: the device stage (csrc/flac.hip, ss_flac_restore) against its host twin bit for bit and against
the integers tests/flac_writer.py encoded, over the grid of tests/flac_cases.py; batch invariance; a refused file inside a batch;
the libFLAC fixture through load_audio_batch against read_wav; and the offline driver on a manifest of stored-zip FLAC cells
against the same audio as WAV files."""
import hashlib
import json
import os
import wave

import numpy as np
import pytest
import torch

import flac_cases as Cases
import flac_writer as W
from test_flac_cpu import stored_zip

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "flac")
FACTS = json.load(open(os.path.join(GOLD, "fixtures.json")))
DEV = "cuda:0"


def _fixture():
    return open(os.path.join(GOLD, FACTS["file"]), "rb").read()


@pytest.mark.parametrize("name", sorted(Cases.catalogue()))
def test_device_restore_is_exact(name):
    """ss_flac_restore == the writer's integers * 2^-(bps-1) == ss_flac_restore_host, planar and mono."""
    from streamspeech_amd import flac
    data, chans, bps, sr = Cases.catalogue()[name]
    part = flac.unpack(data)
    want = np.asarray(chans, np.int64).astype(np.float32) * np.float32(2.0 ** -(bps - 1))
    (y, got_sr), = flac.decode_batch([data], DEV, mono=False, route="device")
    assert got_sr == sr and y.shape == want.shape and y.dtype == torch.float32
    assert np.array_equal(y.cpu().numpy(), want), name
    assert np.array_equal(y.cpu().numpy(), flac.restore_host([part], mono=False)[0])
    (m, _), = flac.decode_batch([data], DEV, mono=True, route="device")
    assert m.shape == (len(chans[0]),) and np.array_equal(m.cpu().numpy(), flac.restore_host([part], mono=True)[0]), name
    (h, _), = flac.decode_batch([data], DEV, mono=True, route="host")
    assert torch.equal(h, m)


def test_wide_accumulator_case_needs_64_bits():
    """The 24-bit, order-32, precision-15 stream is one that a 32-bit accumulator gets wrong: restated with wrapping int32 sums it
    differs from the truth, so the exact device result above shows the 64-bit path was taken."""
    from streamspeech_amd import flac
    data, chans, bps, _ = Cases.catalogue()["wide_accumulator"]
    _, res, rec = flac.unpack(data)
    r = rec[0]
    assert r["order"] == 32 and r["precision"] == 15 and int(r["bps"]) + 15 + 5 > 32
    s = res[:192].astype(np.int64).tolist()
    coef = r["coef"].astype(np.int64).tolist()
    for i in range(32, 192):
        acc = sum(coef[j] * s[i - 1 - j] for j in range(32))
        acc32 = ((acc + (1 << 31)) % (1 << 32)) - (1 << 31)
        assert acc32 != acc
        s[i] = s[i] + (acc32 >> int(r["shift"]))
    assert s != chans[0][:192]


def test_pack_of_everything_equals_host_twin():
    """The whole grid and the libFLAC fixture as ONE ragged pack (mixed channel counts, depths and block sizes): each file's bits
    are those of the host twin, planar and mono."""
    from streamspeech_amd import flac
    names = sorted(Cases.catalogue())
    blobs = [Cases.catalogue()[n][0] for n in names] + [_fixture()]
    parts = [flac.unpack(b) for b in blobs]
    for mono in (False, True):
        host = flac.restore_host(parts, mono=mono)
        dev = flac.restore_device(parts, DEV, mono=mono)
        for n, a, b in zip(names + ["fixture"], host, dev):
            assert np.array_equal(a, b.cpu().numpy()), (n, mono)
    ints = (dev[-1].cpu().numpy() * 32768.0).astype("<i2")
    assert hashlib.md5(ints.tobytes()).hexdigest() == FACTS["prefix_pcm_md5"]


def test_batch_invariance():
    from streamspeech_amd import flac
    names = ["stereo_ms_b24_wasted", "variable", "three_channels"]
    blobs = [Cases.catalogue()[n][0] for n in names]
    alone = [flac.decode_batch([b], DEV, mono=False)[0][0].clone() for b in blobs]
    for order in ([0, 1, 2], [2, 0, 1]):
        got = flac.decode_batch([blobs[i] for i in order], DEV, mono=False, threads=3)
        for i, (y, _) in zip(order, got):
            assert torch.equal(y, alone[i]), names[i]
    got = flac.decode_batch(blobs, DEV, mono=False, max_seconds=0.01)            # one group per file
    for i, (y, _) in enumerate(got):
        assert torch.equal(y, alone[i])
    got = flac.decode_batch(blobs, DEV, mono=True)
    for i, (y, _) in enumerate(got):
        ref = alone[i][0]
        for c in range(1, alone[i].shape[0]):
            ref = ref + alone[i][c]
        assert torch.equal(y, ref * np.float32(1.0 / alone[i].shape[0]))


def test_bad_file_in_batch_names_it():
    from streamspeech_amd import flac, lib as L
    good = Cases.catalogue()["block192"][0]
    bad = bytearray(good)
    bad[60] ^= 0x04                                                               # a flipped bit in the first frame's body
    with pytest.raises(L.StreamSpeechHipError) as e:
        flac.decode_batch([good, bytes(bad), good], DEV, names=["a.flac", "broken.flac", "c.flac"])
    assert "broken.flac" in str(e.value) and "a.flac" not in str(e.value) and e.value.code == flac.SS_ERR_BITSTREAM
    with pytest.raises(flac.FlacError) as e:
        flac.decode_batch([good, b"OggS" + bytes(100)], DEV, names=["a.flac", "ogg.flac"])
    assert "ogg.flac" in str(e.value) and e.value.code == flac.SS_ERR_UNSUPPORTED


def test_restore_refusals():
    from streamspeech_amd import flac, lib as L
    lib = L.load()
    import ctypes as C
    wb = C.c_size_t(0)
    files = np.zeros(1, flac.FILE_DTYPE)
    files[0] = (0, 0, 1, 9, 16, 10)
    assert lib.ss_flac_restore(None, None, None, 9, 10, files.ctypes.data, 1, 1, None, 10, None, C.byref(wb)) == L.SS_ERR_ARG
    files[0] = (0, 0, 1, 1, 32, 10)
    assert lib.ss_flac_restore(None, None, None, 1, 10, files.ctypes.data, 1, 1, None, 10, None, C.byref(wb)) == L.SS_ERR_ARG
    files[0] = (0, 0, 2, 1, 16, 10)
    assert lib.ss_flac_restore(None, None, None, 1, 10, files.ctypes.data, 1, 1, None, 10, None, C.byref(wb)) == L.SS_ERR_ARG
    files[0] = (0, 0, 1, 1, 16, 10)
    assert lib.ss_flac_restore(None, None, None, 1, 10, files.ctypes.data, 1, 1, None, 9, None, C.byref(wb)) == L.SS_ERR_CAPACITY
    assert lib.ss_flac_restore(None, None, None, 1, 10, files.ctypes.data, 1, 1, None, 10, None, C.byref(wb)) == 0
    assert wb.value >= 40
    # a record that does not fit its file is not followed: the frame writes nothing, its neighbour does
    data, chans, _, _ = Cases.catalogue()["block192"]
    info, res, rec = flac.unpack(data)
    rec = rec.copy()
    rec["sample_start"][1] = info["samples"] - 10
    out = flac.restore_device([(info, res, rec)], DEV, mono=True)[0].cpu().numpy()
    assert np.array_equal(out[:192], np.asarray(chans[0][:192], np.float32) / 32768.0)
    assert np.array_equal(out[384:], np.asarray(chans[0][384:], np.float32) / 32768.0)


def _wav(path, x, sr=16000):
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes(np.asarray(x, "<i2").tobytes())


def test_fixture_through_load_audio_batch_equals_read_wav(tmp_path):
    from streamspeech_amd import flac, frontend
    data = _fixture()
    ints = flac.restore_host([flac.unpack(data)], False, True)[1][0][0]
    _wav(tmp_path / "same.wav", ints)
    (tmp_path / "clip.flac").write_bytes(data)
    x, sr = frontend.read_wav(str(tmp_path / "same.wav"))
    (y, sr2), (z, sr3) = frontend.load_audio_batch([str(tmp_path / "clip.flac"), str(tmp_path / "same.wav")], DEV)
    assert sr == sr2 == sr3 == 16000 and y.is_cuda and y.dtype == torch.float32
    assert np.array_equal(y.cpu().numpy(), x) and np.array_equal(z.cpu().numpy(), x)
    a, sr4 = frontend.read_audio(str(tmp_path / "clip.flac"))
    assert sr4 == 16000 and a.dtype == np.float32 and np.array_equal(a, x)
    # a stereo stream: the channel mean, read_wav's bits
    l, r = Cases.catalogue()["stereo_switching"][1]
    with wave.open(str(tmp_path / "st.wav"), "wb") as w:
        w.setnchannels(2); w.setsampwidth(2); w.setframerate(16000)
        w.writeframes(np.asarray([l, r], "<i2").T.copy().tobytes())
    (tmp_path / "st.flac").write_bytes(Cases.catalogue()["stereo_switching"][0])
    xs, _ = frontend.read_wav(str(tmp_path / "st.wav"))
    (ys, _), = frontend.load_audio_batch([str(tmp_path / "st.flac")], DEV)
    assert np.array_equal(ys.cpu().numpy(), xs)


def _tree(root):
    out = {}
    for d, _, fs in os.walk(root):
        for f in fs:
            out[os.path.relpath(os.path.join(d, f), root)] = open(os.path.join(d, f), "rb").read()
    return out


def test_offline_driver_on_stored_zip_flac_manifest(tmp_path):
    """`python -m streamspeech_amd.offline DATA` on a manifest whose src_audio cells point into a stored zip of FLAC members (the
    recipe's --use-audio-input layout) writes the files it writes for the same audio given as WAV paths, byte for byte."""
    from streamspeech_amd import offline, synth
    clips = {f"utt{k}": np.round(synth.synth_pcm(40 + k, n) * 32767.0).astype(np.int16) for k, n in enumerate((9000, 16000, 12345))}
    data = tmp_path / "data"
    data.mkdir()
    members = {}
    for name, x in clips.items():
        members[name + ".flac"] = W.encode([x.tolist()], 16, 16000, (4096,), spec=dict(kind="fixed", order=1, method=1))
        _wav(data / (name + ".wav"), x)
    cells = stored_zip(str(data / "src_flac.zip"), members)
    n_frames = {name: len(x) for name, x in clips.items()}
    for sub, cell_of in (("test", lambda n: cells[n + ".flac"]), ("testwav", lambda n: str(data / (n + ".wav")))):
        with open(data / (sub + ".tsv"), "w") as f:
            f.write("id\tsrc_audio\tsrc_n_frames\ttgt_audio\ttgt_n_frames\n")
            for name in clips:
                f.write(f"{name}\t{cell_of(name)}\t{n_frames[name]}\t1 2 3\t3\n")
    common = ["--path", "synthetic:0", "--vocoder", "synthetic:0", "--device", DEV, "--dur-prediction"]
    offline.main([str(data), "--gen-subset", "test", "--results-path", str(tmp_path / "flac")] + common)
    offline.main([str(data), "--gen-subset", "testwav", "--results-path", str(tmp_path / "wav")] + common)
    a, b = _tree(tmp_path / "flac"), _tree(tmp_path / "wav")
    assert sorted(k.replace("testwav", "test") for k in b) == sorted(a)
    assert sorted(os.listdir(tmp_path / "flac" / "pred_wav")) == ["0_pred.wav", "1_pred.wav", "2_pred.wav"]
    for k in a:
        assert a[k] == b[k.replace("generate-test", "generate-testwav")], k
    assert len((tmp_path / "flac" / "generate-test.txt").read_text().splitlines()) == 9          # T-, H-, D- per utterance
