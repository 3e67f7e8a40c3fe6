"""CPU checks of the FLAC ingest: the host stage (csrc/flac_host.hip via ss_flac_probe / ss_flac_unpack) and the host twin of the
device stage (ss_flac_restore_host) against a real libFLAC stream whose STREAMINFO carries the MD5 of its PCM, against the
independent decoder tests/flac_ref.py, and against the integers tests/flac_writer.py encoded; every refusal; truncations and bit
flips; the stored-zip manifest cells and the refused feature transforms.  No GPU work is issued here (the device stage:
tests/test_flac_gpu.py)."""
import ctypes as C
import hashlib
import io
import json
import os
import re
import wave
import zipfile

import numpy as np
import pytest

import flac_cases as Cases
import flac_ref as R
import flac_writer as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "flac")
FACTS = json.load(open(os.path.join(GOLD, "fixtures.json")))
REF_FLAC = os.path.join("/root/reference", FACTS["source"])
NEW_SYMBOLS = {"ss_flac_streaminfo": 3, "ss_flac_probe": 3, "ss_flac_unpack": 7, "ss_flac_restore_host": 8, "ss_flac_restore": 12,
               "ss_batch_cmvn": 5}
OK, BITSTREAM, UNSUPPORTED = 0, 6, 7


def _flac():
    from streamspeech_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    L.load()
    from streamspeech_amd import flac
    return flac


def _fixture():
    return open(os.path.join(GOLD, FACTS["file"]), "rb").read()


def _decode_ints(data):
    """unpack + ss_flac_restore_host -> (info, int32 [channels, n], float32 [channels, n])."""
    flac = _flac()
    part = flac.unpack(data)
    floats, ints = flac.restore_host([part], mono=False, want_pcm=True)
    return part[0], ints[0], floats[0]


def _code(data, call="probe"):
    flac = _flac()
    try:
        getattr(flac, call)(data)
        return OK
    except flac.FlacError as e:
        return e.code


def test_symbols_exported_and_prototyped():
    from streamspeech_amd import lib as L
    _flac()
    header = open(os.path.join(ROOT, "include", "streamspeech_hip.h")).read()
    lib = L.load()
    for name, nargs in NEW_SYMBOLS.items():
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs, name
        assert hasattr(lib, name)
    assert re.search(r"#define\s+SS_ABI_VERSION\s+2\b", header) and lib.ss_abi_version() == 2
    flac = _flac()
    for name, size in (("ss_flac_info", 64), ("ss_flac_subframe", 96), ("ss_flac_file", 32)):
        assert re.search(r"\}\s*%s;\s*/\*\s*%d bytes" % (name, size), header), name
    assert C.sizeof(flac.FlacInfo) == 64 and flac.SUBFRAME_DTYPE.itemsize == 96 and flac.FILE_DTYPE.itemsize == 32
    build = open(os.path.join(ROOT, "streamspeech_amd", "csrc", "build.sh")).read()
    assert " flac_host " in build and " flac " in build


@pytest.mark.skipif(not os.path.exists(REF_FLAC), reason="the reference tree is not present")
def test_full_libflac_stream_matches_its_streaminfo_md5():
    """The whole 190,800-sample libFLAC 1.2.1 stream: the PCM of unpack + ss_flac_restore_host, and of flac_ref, hash to the MD5 the
    encoder wrote into STREAMINFO."""
    data = open(REF_FLAC, "rb").read()
    assert len(data) == FACTS["source_bytes"]
    flac = _flac()
    info, ints, floats = _decode_ints(data)
    assert info["md5"] == FACTS["streaminfo_md5"] == "4f344650b19e18584ca3db4df9c1279a"
    assert (info["sample_rate"], info["channels"], info["bits_per_sample"]) == (16000, 1, 16)
    assert info["frames"] == FACTS["source_frames"] and info["samples"] == info["total_samples"] == 190800
    assert hashlib.md5(flac.pcm_bytes(ints, 16)).hexdigest() == info["md5"]
    facts, chans = R.decode(data)
    assert W.pcm_md5(chans, 16).hex() == info["md5"] and facts["frames"] == info["frames"]
    assert np.array_equal(floats[0], np.asarray(chans[0], np.int16).astype(np.float32) / 32768.0)
    # the committed fixture is a prefix of this stream, cut at a frame boundary
    assert data[:FACTS["bytes"]] == _fixture()


def test_fixture_decodes_to_the_recorded_prefix_md5():
    """The committed prefix (16 frames, 65,536 samples; STREAMINFO still declares 190,800): fewer frames than declared are accepted,
    the counted samples win, and both decoders give the PCM whose MD5 was recorded after the full decode had matched STREAMINFO."""
    flac = _flac()
    data = _fixture()
    assert len(data) == FACTS["bytes"]
    info, ints, floats = _decode_ints(data)
    assert info["frames"] == FACTS["frames"] == 16 and info["samples"] == FACTS["samples"] == 65536
    assert info["total_samples"] == FACTS["total_samples"] == 190800 and info["md5"] == FACTS["streaminfo_md5"]
    assert info["min_block"] == info["max_block"] == FACTS["block_size"] == 4096
    assert hashlib.md5(flac.pcm_bytes(ints, 16)).hexdigest() == FACTS["prefix_pcm_md5"]
    facts, chans = R.decode(data)
    assert W.pcm_md5(chans, 16).hex() == FACTS["prefix_pcm_md5"] and len(chans[0]) == 65536
    assert flac.probe(data) == info and flac.streaminfo(data)["total_samples"] == 190800
    mono = flac.restore_host([flac.unpack(data)], mono=True)[0]
    assert mono.dtype == np.float32 and np.array_equal(mono, ints[0].astype(np.float32) * np.float32(2.0 ** -15))


@pytest.mark.parametrize("name", sorted(Cases.catalogue()))
def test_writer_streams_come_back_exactly(name):
    """writer -> unpack + restore_host returns the integers that went in, and their floats are s * 2^-(bps-1); the independent
    decoder agrees, and so does the MD5 the writer put into STREAMINFO."""
    flac = _flac()
    data, chans, bps, sr = Cases.catalogue()[name]
    want = np.asarray(chans, np.int64)
    info, ints, floats = _decode_ints(data)
    assert (info["sample_rate"], info["channels"], info["bits_per_sample"], info["samples"]) == (sr, len(chans), bps, len(chans[0]))
    assert np.array_equal(ints.astype(np.int64), want), name
    assert np.array_equal(floats, want.astype(np.float32) * np.float32(2.0 ** -(bps - 1)))
    assert hashlib.md5(flac.pcm_bytes(ints, bps)).hexdigest() == info["md5"]
    if len(chans[0]) <= 6000:
        assert R.decode(data)[1] == chans
    mono = flac.restore_host([flac.unpack(data)], mono=True)[0]
    acc = floats[0].copy()
    for c in range(1, len(chans)):
        acc = acc + floats[c]
    assert np.array_equal(mono, acc * np.float32(1.0 / len(chans)) if len(chans) > 1 else acc)


def test_records_say_what_the_writer_chose():
    flac = _flac()
    _, _, rec = flac.unpack(Cases.catalogue()["types"][0])
    assert rec["type"].tolist() == [flac.CONSTANT, flac.VERBATIM] + [flac.FIXED] * 5
    assert rec["order"].tolist() == [0, 0, 0, 1, 2, 3, 4] and rec["block_size"].tolist() == [192] * 7
    assert rec["coef"][6][:5].tolist() == [4, -6, 4, -1, 0] and rec["sample_start"].tolist() == [192 * k for k in range(7)]
    _, res, rec = flac.unpack(Cases.catalogue()["stereo_ms_b24_wasted"][0])
    assert rec["assignment"].tolist() == [flac.MID_SIDE] * 4 and rec["channel"].tolist() == [0, 1, 0, 1]
    assert rec["bps"].tolist() == [24, 25, 24, 25] and rec["wasted"].tolist() == [3, 0, 3, 0]
    assert rec["type"].tolist() == [flac.LPC] * 4 and rec["shift"].tolist() == [9] * 4 and rec["precision"].tolist() == [12] * 4
    assert rec["res_offset"].tolist() == [0, 192, 384, 492] and len(res) == 600
    _, _, rec = flac.unpack(Cases.catalogue()["variable"][0])
    assert rec["block_size"].tolist() == [16, 17, 192, 1000, 4096, 1] and rec["sample_start"].tolist() == [0, 16, 33, 225, 1225, 5321]
    # warm-up samples sit in the first `order` places, a constant at place 0
    data, chans, _, _ = Cases.catalogue()["lpc_o12_s14_b16"]
    _, res, rec = flac.unpack(data)
    assert res[:12].tolist() == chans[0][:12] and rec["order"][0] == 12
    _, res, _ = flac.unpack(Cases.catalogue()["types"][0])
    assert res[0] == -1234 and not res[1:192].any()


def _streaminfo_patch(data, **kw):
    """The stream with STREAMINFO fields overwritten (rate 20 bits, channels-1 3 bits, depth-1 5 bits at byte 18 of the file)."""
    v = int.from_bytes(data[18:22], "big")
    rate, ch, depth = v >> 12, ((v >> 9) & 7) + 1, ((v >> 4) & 31) + 1
    rate, ch, depth = kw.get("rate", rate), kw.get("channels", ch), kw.get("depth", depth)
    v = (rate << 12) | ((ch - 1) << 9) | ((depth - 1) << 4) | (v & 15)
    return data[:18] + v.to_bytes(4, "big") + data[22:]


def _frame(chans=([5, -5, 9, 0] * 4,), bps=16, **kw):
    return W.write_frame([list(c) for c in chans], bps, 16000, 0, **kw)


def _stream(frames, chans=1, bps=16, n=16):
    return b"fLaC" + W.metadata_block(0, W.streaminfo(16, 16, 16000, chans, bps, n, bytes(16)), True) + frames


def _refix(frame, header_len=None):
    """The frame with both CRCs made right again after an edit (header_len bytes before the CRC-8)."""
    body = bytearray(frame[:-2])
    if header_len is not None:
        body[header_len] = W.crc8(bytes(body[:header_len]))
    return bytes(body) + W.crc16(bytes(body)).to_bytes(2, "big")


def test_refusals():
    good = _stream(_frame(spec=dict(kind="fixed", order=2)))
    assert _code(good) == OK and _code(good, "unpack") == OK
    hdr = 6                                                         # sync(2) codes(2) frame number(1) block size(1), then the CRC-8
    f = bytearray(_frame(spec=dict(kind="fixed", order=2)))
    cases = {}
    # CRC mismatches: a flipped bit in the header, one in the body
    b = bytearray(f); b[3] ^= 0x02; cases["header bit"] = bytes(b)
    b = bytearray(f); b[10] ^= 0x10; cases["body bit"] = bytes(b)
    b = bytearray(f); b[-1] ^= 0x01; cases["crc16 itself"] = bytes(b)
    # reserved codes, with both CRCs right
    b = bytearray(f); b[1] |= 0x02; cases["reserved sync bit"] = _refix(bytes(b), hdr)
    b = bytearray(f); b[2] &= 0x0f; cases["block size code 0"] = _refix(bytes(b), hdr)
    b = bytearray(f); b[2] |= 0x0f; cases["sample rate code 15"] = _refix(bytes(b), hdr)
    b = bytearray(f); b[3] = (b[3] & 0x0f) | 0xb0; cases["channel assignment 11"] = _refix(bytes(b), hdr)
    b = bytearray(f); b[3] = (b[3] & 0xf1) | 0x06; cases["sample size code 3"] = _refix(bytes(b), hdr)
    b = bytearray(f); b[3] |= 0x01; cases["reserved header bit"] = _refix(bytes(b), hdr)
    b = bytearray(f); b[4] = 0xff; cases["frame number lead byte"] = _refix(bytes(b), hdr)
    b = bytearray(f); b[7] |= 0x80; cases["subframe padding bit"] = _refix(bytes(b))
    b = bytearray(f); b[7] = (b[7] & 0x81) | (0x02 << 1); cases["reserved subframe type"] = _refix(bytes(b))
    b = bytearray(f); b[7] = (b[7] & 0x81) | (0x0d << 1); cases["fixed order 5"] = _refix(bytes(b))
    for name, frame in cases.items():
        assert _code(_stream(frame)) == BITSTREAM, name
        assert _code(_stream(frame), "unpack") == BITSTREAM, name
    # an order above the block size; partitions that do not divide the block or undercut the order; a negative shift; precision 1111;
    # a reserved residual method
    def sub(bits):
        w = W.BitWriter()
        w.put(0x3ffe, 14); w.put(0, 2); w.put(6, 4); w.put(5, 4); w.put(0, 4); w.put(4, 3); w.put(0, 1); w.put(0, 8); w.put(bits[0] - 1, 8)
        head = w.bytes()
        w.put(W.crc8(head), 8)
        for v, n in bits[1]:
            w.put(v & ((1 << n) - 1), n)
        w.align()
        body = w.bytes()
        return _stream(body + W.crc16(body).to_bytes(2, "big"), n=bits[0])
    lpc_head = lambda order: [(0, 1), (32 | (order - 1), 6), (0, 1)] + [(1, 16)] * order
    built = {
        "order above block": (4, lpc_head(8) + [(11, 4), (3, 5)] + [(1, 12)] * 8),
        "negative shift": (16, lpc_head(2) + [(11, 4), (-3, 5), (1, 12), (1, 12), (0, 2), (0, 4), (0, 4)] + [(1, 1)] * 14),
        "precision 1111": (16, lpc_head(2) + [(15, 4), (3, 5)] + [(0, 16)] * 8),
        "partition does not divide": (17, [(0, 1), (8, 6), (0, 1), (0, 2), (1, 4)] + [(0, 16)] * 8),
        "first partition below order": (16, [(0, 1), (8 | 4, 6), (0, 1)] + [(1, 16)] * 4 + [(0, 2), (3, 4)] + [(0, 16)] * 8),
        "reserved residual method": (16, [(0, 1), (8, 6), (0, 1), (2, 2), (0, 4)] + [(0, 16)] * 8),
    }
    for name, bits in built.items():
        assert _code(sub(bits)) == BITSTREAM, name
    # frames that disagree with STREAMINFO
    assert _code(_streaminfo_patch(good, rate=8000)) == BITSTREAM
    assert _code(_streaminfo_patch(good, channels=2)) == BITSTREAM
    assert _code(_streaminfo_patch(good, depth=24)) == BITSTREAM
    # containers
    assert _code(good[4:]) == BITSTREAM and _code(b"fLaC") == BITSTREAM and _code(b"") == BITSTREAM
    assert _code(b"fLaC" + W.metadata_block(4, bytes(8), False) + good[4:]) == BITSTREAM          # STREAMINFO must come first
    assert _code(b"fLaC" + W.metadata_block(0, good[8:42], False) + W.metadata_block(0, good[8:42], True) + good[42:]) == BITSTREAM
    assert _code(b"fLaC" + W.metadata_block(127, bytes(4), True)) == BITSTREAM
    assert _code(good + b"\x00\x00\x00") == BITSTREAM                                            # lost sync after the last frame
    # unsupported: more than 24 bits, Ogg
    assert _code(_streaminfo_patch(good, depth=32)) == UNSUPPORTED
    assert _code(b"OggS" + bytes(60)) == UNSUPPORTED
    assert _code(_streaminfo_patch(good, depth=32), "streaminfo") == UNSUPPORTED
    # a leading ID3v2 tag is skipped
    assert _code(b"ID3\x03\x00\x00\x00\x00\x00\x05" + bytes(5) + good) == OK


def test_truncation_at_every_byte():
    """One small stream cut at every length: never a crash, and every outcome is OK with no more frames than fit, or
    SS_ERR_BITSTREAM (a cut inside the metadata)."""
    flac = _flac()
    data, chans, _, _ = Cases.catalogue()["stereo_switching"]
    full = flac.probe(data)
    ends = R.decode(data)[0]["frame_ends"]
    assert full["frames"] == len(ends) == 5
    for n in range(len(data)):
        cut = data[:n]
        try:
            info = flac.probe(cut)
        except flac.FlacError as e:
            assert e.code == BITSTREAM and n < 42, n
            continue
        assert n >= 42 and info["frames"] == sum(1 for e in ends if e <= n), n
        part = flac.unpack(cut)
        ints = flac.restore_host([part], False, True)[1][0]
        assert ints.shape[1] == info["samples"] and ints.tolist() == [c[:info["samples"]] for c in chans]


def test_bit_flips_are_caught_or_harmless():
    """Every single-bit flip in the frames of a small two-frame stream.  The CRCs catch it (SS_ERR_BITSTREAM); the one other outcome
    is a flip that makes a frame's bits run past the end of the data (an escape code, a larger Rice parameter), which is what a
    truncated last frame looks like: the stream ends before that frame.  Nothing crashes, and no flip yields a sample that differs."""
    flac = _flac()
    data, chans, _, _ = Cases.catalogue()["lpc_o8_s14_b16"]
    dropped = 0
    for bit in range(42 * 8, len(data) * 8):
        b = bytearray(data)
        b[bit >> 3] ^= 0x80 >> (bit & 7)
        try:
            info, res, rec = flac.unpack(bytes(b))
        except flac.FlacError as e:
            assert e.code == BITSTREAM, bit
            continue
        assert info["frames"] < 2 and info["samples"] == 192 * info["frames"], bit
        assert flac.restore_host([(info, res, rec)], False, True)[1][0].tolist() == [chans[0][:info["samples"]]]
        dropped += 1
    assert dropped < 0.02 * (len(data) - 42) * 8


def test_pool_size_never_follows_the_machine(monkeypatch):
    flac = _flac()
    monkeypatch.setattr(os, "cpu_count", lambda: 384)
    assert flac.pool_size(1000) == 16 and flac.pool_size(3) == 3 and flac.pool_size(1000, threads=64) == 16
    assert flac.pool_size(0) == 1 and flac.pool_size(5, threads=2) == 2


# ---- manifest cells ----------------------------------------------------------------------------------------------------------------
def _wav_bytes(x, sr=16000):
    bio = io.BytesIO()
    with wave.open(bio, "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(sr)
        w.writeframes(np.asarray(x, "<i2").tobytes())
    return bio.getvalue()


def stored_zip(path, members):
    """A ZIP_STORED archive as fairseq's create_zip writes it, and its manifest as get_zip_manifest reads it: offset of a member =
    header_offset + 30 + len(file name) + len(extra), length = file_size."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_STORED) as z:
        for name, data in members.items():
            z.writestr(name, data)
    cells = {}
    with zipfile.ZipFile(path) as z:
        raw = open(path, "rb").read()
        for i in z.infolist():
            n_name, n_extra = int.from_bytes(raw[i.header_offset + 26:i.header_offset + 28], "little"), \
                int.from_bytes(raw[i.header_offset + 28:i.header_offset + 30], "little")
            cells[i.filename] = f"{path}:{i.header_offset + 30 + n_name + n_extra}:{i.file_size}"
    return cells


def test_parse_audio_cell_and_sniffing(tmp_path):
    from streamspeech_amd import frontend
    _flac()
    pcm = Cases.catalogue()["block192"][1][0]
    feats = np.arange(7 * 80, dtype=np.float32).reshape(7, 80)
    bio = io.BytesIO(); np.save(bio, feats)
    members = {"a.npy": bio.getvalue(), "b.flac": Cases.catalogue()["block192"][0], "c.wav": _wav_bytes(pcm), "d.bin": b"\x00" * 64}
    cells = stored_zip(str(tmp_path / "pack.zip"), members)
    for name, cell in cells.items():
        parsed = frontend.parse_audio_cell(cell)
        assert parsed[0] == str(tmp_path / "pack.zip") and len(parsed) == 3 and parsed[2] == len(members[name])
        assert frontend.read_cell_bytes(cell) == members[name]
    assert frontend.parse_audio_cell("/x/y.wav") == ("/x/y.wav",) and frontend.parse_audio_cell("/x/y.flac") == ("/x/y.flac",)
    assert frontend.parse_audio_cell("/x/y.npy") == ("/x/y.npy",)
    with pytest.raises(ValueError, match="pack.zip:1"):
        frontend.parse_audio_cell("pack.zip:1")
    assert [frontend.sniff(frontend.read_cell_bytes(cells[n]), cells[n]) for n in ("a.npy", "b.flac", "c.wav")] == ["npy", "flac", "wav"]
    with pytest.raises(ValueError) as e:
        frontend.sniff(frontend.read_cell_bytes(cells["d.bin"]), cells["d.bin"])
    assert cells["d.bin"] in str(e.value)
    mp3 = open(os.path.join(ROOT, "tests", "golden", "mp3", "common_voice_fr_17301936.mp3"), "rb").read()
    assert frontend.sniff(mp3) == "mp3"
    assert np.array_equal(frontend.read_features(frontend.read_cell_bytes(cells["a.npy"])), feats)
    with pytest.raises(ValueError, match="shape"):
        bio = io.BytesIO(); np.save(bio, np.zeros((3, 40), np.float32))
        frontend.read_features(bio.getvalue(), "bad.npy")
    # read_wav's file-object form gives the file form's result; the MP3 refusal message is unchanged
    (tmp_path / "c.wav").write_bytes(members["c.wav"])
    x0, sr0 = frontend.read_wav(str(tmp_path / "c.wav"))
    x1, sr1 = frontend.read_wav(io.BytesIO(frontend.read_cell_bytes(cells["c.wav"])))
    assert sr0 == sr1 == 16000 and np.array_equal(x0, x1) and np.array_equal(x0, np.asarray(pcm, np.float32) / 32768.0)
    with pytest.raises(IOError, match="no MP3 decoder is available here; convert x.mp3 to PCM WAV"):
        frontend.read_wav("x.mp3")
    assert frontend.is_flac("A.FLAC") and frontend.is_flac(b"fLaC\x00") and not frontend.is_flac("a.wav") and not frontend.is_flac(b"RIFF")
    # a cell that reaches past the end of the archive
    with pytest.raises(ValueError, match="past the end"):
        frontend.read_cell_bytes(f"{tmp_path / 'pack.zip'}:10:{10 ** 7}")


def test_refused_transforms_are_named(tmp_path):
    import argparse
    from streamspeech_amd import frontend
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    frontend.check_eval_transforms({"transforms": {"*": ["global_cmvn"], "_train": ["global_cmvn", "specaugment"]}})
    frontend.check_eval_transforms({})
    with pytest.raises(ValueError, match="utterance_cmvn"):
        frontend.check_eval_transforms({"transforms": {"*": ["utterance_cmvn"]}})
    with pytest.raises(ValueError, match="delta_deltas"):
        frontend.check_eval_transforms({"feature_transforms": {"_eval": ["global_cmvn", "delta_deltas"], "*": ["global_cmvn"]}})
    with pytest.raises(ValueError, match="specaugment"):
        frontend.check_eval_transforms({"transforms": {"dev": ["specaugment"], "*": ["global_cmvn"]}}, "dev")
    # through the loader the offline driver and the agents use: refused before any model is built
    (tmp_path / "config.yaml").write_text("transforms:\n  '*':\n  - utterance_cmvn\n")
    ns = argparse.Namespace(config_yaml="config.yaml", data_bin=str(tmp_path), model_path="synthetic:0", global_stats=None)
    with pytest.raises(ValueError, match="utterance_cmvn"):
        StreamSpeechS2STAgent.load_model_vocab(argparse.Namespace(device="cpu"), ns)
