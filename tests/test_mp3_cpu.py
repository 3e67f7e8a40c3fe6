"""CPU checks of the MP3 ingest's host stage (csrc/mp3_host.hip via ss_mp3_probe / ss_mp3_unpack) and of the constant tables
typed in from the standard (csrc/mp3_tables.hpp): no GPU work is issued here.  The numeric stage is checked on the GPU
(tests/test_mp3_gpu.py) against the float64 restatement tests/mp3_ref.py, which is exercised here on the example streams."""
import hashlib
import json
import os
import wave

import numpy as np
import pytest

import mp3_ref as R
import mp3_writer as Wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "mp3")
FACTS = json.load(open(os.path.join(GOLD, "fixtures.json")))["files"]
EXAMPLES = sorted(FACTS)


def _lib():
    from streamspeech_amd import lib as L
    if not os.path.exists(L.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build()
    return L.load()


def _mp3():
    _lib()
    from streamspeech_amd import mp3
    return mp3


def _data(name):
    return open(os.path.join(GOLD, name), "rb").read()


# ---- tables -----------------------------------------------------------------------------------------------------------------------
# (table, entries, sum of code words, sum of code lengths) as typed in from Table B.7; tables 16-23 share table 16's codes and
# 24-31 table 24's (only linbits differ: csrc/mp3_tables.hpp kBigValueTables)
HUFF = [("1", 4, 3, 9), ("2", 9, 14, 37), ("3", 9, 14, 36), ("5", 16, 54, 91), ("6", 16, 51, 75), ("7", 36, 275, 267),
        ("8", 36, 266, 271), ("9", 36, 248, 229), ("10", 64, 1011, 554), ("11", 64, 1035, 507), ("12", 64, 990, 465),
        ("13", 256, 10746, 3025), ("15", 256, 13176, 2525), ("16", 256, 76158, 2921), ("24", 256, 62529, 2348),
        ("A", 16, 63, 78), ("B", 16, 120, 64)]


@pytest.mark.parametrize("name,n,csum,lsum", HUFF)
def test_huffman_table_is_a_complete_prefix_code(name, n, csum, lsum):
    cod, ln = R.table("h%s_cod" % name).astype(int), R.table("h%s_len" % name).astype(int)
    assert len(cod) == len(ln) == n
    assert int(cod.sum()) == csum and int(ln.sum()) == lsum
    assert all(c < (1 << l) for c, l in zip(cod, ln))
    words = [format(c, "0%db" % l) for c, l in zip(cod, ln)]
    for i, w in enumerate(words):
        for j, v in enumerate(words):
            assert i == j or not v.startswith(w), (name, i, j)
    assert sum(2.0 ** -l for l in ln) == 1.0                 # Kraft: every table of the standard is complete


def test_linbits_tables_share_codes():
    src = open(R.TABLES_HPP).read()
    rows = src[src.index("kBigValueTables[32]"):src.index("kSampleRates")]
    for t in range(16, 24):
        assert "{h16_cod, h16_len, 16, %d}" % Wr.LINBITS[t] in rows
    for t in range(24, 32):
        assert "{h24_cod, h24_len, 16, %d}" % Wr.LINBITS[t] in rows
    assert rows.count("{h16_cod") == 8 and rows.count("{h24_cod") == 8


def test_scalefactor_bands_all_nine_rates():
    for sr in range(9):
        assert R.SFB_LONG[sr][0] == 0 and R.SFB_LONG[sr][-1] == 576 and (np.diff(R.SFB_LONG[sr]) > 0).all()
        assert R.SFB_SHORT[sr][0] == 0 and R.SFB_SHORT[sr][-1] == 192 and (np.diff(R.SFB_SHORT[sr]) > 0).all()
    assert len(R.PRETAB) == 22 and R.PRETAB.sum() == 19


def test_synthesis_window_smooth():
    """D is stored as its half table kWinBase (symmetry is structural, not tested); the typed-in half must be smooth."""
    D = R.window_d()
    i = np.arange(512)
    h = D * np.where((i // 64) % 2 == 1, -1.0, 1.0)             # the prototype low-pass
    assert len(R.table("kWinBase")) == 257
    assert abs(D[256] - 1.144989014) < 1e-9 and D[0] == 0.0
    # the true window's fourth differences stay within 6 / 65536; one mistyped entry off by >= 3 units shows 6x that
    assert np.abs(np.diff(h, 4)).max() * 65536 <= 8


def test_device_cosine_and_window_tables():
    """The float32 tables the kernels read (kCos128, kCos144, kImdctWin, kAliasCs / Ca) are the float32 roundings of their
    defining formulas."""
    f32 = lambda x: np.where(np.abs(x) < 1e-12, 0.0, x).astype(np.float32)
    assert np.array_equal(R.table("kCos128").astype(np.float32), f32(np.cos(np.pi * np.arange(128) / 64)))
    assert np.array_equal(R.table("kCos144").astype(np.float32), f32(np.cos(np.pi * np.arange(144) / 72)))
    win = R._windows()
    assert np.array_equal(R.table("kImdctWin").astype(np.float32), f32(win.ravel()))
    c = R.ALIAS_C
    assert np.array_equal(R.table("kAliasCs").astype(np.float32), f32(1 / np.sqrt(1 + c * c)))
    assert np.array_equal(R.table("kAliasCa").astype(np.float32), f32(c / np.sqrt(1 + c * c)))


def test_synthesis_window_reconstructs_through_the_analysis_bank():
    """Analysis (C = D / 32, M[i][k] = cos((2i + 1)(k - 16) pi / 64)) then synthesis returns white noise delayed by 481
    samples to ~1e-4: the near-perfect reconstruction of the standard's filter bank, which a wrong sign or entry of D breaks."""
    D = R.window_d()
    M = np.cos((2 * np.arange(32)[:, None] + 1) * (np.arange(64)[None, :] - 16) * np.pi / 64)
    N = np.cos((16 + np.arange(64)[:, None]) * (2 * np.arange(32)[None, :] + 1) * np.pi / 64)
    x = np.random.default_rng(0).standard_normal(32 * 120)
    X, V, out = np.zeros(512), np.zeros(1024), []
    for t in range(120):
        X[32:] = X[:-32].copy(); X[:32] = x[32 * t:32 * t + 32][::-1]
        S = M @ (D / 32 * X).reshape(8, 64).sum(0)
        V[64:] = V[:-64].copy(); V[:64] = N @ S
        U = np.concatenate([np.concatenate([V[k * 128:k * 128 + 32], V[k * 128 + 96:k * 128 + 128]]) for k in range(8)])
        out.append((U * D).reshape(16, 32).sum(0))
    y = np.concatenate(out)
    err = y[481 + 512:] - x[512:len(y) - 481]
    assert np.sqrt(np.mean(err ** 2)) < 2e-4


# ---- example streams --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", EXAMPLES)
def test_fixture_is_the_recorded_file(name):
    d = _data(name)
    assert hashlib.sha256(d).hexdigest() == FACTS[name]["sha256"] and len(d) == FACTS[name]["bytes"]


@pytest.mark.parametrize("name", EXAMPLES)
def test_probe_example(name):
    info = _mp3().probe(_data(name))
    f = FACTS[name]
    assert (info["version"], info["sample_rate"], info["channels"]) == (1, 48000, 1)
    assert info["frames"] == f["frames"] and info["samples"] == f["samples"] == f["frames"] * 1152
    assert info["skip"] == 0 and info["delay"] == -1


def test_example_bit_accounting_is_exact():
    """Every granule-channel's scalefactors + Huffman data end exactly at its part2_3_length (694 in the two files), and the
    block types are the recorded ones: real LAME output through every Huffman table of the standard."""
    total = 0
    used = set()
    for name in EXAMPLES:
        d = _data(name)
        info, q, rec, bits = _mp3().unpack(d)
        p23 = np.array(R.part2_3_lengths(d))
        assert len(p23) == len(bits) == info["granule_channels"]
        assert np.array_equal(bits, p23)
        total += len(bits)
        f = FACTS[name]
        bt = rec["block_type"]
        assert [(bt == k).sum() for k in range(4)] == [f["granules_long"], f["granules_start"], f["granules_short"],
                                                       f["granules_stop"]]
        assert rec["mixed"].sum() == 0
        for pos, h in R.frames(d):
            b = R._Bits(d[pos + 4:pos + 4 + h["side"]])
            b.get(18)
            for _ in range(2):
                b.get(12 + 9 + 8 + 4)
                ws = b.get(1)
                if ws:
                    b.get(3); used.update([b.get(5), b.get(5)]); b.get(9)
                else:
                    used.update([b.get(5), b.get(5), b.get(5)]); b.get(7)
                b.get(2); used.add(("c1", b.get(1)))
    assert total == 694
    tables = {t for t in used if isinstance(t, int)}
    code_tables = {16 if 16 <= t < 24 else 24 if t >= 24 else t for t in tables} - {0}
    assert code_tables == {1, 2, 3, 5, 6, 7, 8, 9, 10, 11, 12, 13, 15, 16, 24}
    assert {("c1", 0), ("c1", 1)} <= used


@pytest.mark.parametrize("name", EXAMPLES)
def test_example_restatement_pcm_is_plausible(name):
    info, q, rec, _ = _mp3().unpack(_data(name))
    y = R.synthesize(info, q, rec)
    assert y.shape == (FACTS[name]["samples"],)
    assert np.isfinite(y).all() and np.abs(y).max() < 1.5
    assert 1e-3 < np.sqrt(np.mean(y ** 2)) < 0.5


# ---- writer streams ---------------------------------------------------------------------------------------------------------------
CAT = Wr.catalogue()


@pytest.mark.parametrize("name", sorted(CAT))
def test_writer_round_trip(name):
    data, sides, gr, sr, nch, lame = CAT[name]
    info, q, rec, bits = _mp3().unpack(data)
    flat = [g for fr in gr for grr in fr for g in grr]
    ngr = 2 if sr >= 32000 else 1
    assert (info["sample_rate"], info["channels"], info["frames"]) == (sr, nch, len(gr))
    assert info["version"] == (1 if sr >= 32000 else 2 if sr >= 16000 else 25)
    assert len(flat) == info["granule_channels"] == len(gr) * ngr * nch
    for i, g in enumerate(flat):
        assert np.array_equal(q[i], g.q), (name, i)
        assert np.array_equal(rec["sf_l"][i], g.sf_l) and np.array_equal(rec["sf_s"][i], g.sf_s), (name, i)
        assert (rec["global_gain"][i], rec["block_type"][i], rec["mixed"][i]) == (g.global_gain, g.block_type, int(g.mixed))
        assert tuple(rec["subblock_gain"][i]) == g.sbg and rec["scalefac_scale"][i] == g.scalefac_scale
        assert rec["preflag"][i] == g.preflag
        assert bits[i] == sides[i]["part2_3"]
        assert rec["nz"][i] == (np.nonzero(g.q)[0].max() + 1 if g.q.any() else 0)
    assert set(rec["ms"].tolist()) == ({1} if "ms" in name else {0})
    total = len(gr) * ngr * 576
    if lame:
        d, p = lame
        assert (info["delay"], info["padding"], info["skip"]) == (d, p, d + 529)
        assert info["samples"] == total - (d + 529) - (p - 529)
    else:
        assert info["samples"] == total and info["skip"] == 0


def test_writer_covers_the_lsf_scalefactor_ranges():
    """ISO/IEC 13818-3 scalefac_compress: < 400, 400..499 and 500..511 (preflag) all round-trip (test_writer_round_trip), in
    long, short and mixed granules."""
    seen = set()
    for name, (data, sides, gr, sr, nch, _) in CAT.items():
        if sr >= 32000:
            continue
        _, _, rec, _ = _mp3().unpack(data)
        for s, r in zip(sides, rec):
            rng = 0 if s["sfc"] < 400 else 1 if s["sfc"] < 500 else 2
            assert r["preflag"] == (rng == 2)
            seen.add((rng, int(s["block_type"] == 2) + int(s["mixed"])))
    assert {(r, c) for r in range(3) for c in range(3)} <= seen, seen


def test_writer_streams_use_the_reservoir():
    data, _, _, _, _, _ = CAT["mpeg1_stereo_ms"]
    mdb = [int.from_bytes(data[p + 4:p + 6], "big") >> 7 for p, _ in R.frames(data)]
    assert mdb[0] == 0 and all(m > 0 for m in mdb[1:])


def test_garbage_before_the_first_frame_is_skipped():
    data = CAT["crc_32k"][0]
    mp3 = _mp3()
    ref = mp3.unpack(data)
    got = mp3.unpack(bytes(range(1, 200)) + data)
    assert got[0]["frames"] == ref[0]["frames"] and np.array_equal(got[1], ref[1])


def _patched(data, fn):
    b = bytearray(data)
    for p, _ in R.frames(data):
        fn(b, p)
    return bytes(b)


def test_refused_headers():
    mp3 = _mp3()
    ms = CAT["mpeg1_stereo_ms"][0]
    intensity = _patched(ms, lambda b, p: b.__setitem__(p + 3, b[p + 3] | 0x10))
    free = Wr.raw_header(bri=0) + bytes(400)
    layer2 = (Wr.raw_header(layer=2) + bytes(188)) * 4
    reserved = Wr.raw_header(sri=3) + bytes(400)
    for name, d in (("intensity", intensity), ("free", free), ("layer2", layer2), ("reserved", reserved)):
        with pytest.raises(mp3.Mp3Error) as e:
            mp3.unpack(d)
        assert e.value.code == mp3.SS_ERR_UNSUPPORTED, name
    lib = _lib()
    assert b"unsupported" in lib.ss_error_string(mp3.SS_ERR_UNSUPPORTED)
    assert b"bitstream" in lib.ss_error_string(mp3.SS_ERR_BITSTREAM)


@pytest.mark.parametrize("name", EXAMPLES)
def test_truncation_never_crashes(name):
    """Cut at every 97th byte: each cut decodes fewer frames or reports SS_ERR_BITSTREAM."""
    mp3 = _mp3()
    d = _data(name)
    full = FACTS[name]["frames"]
    for cut in range(0, len(d), 97):
        try:
            info, q, rec, bits = mp3.unpack(d[:cut])
        except mp3.Mp3Error as e:
            assert e.code == mp3.SS_ERR_BITSTREAM, cut
            continue
        assert info["frames"] < full and len(bits) == info["granule_channels"]


def test_unpack_capacity_is_checked():
    mp3 = _mp3()
    lib = _lib()
    d = _data(EXAMPLES[0])
    q = np.zeros((10, 576), np.int16)
    rec = np.zeros(10, mp3.GRANULE_DTYPE)
    assert lib.ss_mp3_unpack(d, len(d), 10, q.ctypes.data, rec.ctypes.data, None) == mp3.SS_ERR_CAPACITY


def test_read_audio_wav_is_read_wav(tmp_path):
    from streamspeech_amd import frontend
    x = (np.sin(np.arange(4000) * 0.05) * 12000).astype("<i2")
    p = tmp_path / "a.wav"
    with wave.open(str(p), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(48000); w.writeframes(x.tobytes())
    a, sa = frontend.read_audio(str(p))
    b, sb = frontend.read_wav(str(p))
    assert sa == sb == 48000 and a.dtype == np.float32 and np.array_equal(a, b)
