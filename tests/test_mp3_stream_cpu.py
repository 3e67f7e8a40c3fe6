"""CPU checks of the resumable MP3 host stage (ss_mp3_stream_*, csrc/mp3_host.hip) and of the pools' MP3 route on a stub engine: no
GPU work is issued here.  The yardstick is the whole-file decoder (ss_mp3_probe / ss_mp3_unpack) and every comparison is exact.
The device stage is checked on the GPU (tests/test_mp3_stream_gpu.py).

Trailing tags are not recognised in a stream (finding them needs the end of the file), and the identity with the whole-file calls
is stated for inputs whose end the whole-file scan does not cut.  One catalogue stream, `id3_wrapped`, carries an ID3v1 trailer
behind its ID3v2 header: it is streamed without the trailer (test_inputs_end_on_a_frame checks that this is the only such input and
that the whole-file records do not depend on the trailer); test_trailing_tag_is_garbage_in_a_stream pins what a stream does with it."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import mp3_ref as R
import mp3_writer as Wr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden", "mp3")
EXAMPLES = sorted(f for f in os.listdir(GOLD) if f.endswith(".mp3"))
CAT = Wr.catalogue()
MAX_KEPT = 1441 + 4                              # one maximal frame + the look-ahead: what a stream may keep unconsumed

STREAM_SYMBOLS = ("ss_mp3_stream_create", "ss_mp3_stream_destroy", "ss_mp3_stream_reset", "ss_mp3_stream_bound", "ss_mp3_stream_push",
                  "ss_mp3_stream_query", "ss_mp3_stream_copy", "ss_mp3_stream_synthesize")


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


def stream_inputs():
    """name -> bytes: every catalogue stream and both example files, as a stream sees them (see the module docstring)."""
    out = {}
    for name, entry in CAT.items():
        d = entry[0]
        out[name] = d[:-128] if name == "id3_wrapped" else d
    for name in EXAMPLES:
        out[name] = open(os.path.join(GOLD, name), "rb").read()
    return out


INPUTS = stream_inputs()


def chunkings(n, with_bytes=True):
    """name -> chunk sizes covering n bytes: whole, 1 byte at a time, fixed 7 / 417 / 2560 / 4096, three seeded random ones with
    sizes in [0, 3000]."""
    out = {"whole": [n]}
    if with_bytes:
        out["1"] = [1] * n
    for k in (7, 417, 2560, 4096):
        out[str(k)] = [k] * (n // k) + ([n % k] if n % k else [])
    for seed in (1, 2, 3):
        rng, sizes, left = np.random.default_rng(seed), [], n
        while left:
            k = min(int(rng.integers(0, 3001)), left)
            sizes.append(k)
            left -= k
        out[f"random{seed}"] = sizes
    return out


def feed(data, sizes, join=False, finish=True):
    """Push `data` in chunks of `sizes` (the last with finished) -> (q, rec, bits of all pushes, the infos after each push)."""
    mp3 = _mp3()
    st = mp3.Mp3Stream(join)
    qs, recs, bits, infos, at = [], [], [], [], 0
    for i, k in enumerate(sizes):
        ch = st.push(data[at:at + k], finished=finish and i == len(sizes) - 1)
        at += k
        qs.append(ch.q.copy()); recs.append(ch.rec.copy()); bits.append(ch.bits.copy()); infos.append(ch.info)
    assert at == len(data)
    st.close()
    return np.concatenate(qs), np.concatenate(recs), np.concatenate(bits), infos


def same_records(got, want):
    q, rec, bits = got[:3]
    wq, wrec, wbits = want
    return (q.shape == wq.shape and np.array_equal(q, wq) and rec.tobytes() == wrec.tobytes() and np.array_equal(bits, wbits))


# ---- ABI ----------------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_header_and_bindings():
    from streamspeech_amd import lib as L
    lib = _lib()
    header = open(os.path.join(ROOT, "include", "streamspeech_hip.h")).read()
    declared = set(re.findall(r"\b(ss_[a-z0-9_]+)\s*\(", header))
    for name in STREAM_SYMBOLS:
        assert name in declared and name in L.SIGNATURES and hasattr(lib, name), name
    assert lib.ss_abi_version() == 2 and "#define SS_ABI_VERSION 2" in header
    mp3 = _mp3()
    assert C.sizeof(mp3.Mp3StreamInfo) == 80 and mp3.STREAM_SEG_DTYPE.itemsize == 48


def test_inputs_end_on_a_frame():
    """Every streamed input ends where its last frame ends (the condition of the identity), and the one trailer removed for that
    changes nothing the whole-file calls write."""
    mp3 = _mp3()
    for name, d in INPUTS.items():
        fr = R.frames(d)
        assert fr[-1][0] + fr[-1][1]["len"] == len(d), name
    full, cut = mp3.unpack(CAT["id3_wrapped"][0]), mp3.unpack(INPUTS["id3_wrapped"])
    assert full[0] == cut[0] and same_records(full[1:], cut[1:])
    assert [n for n, e in CAT.items() if e[0] != INPUTS[n]] == ["id3_wrapped"]


# ---- any chunking equals the whole-file unpack ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_chunkings_equal_the_whole_file_unpack(name):
    mp3 = _mp3()
    d = INPUTS[name]
    info, q, rec, bits = mp3.unpack(d)
    for cname, sizes in chunkings(len(d)).items():
        got = feed(d, sizes)
        assert same_records(got, (q, rec, bits)), (name, cname)
        last = got[3][-1]
        assert (last["frames"], last["granules"], last["sample_rate"], last["channels"], last["version"], last["delay"],
                last["padding"], last["samples"], last["skip"]) == \
               (info["frames"], info["granules"], info["sample_rate"], info["channels"], info["version"], info["delay"],
                info["padding"], info["samples"], info["skip"]), (name, cname)
        assert last["finished"] == 1 and last["buffered"] == 0 and last["bytes_in"] == len(d) and last["skipped_frames"] == 0
        assert max(i["buffered"] for i in got[3]) < MAX_KEPT, (name, cname)


@pytest.mark.parametrize("name", EXAMPLES)
def test_a_frame_is_out_four_bytes_after_its_end(name):
    """Byte by byte: frame k's records are out no later than the push that delivers byte pos[k + 1] + 3 (the look-ahead header)."""
    d = INPUTS[name]
    pos = [p for p, _ in R.frames(d)]
    st = _mp3().Mp3Stream()
    frames_after = np.zeros(len(d), np.int64)
    for i in range(len(d)):
        frames_after[i] = st.push(d[i:i + 1]).info["frames"]
    for k in range(len(pos) - 1):
        assert frames_after[pos[k + 1] + 3] >= k + 1, k
        assert frames_after[pos[k + 1] + 2] <= k, k                 # and not before the look-ahead is complete
    assert st.push(b"", finished=True).info["frames"] == len(pos)   # the last frame needs no look-ahead
    st.close()


def test_state_stays_bounded_on_a_long_stream():
    """Sixty frames (ten times a catalogue stream) written as ONE stream, since every frame after the first points back into the
    reservoir: after every push the object keeps fewer bytes than one maximal frame + 4."""
    mp3 = _mp3()
    rng = np.random.default_rng(77)
    gr = Wr.sequence(rng, 60, 2, 1, [(0, False), (1, False), (2, False), (3, False)])
    d, _ = Wr.write_stream(gr, 48000)
    want = mp3.unpack(d)
    assert want[0]["frames"] == 60
    for cname, sizes in chunkings(len(d), with_bytes=False).items():
        got = feed(d, sizes)
        assert same_records(got, want[1:]), cname
        kept = [i["buffered"] for i in got[3]]
        assert max(kept) < MAX_KEPT and kept[-1] == 0, (cname, max(kept))


# ---- a push is a transaction --------------------------------------------------------------------------------------------------------
def _corrupt_big_values(data, frame):
    """big_values of granule 0, channel 0 of `frame` := 511 (> 288), in an MPEG-1 stereo stream without CRC: bits 32..40 of the side
    info (9 main_data_begin + 3 private + 8 scfsi + 12 part2_3_length in front)."""
    b = bytearray(data)
    p = R.frames(data)[frame][0] + 4
    b[p + 4] = 0xFF
    b[p + 5] |= 0x80
    return bytes(b)


def test_a_failed_push_leaves_the_stream_as_it_was():
    mp3 = _mp3()
    d = CAT["mpeg1_stereo_ms"][0]
    pos = [p for p, _ in R.frames(d)]
    want = mp3.unpack(d)
    bad = _corrupt_big_values(d, 3)
    with pytest.raises(mp3.Mp3Error) as e:
        mp3.unpack(bad)
    assert e.value.code == mp3.SS_ERR_BITSTREAM
    c0 = pos[2] + 50                                               # mid-frame, so the object holds unconsumed bytes
    st = mp3.Mp3Stream()
    parts = [st.push(d[:c0])]
    before = st.info
    with pytest.raises(mp3.Mp3Error) as e:
        st.push(bad[c0:pos[4] + 4])                                # completes the corrupt frame 3
    assert e.value.code == mp3.SS_ERR_BITSTREAM and st.info == before
    with pytest.raises(mp3.Mp3Error) as e:
        st.push(d[c0:pos[4] + 4], cap=1)                           # frames 2 and 3: eight records do not fit one
    assert e.value.code == mp3.SS_ERR_CAPACITY and st.info == before
    parts.append(st.push(d[c0:], finished=True))
    got = tuple(np.concatenate([getattr(p, k) for p in parts]) for k in ("q", "rec", "bits"))
    assert same_records(got, want[1:])
    assert st.info["bytes_in"] == len(d)
    with pytest.raises(mp3.Mp3Error) as e:                         # finished: no more data until reset()
        st.push(b"x")
    assert e.value.code == 2
    st.reset()
    again = st.push(d, finished=True)
    assert same_records((again.q, again.rec, again.bits), want[1:])
    st.close()


def test_bound_always_suffices_and_rollback_takes_a_push_back():
    mp3 = _mp3()
    d = CAT["mpeg2_24k"][0]                                         # the most records per byte of the catalogue
    st = mp3.Mp3Stream()
    assert st.lib.ss_mp3_stream_bound(st._h, len(d)) >= mp3.probe(d)["granule_channels"]
    st.push(d[:700])
    st.mark()
    before = st.info
    ch = st.push(d[700:1500])
    assert st.info != before and ch.granules > 0
    st.rollback()
    assert st.info == before
    rest = st.push(d[700:], finished=True)
    assert st.info["frames"] == mp3.probe(d)["frames"] and rest.granules > 0
    st.close()


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_refusals_are_those_of_the_whole_file_calls():
    mp3 = _mp3()
    ms = CAT["mpeg1_stereo_ms"][0]
    b = bytearray(ms)
    for p, _ in R.frames(ms):
        b[p + 3] |= 0x10
    cases = {"intensity": bytes(b), "free": Wr.raw_header(bri=0) + bytes(400), "layer2": (Wr.raw_header(layer=2) + bytes(188)) * 4,
             "reserved": Wr.raw_header(sri=3) + bytes(400)}
    for name, d in cases.items():
        with pytest.raises(mp3.Mp3Error) as e:
            mp3.unpack(d)
        assert e.value.code == mp3.SS_ERR_UNSUPPORTED, name
        for sizes in ([len(d)], [3, 5, len(d) - 8]):
            st = mp3.Mp3Stream()
            with pytest.raises(mp3.Mp3Error) as e:
                at = 0
                for i, k in enumerate(sizes):
                    st.push(d[at:at + k], finished=i == len(sizes) - 1)
                    at += k
            assert e.value.code == mp3.SS_ERR_UNSUPPORTED, name
            st.close()
    for name in EXAMPLES + ["mpeg1_stereo_ms"]:                    # cut at a frame start: the first frame points back
        d = INPUTS[name]
        cut = d[R.frames(d)[2][0]:]
        with pytest.raises(mp3.Mp3Error) as e:
            mp3.unpack(cut)
        assert e.value.code == mp3.SS_ERR_BITSTREAM
        st = mp3.Mp3Stream(join=False)
        with pytest.raises(mp3.Mp3Error) as e:
            st.push(cut, finished=True)
        assert e.value.code == mp3.SS_ERR_BITSTREAM and st.info["frames"] == 0
        st.close()


def test_trailing_tag_is_garbage_in_a_stream():
    """The documented limit: a last frame directly followed by an ID3v1 tag fails its look-ahead in a stream (the whole-file scan
    cuts the tag first); nothing faults, earlier frames are those of the file."""
    mp3 = _mp3()
    d = CAT["id3_wrapped"][0]
    want = mp3.unpack(d)
    per = want[0]["granule_channels"] // want[0]["frames"]
    st = mp3.Mp3Stream()
    ch = st.push(d)                                                # everything but what still waits for more bytes
    n = len(ch.q)
    assert n >= len(want[1]) - per and np.array_equal(ch.q[:len(want[1]) - per], want[1][:len(want[1]) - per])
    assert st.info["buffered"] < MAX_KEPT
    st.close()


# ---- joining mid-stream -------------------------------------------------------------------------------------------------------------
def first_decodable(data, frame_list, start):
    """Index of the first frame from `start` on whose main data lies wholly in the frames from `start` on: main_data_begin <= the
    main-data bytes of the frames between (frame length - header - CRC - side info each)."""
    have = 0
    for k in range(start, len(frame_list)):
        p, h = frame_list[k]
        crc = 0 if h["prot"] else 2
        mdb = R._Bits(data[p + 4 + crc:p + 4 + crc + 2]).get(9 if h["ver"] == 3 else 8)
        if mdb <= have:
            return k
        have += h["len"] - 4 - crc - h["side"]
    return None


@pytest.mark.parametrize("name", EXAMPLES)
def test_join_decodes_from_the_first_wholly_decodable_frame(name):
    mp3 = _mp3()
    d = INPUTS[name]
    fr = R.frames(d)
    info, q, rec, bits = mp3.unpack(d)
    per = info["granule_channels"] // info["frames"]
    for start in (40, 41, 100):
        k = first_decodable(d, fr, start)
        assert k is not None and k > start
        cut = d[fr[start][0]:]
        for sizes in ([len(cut)], chunkings(len(cut), False)["417"], chunkings(len(cut), False)["random2"]):
            got = feed(cut, sizes, join=True)
            assert same_records(got, (q[k * per:], rec[k * per:], bits[k * per:])), (name, start)
            assert got[3][-1]["skipped_frames"] == k - start and got[3][-1]["frames"] == len(fr) - k
    # 100 bytes into a frame: first make sure the whole-file scan finds exactly the following frames behind the cut (no false sync)
    for start in (40, 100):
        cut = d[fr[start][0] + 100:]
        assert mp3.probe(cut)["frames"] == len(fr) - (start + 1)
        k = first_decodable(d, fr, start + 1)
        got = feed(cut, chunkings(len(cut), False)["2560"], join=True)
        assert same_records(got, (q[k * per:], rec[k * per:], bits[k * per:])), (name, start)


def test_join_frames_are_the_ones_computed_by_hand():
    """171 main-data bytes per 192-byte frame and the main_data_begin values of the two files: cuts at 40 / 41 / 100 start
    decoding at 41 / 42 / 103 and 43 / 44 / 102 (derived here as the join test derives them, not looked up)."""
    want = {"common_voice_fr_17301936.mp3": [41, 42, 103], "common_voice_fr_17767732.mp3": [43, 44, 102]}
    for name, ks in want.items():
        d = INPUTS[name]
        fr = R.frames(d)
        assert all(h["len"] == 192 and h["len"] - 4 - h["side"] == 171 for _, h in fr)
        assert [first_decodable(d, fr, s) for s in (40, 41, 100)] == ks


# ---- gapless ------------------------------------------------------------------------------------------------------------------------
def test_gapless_skip_and_hold_back():
    mp3 = _mp3()
    d = INPUTS["lame_gapless"]
    pr = mp3.probe(d)
    assert (pr["delay"], pr["padding"]) == (576, 1200)
    total, skip, hold = pr["granules"] * 576, 576 + 529, 1200 - 529
    assert pr["samples"] == total - skip - hold
    for sizes in chunkings(len(d)).values():
        st = mp3.Mp3Stream()
        at, released, written = 0, 0, 0
        for i, k in enumerate(sizes):
            ch = st.push(d[at:at + k], finished=i == len(sizes) - 1)
            at += k
            released += ch.released
            written += ch.written
            assert ch.held == written - ch.written - (released - ch.released)
            assert released == ch.info["samples"] <= total - skip - hold
            assert released == max(0, ch.info["granules"] * 576 - skip - hold)        # never into the last `hold` decoded samples
        assert released == pr["samples"] and written == total - skip
        st.close()
    plain = feed(INPUTS["crc_32k"], chunkings(len(INPUTS["crc_32k"]))["7"])[3]
    assert all(i["samples"] == i["granules"] * 576 and i["skip"] == 0 and i["hold"] == 0 for i in plain)   # no tag: nothing held


# ---- the pools' host logic on a stub engine -------------------------------------------------------------------------------------------
def _stub_pool(max_sessions=4, max_rows=64, speech=False):
    import test_pcm_cpu as P

    class Engine(P._StubEngine):
        def __init__(self):
            super().__init__()
            self.mp3_calls = []

        def mp3_stream_decode(self, arena, items):
            self.mp3_calls.append([(ch.granules, at) for ch, _, _, at, _ in items])
            n = 0
            for ch, state, dst, at, _ in items:
                assert state.shape == (2, ch.channels, 1152) and at + ch.written <= dst.numel()
                dst[at:at + ch.written] = 1.0
                n += len(ch.rec)
            return n, n * (1152 + 80)

    from streamspeech_amd.speech_pool import SpeechSessionPool
    from streamspeech_amd.text_pool import TextSessionPool
    eng = Engine()
    pool = SpeechSessionPool(eng, max_sessions, max_rows, vocoder=P._Voc()) if speech else TextSessionPool(eng, max_sessions, max_rows)
    return pool, eng, P


def test_pool_routes_exclude_each_other():
    from streamspeech_amd.pcm import PcmFormat
    from streamspeech_amd.simuleval_shim import SpeechSegment
    pool, eng, P = _stub_pool(speech=True)
    a48 = P._args(sr=48000)
    with pytest.raises(ValueError):
        pool.open("asr", a48, dicts=P._dicts(), mp3_in=True, pcm_in=PcmFormat("s16le"))
    with pytest.raises(ValueError):
        pool.open("asr", a48, dicts=P._dicts(), mp3_in={"joined": True})
    assert pool.sessions == {}
    m = pool.open("s2st", a48, dicts=P._dicts(), mp3_in={"join": True}, pcm_out="s16le")
    p = pool.open("asr", a48, dicts=P._dicts(), pcm_in=PcmFormat("s16le"))
    q = pool.open("asr", a48, dicts=P._dicts())
    assert pool.sessions[m].mp3_in == {"join": True} and pool.sessions[m].pcm_out == "s16le" and pool.sessions[p].mp3_in is None
    seg = SpeechSegment(content=[0.0] * 300, sample_rate=48000, finished=True)
    d = INPUTS[EXAMPLES[0]]
    for bad in (lambda: pool.push(m, seg), lambda: pool.push_pcm(m, bytes(600)), lambda: pool.step({q: seg, m: seg}),
                lambda: pool.push_mp3(p, d[:500]), lambda: pool.push_mp3(q, d[:500])):
        with pytest.raises(ValueError):
            bad()
    for s in pool.sessions.values():
        assert not s.pending and s.n_source() == 0 and s.mp3_chunk is None and s.pcm_chunk is None and not s.states.source_finished
    assert pool.sessions[m].mp3.info["bytes_in"] == 0


def test_pool_refused_pushes_change_nothing_and_finished_is_kept():
    mp3 = _mp3()
    pool, eng, P = _stub_pool(max_sessions=2, max_rows=16)
    d = INPUTS[EXAMPLES[0]]
    pos = [p for p, _ in R.frames(d)]
    # the rate: the file is at 48 kHz, the session at 16 kHz -- refused at the first accepted header, naming both
    low = pool.open("asr", P._args(sr=16000), dicts=P._dicts(), mp3_in=True)
    pool.push_mp3(low, d[:100])                                     # no header accepted yet (its look-ahead has not come): fine
    pool.step()
    before = pool.sessions[low].mp3.info
    with pytest.raises(ValueError) as e:
        pool.push_mp3(low, d[100:1000])
    assert "48000" in str(e.value) and "16000" in str(e.value) and f"session {low}" in str(e.value)
    assert pool.sessions[low].mp3.info == before and not pool.sessions[low].pending and pool.sessions[low].mp3_chunk is None
    pool.close(low)
    sid = pool.open("asr", P._args(sr=48000), dicts=P._dicts(), mp3_in=True)
    s = pool.sessions[sid]
    # admission: 30 frames are 34560 samples, 72 fbank rows, 18 encoder rows > max_rows 16
    with pytest.raises(ValueError) as e:
        pool.push_mp3(sid, d[:pos[30] + 4])
    assert f"session {sid}" in str(e.value) and "max_rows" in str(e.value)
    assert s.mp3.info["bytes_in"] == 0 and s.mp3.info["frames"] == 0 and not s.pending and s.n_source() == 0
    # a stream the decoder refuses: the library's code, the session named, nothing changed
    bad = bytearray(d[:pos[3] + 4])
    assert R.frames(d)[1][1]["prot"] == 1 and R.frames(d)[1][1]["nch"] == 1
    bad[pos[1] + 4 + 3] |= 0x03; bad[pos[1] + 4 + 4] |= 0xFE          # MPEG-1 mono, no CRC: big_values of granule 0 are bits 30..38
    with pytest.raises(mp3.Mp3Error) as e:
        pool.push_mp3(sid, bytes(bad))
    assert e.value.code == mp3.SS_ERR_BITSTREAM and f"session {sid}" in str(e.value) and s.mp3.info["bytes_in"] == 0
    # one frame (1152 samples: no fbank row yet at 48 kHz, so the stub engine needs no device), then the rest of the step's protocol
    pool.push_mp3(sid, d[:pos[1] + 4])
    assert s.pending and s.n_source() == 1152 and s.fe.n_pcm == 0 and not s.states.source_finished
    with pytest.raises(ValueError):
        pool.push_mp3(sid, d[pos[1] + 4:pos[1] + 8])                # already pushed in this step
    assert s.mp3.info["bytes_in"] == pos[1] + 4
    out = pool.step()
    assert set(out) == {sid} and len(eng.mp3_calls) == 1 and eng.mp3_calls[0] == [(2, 0)]
    ls = pool.last_step
    assert (ls["mp3_uploads"], ls["mp3_synth_calls"], ls["mp3_bytes_in"], ls["mp3_granules"]) == (1, 1, pos[1] + 4, 2)
    assert (ls["pcm_uploads"], ls["pcm_scatter_calls"]) == (0, 0)
    assert s.fe.n_pcm == 1152 and s.mp3_chunk is None and bool((s.fe._dev[:1152] == 1.0).all())
    pool.push_mp3(sid, b"", finished=True)                          # a bare finished: nothing to decode, the flag is kept
    assert s.states.source_finished
    pool.step()
    assert len(eng.mp3_calls) == 1 and (pool.last_step["mp3_uploads"], pool.last_step["mp3_synth_calls"]) == (0, 0)
    pool.reset(sid)
    assert s.mp3.info["bytes_in"] == 0 and s.mp3_state is None and s.n_source() == 0
    pool.close(sid)
    assert sid not in pool.sessions


def test_pool_holds_back_a_gapless_tail_in_the_history():
    """A LAME-tagged stream: the samples decoded but not released yet lie in the device history past n_pcm, the next step writes
    behind them, and what was committed at the end is the file's sample count."""
    mp3 = _mp3()
    pool, eng, P = _stub_pool()
    d = INPUTS["lame_gapless"]
    pr = mp3.probe(d)
    sid = pool.open("asr", P._args(sr=48000), dicts=P._dicts(), mp3_in=True)
    s = pool.sessions[sid]
    pos = [p for p, _ in R.frames(d)]
    cuts = [0, pos[1] + 4, pos[2] + 4, len(d)]
    written = 0
    for i in range(3):
        pool.push_mp3(sid, d[cuts[i]:cuts[i + 1]], finished=i == 2)
        ch = s.mp3_chunk
        at_want = s.fe.n_pcm + s.mp3_held
        if s.n_source() >= 1200:                                    # the stub engine has no fbank: stop before a row is due
            break
        pool.step()
        written += ch.written
        assert eng.mp3_calls[-1] == [(ch.granules, at_want)]
        assert s.fe.n_pcm + s.mp3_held == written and s.fe.n_pcm == max(0, s.mp3.info["granules"] * 576 - 1105 - 671)
    assert pr["samples"] == 6 * 1152 - 1105 - 671
