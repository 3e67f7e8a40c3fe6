"""MP3 streams on the GPU: the incremental decoder (mp3.Mp3StreamDecoder, ss_mp3_stream_synthesize) against the whole-file decoder
(mp3.decode_batch) on the same bytes, and MP3-fed pool sessions against PCM-fed twins given the whole-file decode's samples.  Every
comparison is on the float32 bit patterns; no tolerance appears anywhere.  Inputs and chunkings are those of
tests/test_mp3_stream_cpu.py (whose docstring says why one catalogue stream is streamed without its ID3v1 trailer)."""
import numpy as np
import pytest
import torch

from tests import ref_fixtures as RF
from tests import mp3_ref as R
from tests.test_mp3_stream_cpu import EXAMPLES, INPUTS, chunkings, first_decodable

pytestmark = pytest.mark.gpu

BYTEWISE = "mpeg25_8k"                          # the one (short) stream also fed a byte at a time


@pytest.fixture(scope="module")
def model(hip_model):
    return hip_model


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _whole(name, dev, mono):
    from streamspeech_amd import mp3
    (pcm, sr), = mp3.decode_batch([INPUTS[name]], dev, mono=mono)
    return pcm.cpu().numpy(), sr


def _stream(data, sizes, dev, mono, join=False):
    from streamspeech_amd import mp3
    dec = mp3.Mp3StreamDecoder(dev, mono=mono, join=join)
    parts, at = [], 0
    for i, k in enumerate(sizes):
        parts.append(dec.push(data[at:at + k], finished=i == len(sizes) - 1))
        at += k
    info = dec.info
    dec.close()
    full = [p for p in parts if p.numel()]                       # (before the first header the channel count is unknown)
    return (torch.cat(full, dim=-1) if full else parts[-1]).cpu().numpy(), info


@pytest.mark.parametrize("mono", [True, False])
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_streaming_equals_whole_file(model, name, mono):
    d = INPUTS[name]
    want, _ = _whole(name, model.device, mono)
    for cname, sizes in chunkings(len(d), with_bytes=name == BYTEWISE).items():
        got, info = _stream(d, sizes, model.device, mono)
        assert got.shape == want.shape, (name, cname, got.shape, want.shape)
        assert np.array_equal(_bits(got), _bits(want)), (name, cname)
        assert info["samples"] == want.shape[-1]


def test_batch_invariance_of_the_many_session_call(model):
    """Sessions of different rate / version / channels in ONE ss_mp3_stream_synthesize call per step, each on its own chunk schedule
    (steps of zero, one and many granules): every session's output is its own whole-file decode, mono and planar."""
    from streamspeech_amd import mp3
    from streamspeech_amd.pcm import PcmArena
    names = ["mpeg1_stereo_ms", "mpeg2_24k", "mpeg25_8k", EXAMPLES[0], "lame_gapless", "mpeg25_11k_preflag_ms"]
    dev = model.device
    for mono in (True, False):
        want = {n: _whole(n, dev, mono)[0] for n in names}
        rng = np.random.default_rng(5)
        arena = PcmArena(dev)
        sess = []
        for i, n in enumerate(names):
            info = mp3.probe(INPUTS[n])
            rows = 1 if mono else info["channels"]
            cap = info["granules"] * 576 + 7                       # the held-back tail of a gapless stream is written too
            sess.append(dict(name=n, st=mp3.Mp3Stream(), at=0, written=0, released=0, state=None,
                             dst=torch.full((rows, cap), -777.25, dtype=torch.float32, device=dev), per=[], step=[0, 200, 2000, 777][i % 4]))
        steps = 0
        while any(s["at"] < len(INPUTS[s["name"]]) for s in sess):
            items = []
            for i, s in enumerate(sess):
                d = INPUTS[s["name"]]
                if s["at"] >= len(d):
                    continue
                k = s["step"] if s["step"] else int(rng.choice([0, 1, 50, 400, 3000]))
                if (steps + i) % 5 == 0:
                    k = 0                                          # a step without bytes
                chunk = d[s["at"]:s["at"] + k]
                s["at"] += len(chunk)
                ch = s["st"].push(chunk, finished=s["at"] >= len(d))     # (k == 0 leaves `at` short of the end)
                s["per"].append(ch.granules)
                if ch.granules and s["state"] is None:
                    s["state"] = mp3.stream_state(ch.channels, dev)
                if ch.granules:
                    items.append((ch, s["state"], s["dst"], s["written"], s["dst"].shape[1]))
                s["written"] += ch.written
                s["released"] += ch.released
            arena.clear()
            n_rec, _ = mp3.decode_stream_batch(arena, items, mono)
            assert n_rec == sum(len(it[0].rec) for it in items)
            steps += 1
        torch.cuda.synchronize()
        seen = set()
        for s in sess:
            got = s["dst"].cpu().numpy()
            w = want[s["name"]].reshape(got.shape[0], -1)
            assert s["released"] == w.shape[1], s["name"]
            assert np.array_equal(_bits(got[:, :w.shape[1]]), _bits(w)), (s["name"], mono)
            assert np.all(got[:, s["written"]:] == np.float32(-777.25)), s["name"]     # nothing past what was written
            seen |= {min(g, 2) for g in s["per"]}
            s["st"].close()
        assert seen == {0, 1, 2} and steps > 10                    # steps of zero, one and many granules all occurred


@pytest.mark.parametrize("name", EXAMPLES)
def test_join_on_the_device(model, name):
    """A stream joined at frames 40 / 41 / 100 (and 100 bytes into frames 40 and 100): from the third decoded granule on, the output
    is the whole-file decode at the same absolute positions.  Exactly the first 1152 samples after the join -- two granules formed
    against an empty history instead of the stream's -- are left out of the comparison; they are finite."""
    d = INPUTS[name]
    fr = R.frames(d)
    want, _ = _whole(name, model.device, True)
    for start, off in ((40, 0), (41, 0), (100, 0), (40, 100), (100, 100)):
        cut = d[fr[start][0] + off:]
        k = first_decodable(d, fr, start + (1 if off else 0))
        sizes = chunkings(len(cut), False)["2560" if start != 41 else "random1"]
        got, info = _stream(cut, sizes, model.device, True, join=True)
        assert info["frames"] == len(fr) - k and got.shape[0] == (len(fr) - k) * 1152
        assert np.array_equal(_bits(got[1152:]), _bits(want[k * 1152 + 1152:])), (name, start, off)
        assert np.isfinite(got[:1152]).all()


# ---- the pools ----------------------------------------------------------------------------------------------------------------------
def _args(kind, ms, sr):
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.agent_text import StreamSpeechASRAgent, StreamSpeechS2TTAgent
    return RF.agent_args({"asr": StreamSpeechASRAgent, "s2tt": StreamSpeechS2TTAgent, "s2st": StreamSpeechS2STAgent}[kind], ms, sr)


def _run_pairs(pool, kinds, d, model):
    """For every kind: an MP3-fed session, a twin fed the whole-file decode's samples as f32le, and a list-fed third, in ONE pool.
    The MP3 sessions get 2560-byte chunks (320 ms); after each push the twins get exactly the samples the MP3 session gained."""
    from streamspeech_amd import pcm
    from streamspeech_amd.simuleval_shim import SpeechSegment
    names = [EXAMPLES[i % len(EXAMPLES)] for i in range(len(kinds))]
    want = [_whole(n, model.device, True)[0] for n in names]
    trio = []
    for kind in kinds:
        out = "s16le" if kind == "s2st" else None
        trio.append((pool.open(kind, _args(kind, 320, 48000), dicts=d, mp3_in=True, pcm_out=out),
                     pool.open(kind, _args(kind, 320, 48000), dicts=d, pcm_in=pcm.PcmFormat("f32le"), pcm_out=out),
                     pool.open(kind, _args(kind, 320, 48000), dicts=d, pcm_out=out)))
    at, pos = [0] * len(kinds), [0] * len(kinds)
    steps = writes = 0
    while any(at[i] < len(INPUTS[names[i]]) for i in range(len(kinds))):
        live, segs, pushed = [], {}, 0
        for i, (m, p, l) in enumerate(trio):
            data = INPUTS[names[i]]
            if at[i] >= len(data):
                continue
            chunk = data[at[i]:at[i] + 2560]
            at[i] += len(chunk)
            fin = at[i] >= len(data)
            pushed += len(chunk)
            pool.push_mp3(m, chunk, finished=fin)
            gained = pool.sessions[m].mp3_chunk.released
            x = want[i][pos[i]:pos[i] + gained]
            assert len(x) == gained
            pos[i] += gained
            pool.push_pcm(p, x, finished=fin)
            segs[l] = SpeechSegment(content=x.astype(np.float64).tolist(), sample_rate=48000, finished=fin)
            live.append(i)
        out = pool.step(segs)
        ls = pool.last_step
        assert ls["mp3_uploads"] == 1 and ls["mp3_synth_calls"] == 1 and ls["pcm_uploads"] == 1, steps
        assert ls["mp3_granules"] > 0 and ls["mp3_bytes_in"] == pushed and ls["sessions"] == 3 * len(live)
        for i in live:
            m, p, l = trio[i]
            a, b, c = out[m], out[p], out[l]
            assert type(a) is type(b) and (a.is_empty, a.content, bool(a.finished)) == (b.is_empty, b.content, bool(b.finished)), (steps, i)
            assert (a.is_empty, a.content, bool(a.finished)) == (c.is_empty, c.content, bool(c.finished)), (steps, i)
            writes += bool(a.content)
            sa, sb = pool.sessions[m], pool.sessions[p]
            assert sa.fe.n_pcm == sb.fe.n_pcm
            if sa.fe._dev is not None and sa.fe.n_pcm:              # (a finished agent has reset its extractor)
                n = sa.fe.n_pcm
                assert sa.fe.n_pcm == pos[i]
                assert torch.equal(sa.fe._dev[:n].view(torch.int32), sb.fe._dev[:n].view(torch.int32)), (steps, i)
        steps += 1
    assert all(pos[i] == len(want[i]) for i in range(len(kinds)))
    return steps, writes


def test_text_pool_mp3_sessions_equal_pcm_and_list_twins(model, synth_weights):
    from streamspeech_amd.text_pool import TextSessionPool
    pool = TextSessionPool(model, 8, 512)
    steps, writes = _run_pairs(pool, ["asr", "s2tt"], RF.dictionaries(synth_weights[0]), model)
    assert steps > 8 and writes > 0


def test_speech_pool_mp3_in_pcm_out(model, hip_vocoder, synth_weights):
    from streamspeech_amd.speech_pool import SpeechSessionPool
    pool = SpeechSessionPool(model, 8, 512, vocoder=hip_vocoder)
    steps, writes = _run_pairs(pool, ["s2st", "asr"], RF.dictionaries(synth_weights[0]), model)
    assert steps > 8 and writes > 0
