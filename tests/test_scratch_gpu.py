"""Scratch sets as objects of their own (ss_scratch_*): weight handles of several languages run on ONE scratch set,
with the bits they have on scratch sets of their own; trim releases the activations and the next call re-grows them; a cap turns
growth past it into SS_ERR_SCRATCH_CAP and leaves the set usable.  Reference shape: one model per language directory
(configs/{fr,es,de}-en/, agent/speech_to_speech.streamspeech.agent.py:357-401), all resident in one process."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def languages():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import synth
    from streamspeech_amd.config import ModelConfig, VocoderConfig
    from streamspeech_amd.engine import HipModel, HipVocoder
    cfg, vcfg = ModelConfig(), VocoderConfig()
    out = []
    for seed in (0, 1, 2):
        out.append((HipModel(synth.make_model_state_dict(seed, cfg), cfg), HipVocoder(synth.make_vocoder_state_dict(seed, vcfg), vcfg)))
    return out


def _batch(n=6, seed0=300):
    from streamspeech_amd import synth, workload
    utts = sorted(workload.make_utterances(40), key=lambda u: u.seconds)[4:4 + n]
    pcm = torch.cat([torch.from_numpy(synth.synth_pcm(seed0 + u.idx, u.n_samples)) for u in utts]).cuda()
    return utts, pcm


def _run(m, v, utts, pcm):
    from streamspeech_amd import workload
    wavs, asr, st, toks = workload.run_batch(m, v, pcm, utts)
    return [w.clone() for w in wavs], asr, st, toks


def test_three_languages_share_one_scratch_set_bit_for_bit(languages):
    from streamspeech_amd.engine import Scratch
    utts, pcm = _batch()
    own = [_run(m, v, utts, pcm) for m, v in languages]                   # every handle on the scratch set it was created with
    assert own[0][1] != own[1][1] or own[0][3] != own[1][3]               # different weights do give different ids
    shared = Scratch()
    handles = [(m.new_context(scratch=shared), v.new_context(scratch=shared)) for m, v in languages]
    for rep in range(2):                                                  # interleaved: fr, es, de, fr, es, de on the same set
        for (m, v), ref in zip(handles, own):
            wavs, asr, st, toks = _run(m, v, utts, pcm)
            assert asr == ref[1] and st == ref[2] and toks == ref[3]
            assert all(torch.equal(a, b) for a, b in zip(wavs, ref[0]))
    # one set holds what ONE language's pack needs, not three times that
    lone = Scratch()
    m0, v0 = languages[0][0].new_context(scratch=lone), languages[0][1].new_context(scratch=lone)
    _run(m0, v0, utts, pcm)
    assert shared.bytes() <= 1.05 * lone.bytes() + (64 << 20), (shared.bytes(), lone.bytes())


def test_trim_releases_and_the_next_call_regrows(languages):
    from streamspeech_amd.engine import Scratch
    utts, pcm = _batch(4, 400)
    sc = Scratch()
    m, v = languages[0][0].new_context(scratch=sc), languages[0][1].new_context(scratch=sc)
    ref = _run(m, v, utts, pcm)
    grown = sc.bytes()
    assert grown > (128 << 20)
    free0 = torch.cuda.mem_get_info()[0]
    sc.trim(0)
    assert sc.bytes() < (64 << 20) and torch.cuda.mem_get_info()[0] - free0 > 0.8 * (grown - sc.bytes())
    again = _run(m, v, utts, pcm)
    assert again[1:] == ref[1:] and all(torch.equal(a, b) for a, b in zip(again[0], ref[0]))
    sc.trim(grown)                                                        # keep_bytes above what is held: nothing to do
    assert sc.bytes() >= 0.9 * grown


def test_cap_is_a_clean_error_and_the_set_stays_usable(languages):
    from streamspeech_amd.engine import Scratch
    utts, pcm = _batch(4, 500)
    sc = Scratch(cap_bytes=64 << 20)                                      # room for the fixed pieces (25-MB MT cache, token chain), not for a pack's activations
    m, v = languages[0][0].new_context(scratch=sc), languages[0][1].new_context(scratch=sc)
    with pytest.raises(RuntimeError, match="cap"):
        _run(m, v, utts, pcm)
    assert sc.bytes() <= (64 << 20)
    sc.set_cap(0)
    ref = _run(*languages[0], utts, pcm)
    got = _run(m, v, utts, pcm)
    assert got[1:] == ref[1:] and all(torch.equal(a, b) for a, b in zip(got[0], ref[0]))


def test_stateful_sequences_live_in_the_scratch_set(languages):
    """The MT search state (KV cache, length) belongs to the scratch set: a second handle bound to the same set continues nothing --
    it starts its own sequence with mt_begin -- and the first handle's finished results are unaffected."""
    from streamspeech_amd import synth
    from streamspeech_amd.engine import Scratch
    from streamspeech_amd.pipeline import mt_greedy
    sc = Scratch()
    m_fr, m_es = languages[0][0].new_context(scratch=sc), languages[1][0].new_context(scratch=sc)
    fb = torch.from_numpy(synth.synth_fbank(77, 231)).cuda()
    enc_fr, enc_es = m_fr.encoder_forward(fb), m_es.encoder_forward(fb)
    t_fr, f_fr = mt_greedy(m_fr, enc_fr, max_new_tokens=9)
    f_fr = f_fr.clone()
    t_es, _ = mt_greedy(m_es, enc_es, max_new_tokens=9)
    t_fr2, f_fr2 = mt_greedy(m_fr, enc_fr, max_new_tokens=9)
    assert t_fr2 == t_fr and torch.equal(f_fr2, f_fr)
    assert t_es == mt_greedy(languages[1][0], languages[1][0].encoder_forward(fb), max_new_tokens=9)[0]


# ---- the booking contract under the incremental streaming encoder (ss_encoder_stream_*) -------------------------------------------------
# Its per-set state is the largest a context keeps: per layer the q|k|v and GLU rows of every frame so far (4d floats a row) plus the
# finished output rows, es_cap rows each.  es_cap grows to min(max_rel_pos, max(2 T2, 256)) rows when a call has T2 > es_cap
# (ss_encoder_stream_forward); these tests mirror that rule.

def _es_cap_after(cap, T2, max_rel_pos):
    return cap if T2 <= cap else min(max_rel_pos, max(2 * T2, 256))


def _state_bytes(cfg, rows):
    return cfg.enc_layers * rows * 4 * cfg.enc_dim * 4                # q|k|v + GLU rows of every layer, float32 (the output rows come on top)


def _keeps_books(sc, what):
    booked, held = sc.audit()                                         # raises if a buffer of the set is booked under another account
    assert booked == held == sc.bytes(), (what, booked, held, sc.bytes())


def test_streaming_growth_is_booked(languages):
    """Every growth of the streaming state shows in ss_scratch_bytes: the first by at least the state it allocates, a later one by at
    least the rows it adds (the old buffers go once their final rows are copied)."""
    from streamspeech_amd import synth
    from streamspeech_amd.engine import Scratch
    sc = Scratch()
    m = languages[0][0].new_context(scratch=sc)
    max_rel_pos = m._dims[0]
    fb_all = torch.from_numpy(synth.synth_fbank(61, 1300)).to(m.device)
    Ts = list(range(40, 1300, 48)) + [1300]
    m.encoder_forward(fb_all, 8, 8)                                   # activations and attention scratch at their largest first: what
    cap, growths = 0, 0                                               # the stream grows below is its own state
    grown0 = sc.bytes()
    m.encoder_stream_reset()
    for T in Ts:
        T2 = m.encoder_out_len(T)
        new_cap = _es_cap_after(cap, T2, max_rel_pos)
        before = sc.bytes()
        m.encoder_stream_forward(fb_all[:T].contiguous(), 8, 8)
        if new_cap > cap:
            grew = sc.bytes() - before
            assert grew >= _state_bytes(m.cfg, new_cap - cap), (T, cap, new_cap, grew)
            growths += 1
        cap = new_cap
    assert growths >= 2 and cap > 256
    assert sc.bytes() >= grown0 + _state_bytes(m.cfg, cap)
    m.encoder_stream_reset()


def test_streaming_under_a_cap(languages):
    """A streaming call that must grow past the cap is refused with SS_ERR_SCRATCH_CAP and changes nothing: the set holds the same
    bytes, and the stream goes on from where it was once the cap is raised -- the same final rows, bit for bit, as a stream that never
    met the cap, and every output within the streaming bar of the full recompute."""
    from streamspeech_amd import synth
    from streamspeech_amd import lib as L
    from streamspeech_amd.engine import Scratch
    base = languages[0][0]
    sc = Scratch()
    m, ref_m = base.new_context(scratch=sc), base.new_context()          # ref_m: the same launch-per-op form on a set of its own
    max_rel_pos = m._dims[0]
    fb_all = torch.from_numpy(synth.synth_fbank(62, 1300)).to(m.device)
    Ts = list(range(40, 1300, 48)) + [1300]
    ref_m.encoder_stream_reset()
    ref = []
    for T in Ts:
        ref.append((ref_m.encoder_stream_forward(fb_all[:T].contiguous(), 8, 8).clone(), ref_m.stream_stats))
    cap, refused = 0, 0
    m.encoder_stream_reset()
    for i, T in enumerate(Ts):
        fb = fb_all[:T].contiguous()
        T2 = m.encoder_out_len(T)
        new_cap = _es_cap_after(cap, T2, max_rel_pos)
        if cap > 0 and new_cap > cap and not refused:                    # part way: this call must grow the state
            held, stats = sc.bytes(), m.stream_stats
            sc.set_cap(held + (1 << 20))
            with pytest.raises(L.StreamSpeechHipError, match="cap") as e:
                m.encoder_stream_forward(fb, 8, 8)
            assert e.value.code == L.SS_ERR_SCRATCH_CAP
            assert sc.bytes() == held and m.stream_stats == stats
            raised = held + 2 * _state_bytes(m.cfg, new_cap) + (64 << 20)   # room for the new state next to the old one while rows move
            sc.set_cap(raised)
            refused = 1
            out = m.encoder_stream_forward(fb, 8, 8)                          # the same call again
            assert held + _state_bytes(m.cfg, new_cap - cap) <= sc.bytes() <= raised
        else:
            out = m.encoder_stream_forward(fb, 8, 8)
        cap = new_cap
        ref_out, ref_stats = ref[i]
        assert m.stream_stats == ref_stats, (T, m.stream_stats, ref_stats)
        nf = ref_stats[0]
        assert torch.equal(out[:nf], ref_out[:nf]), T
        full = m.encoder_forward(fb, 8, 8)
        assert (out - full).abs().max().item() < 5e-5, T
    assert refused
    sc.set_cap(0)
    m.encoder_stream_reset()


def test_trim_mid_stream_starts_the_stream_over(languages):
    from streamspeech_amd import synth
    from streamspeech_amd.engine import Scratch
    sc = Scratch()
    m = languages[0][0].new_context(scratch=sc)
    fb_all = torch.from_numpy(synth.synth_fbank(63, 900)).to(m.device)
    Ts = list(range(40, 900, 40)) + [900]
    m.encoder_stream_reset()
    for i, T in enumerate(Ts):
        fb = fb_all[:T].contiguous()
        if i == len(Ts) // 2:
            assert m.stream_stats[0] > 0                                   # rows are final: the next call would start from them
            held = sc.bytes()
            sc.trim(0)
            trimmed = sc.bytes()
            assert trimmed < held - _state_bytes(m.cfg, 256)
            _keeps_books(sc, "trim")
        out = m.encoder_stream_forward(fb, 8, 8)
        if i == len(Ts) // 2:
            assert m.stream_stats[1] == m.encoder_out_len(T)               # every row computed afresh: nothing served from before the trim
            assert sc.bytes() >= trimmed + _state_bytes(m.cfg, 256)        # the state is back, and booked
        assert (out - m.encoder_forward(fb, 8, 8)).abs().max().item() < 5e-5, T
        _keeps_books(sc, f"stream T={T}")
    m.encoder_stream_reset()


def test_every_entry_point_keeps_the_books(languages):
    """ss_debug_scratch_audit after every entry-point family on ONE set: the bytes the set books are the bytes its buffers hold, and
    no buffer of it is booked under another account (or none)."""
    from streamspeech_amd import synth
    from streamspeech_amd.engine import Scratch
    sc, other = Scratch(), Scratch()
    m, v = languages[0][0].new_context(scratch=sc), languages[0][1].new_context(scratch=sc)
    _keeps_books(sc, "bind")
    cfg = m.cfg
    fb = torch.from_numpy(synth.synth_fbank(64, 331)).to(m.device)
    enc = m.encoder_forward(fb)
    m.encoder_forward(fb, 8, 8)
    _keeps_books(sc, "encoder_forward")
    for head in (0, 1):
        m.ctc_greedy(head, enc)
    m.ctc_greedy(1, enc, want_logits=True)
    _keeps_books(sc, "ctc_greedy")
    for wg in (0, 64):
        m.set_persistent_mt_step(wg)
        m.mt_begin(enc)
        _, nx = m.mt_append([cfg.eos], 0, True, False)
        m.mt_append([nx], 1, False, False)
        _keeps_books(sc, f"mt_begin / mt_append persistent={wg}")
        toks, feats = m.mt_greedy(enc, [], max_len=12)
        _keeps_books(sc, f"mt_greedy persistent={wg}")
    m.t2u_units(feats)
    _keeps_books(sc, "t2u_units")
    utts, pcm = _batch(4, 600)
    _run(m, v, utts, pcm)
    _keeps_books(sc, "run_batch")
    v.forward(list(range(3, 40)))
    _keeps_books(sc, "vocoder_forward")
    v.batch_forward([list(range(5, 30)), list(range(100, 140))])
    _keeps_books(sc, "batch_vocoder_forward")
    fb_all = torch.from_numpy(synth.synth_fbank(65, 1200)).to(m.device)
    for persistent in (64, 0):
        m.set_persistent_mt_step(persistent)
        m.encoder_stream_reset()
        for T in list(range(40, 1200, 64)) + [1200]:                    # T2 up to 299 rows: the state grows twice
            m.encoder_stream_forward(fb_all[:T].contiguous(), 8, 8)
            _keeps_books(sc, f"encoder_stream_forward T={T} persistent={persistent}")
    for keep in (sc.bytes() // 2, 0):
        sc.trim(keep)
        _keeps_books(sc, f"trim({keep})")
    m.encoder_stream_forward(fb_all[:300].contiguous(), 8, 8)
    m.bind_scratch(other)
    _keeps_books(sc, "left by the handle")
    m.encoder_stream_forward(fb_all[:300].contiguous(), 8, 8)
    _keeps_books(other, "other set")
    m.bind_scratch(sc)
    _keeps_books(other, "left by the handle")
    m.encoder_stream_reset()
    m.encoder_stream_forward(fb_all[:500].contiguous(), 8, 8)
    _keeps_books(sc, "rebound, reset, streamed")
    m.encoder_stream_reset()
