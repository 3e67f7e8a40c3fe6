"""Beam search of the offline first-pass text decoder on the GPU (ss_batch_mt_beam, beam.hip) against the reference's offline
generator with beam_size_mt = k (fixture tests/golden/offline_beam.json, written by tests/make_golden_beam.py): identical n-best
token lists and order, scores within tau / 4 for every utterance whose decisive margin exceeds tau; the driver's A-/S-/D- lines
and unit strings.  Beam 1 gives the greedy twin's tokens and decoder states; an utterance's n-best list is the same alone, in
mixed packs and across a split of more than 256 rows; the scratch books hold; bad arguments are refused before any launch."""
import ctypes as C
import json
import os
import struct

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = os.path.join(ROOT, "tests", "golden", "offline_beam.json")


def _fix():
    return json.load(open(FIX, encoding="utf-8"))


def _model_for(group, hip_model, synth_weights):
    if group["eos_scale"] == 1.0:
        return hip_model
    from streamspeech_amd.engine import HipModel
    from tests.make_golden_beam import state_dict
    cfg = synth_weights[0]
    g = np.load(os.path.join(ROOT, "tests", "golden", "gcmvn_fr-en.npz"))
    return HipModel(state_dict(group["eos_scale"], cfg), cfg, cmvn_mean=g["mean"], cmvn_std=g["std"])


def _encode(model, pcms):
    lens = [int(p.numel()) for p in pcms]
    feat, T = model.batch_fbank_cmvn(torch.cat(pcms).cuda(), lens)
    enc, Tp = model.batch_encoder_forward(feat, T)
    return enc, Tp


def _pcm(rec):
    from tests.make_golden_beam import sample_pcm
    return torch.from_numpy(sample_pcm(rec["pcm_seed"], rec["n_samples"]))


def _bits(x):
    return struct.pack("<f", x)


@pytest.mark.parametrize("name", ["beam4", "beam10_early_eos", "beam5_unnorm_unkpen"])
def test_beam_nbest_equals_reference(name, hip_model, synth_weights, tmp_path):
    from streamspeech_amd import offline
    from oracle.ref_agent import make_dicts
    grp = _fix()["groups"][name]
    model = _model_for(grp, hip_model, synth_weights)
    ids = list(grp["hypotheses"])
    recs = [grp["hypotheses"][i] for i in ids]
    enc, Tp = _encode(model, [_pcm(r) for r in recs])
    nbest, _, _ = model.batch_mt_beam(enc, Tp, [grp["max_len_b_mt"]] * len(ids), grp["beam"], 1, grp["unk_penalty"], grp["normalize"])
    worst, under = 0.0, []
    for sid, rec, hyps in zip(ids, recs, nbest):
        if not rec["margin"] > rec["tau"]:
            under.append(sid)
            continue
        ref = rec["nbest"]
        assert [h["tokens"] for h in hyps] == [h["tokens"] for h in ref], f"{name} sample {sid}: n-best tokens / order"
        for h, r in zip(hyps, ref):
            d = abs(h["score"] - r["score"])
            worst = max(worst, d)
            assert d < rec["tau"] / 4, f"{name} sample {sid}: score {h['score']} vs {r['score']}"
            assert np.abs(np.array(h["positional_scores"]) - np.array(r["positional_scores"])).max() < rec["tau"]
    print(f"{name}: worst |HIP - reference| score {worst:.3g}; utterances under the margin (not compared): {len(under)} {under}")
    assert len(ids) - len(under) >= 6
    # the driver: A-/S-/D- lines (D- from hypothesis 0) and unit strings
    dicts = make_dicts(model.cfg)
    items = [(int(i), _pcm(r).cuda()) for i, r in zip(ids, recs)]
    hyps = offline.generate(model, None, items, dicts, str(tmp_path), "test", max_len_b_mt=grp["max_len_b_mt"], dump_wav=False,
                            beam_mt=grp["beam"], unk_penalty=grp["unk_penalty"], normalize=grp["normalize"])
    log = open(tmp_path / "generate-test.log", encoding="utf-8").read().splitlines()
    for sid, rec in zip(ids, recs):
        if sid in under:
            continue
        assert [ln for ln in log if ln.split("\t")[0] in (f"A-{sid}", f"S-{sid}", f"D-{sid}")] == rec["log"]
        assert hyps[int(sid)]["units"] == rec["units"]


def test_beam1_is_greedy(hip_model):
    from tests.offline_fixture import load
    from oracle.make_golden_offline import sample_pcm
    fix = load()
    pcms = [torch.from_numpy(sample_pcm(s["pcm_seed"], s["n_samples"])) for s in fix["samples"]]
    enc, Tp = _encode(hip_model, pcms)
    for ml in (10, 40):
        mx = [ml] * len(Tp)
        toks, feats, n = hip_model.batch_mt_greedy(enc, Tp, mx)
        nbest, bfeats, bn = hip_model.batch_mt_beam(enc, Tp, mx, 1)
        assert [h[0]["tokens"] for h in nbest] == toks
        assert bn == n
        for b in range(len(Tp)):
            assert torch.equal(bfeats[b, :n[b]], feats[b, :n[b]])


def _synthetic(n, seed0):
    from streamspeech_amd import synth, workload
    utts = sorted(workload.make_utterances(60), key=lambda u: u.seconds)[:n]
    return [torch.from_numpy(synth.synth_pcm(seed0 + u.idx, u.n_samples)) for u in utts]


def test_beam_pack_invariance_and_split(hip_model):
    pcms = _synthetic(30, 900)
    enc, Tp = _encode(hip_model, pcms)
    off = np.concatenate([[0], np.cumsum(Tp)])
    beam, ml = 10, 12
    mx = [ml + (b % 3) for b in range(len(Tp))]          # mixed max lengths too

    def key(h):
        return [(x["tokens"], _bits(x["score"]), [_bits(p) for p in x["positional_scores"]]) for x in h]
    whole, wf, wn = hip_model.batch_mt_beam(enc, Tp, mx, beam)           # 300 rows: split 25 + 5
    for b in (0, 7, 26, 29):
        alone, af, an = hip_model.batch_mt_beam(enc[off[b]:off[b + 1]], [Tp[b]], [mx[b]], beam)
        assert key(alone[0]) == key(whole[b]), f"utterance {b}: alone vs in a split pack of {len(Tp)}"
        assert an[0] == wn[b] and torch.equal(af[0, :an[0]], wf[b, :wn[b]])
    sel = [26, 3, 11]                                                 # a pack of mixed lengths in another order
    enc3 = torch.cat([enc[off[b]:off[b + 1]] for b in sel])
    three, _, _ = hip_model.batch_mt_beam(enc3, [Tp[b] for b in sel], [mx[b] for b in sel], beam)
    for j, b in enumerate(sel):
        assert key(three[j]) == key(whole[b])


def test_beam_keeps_scratch_books_and_cap(hip_model):
    from streamspeech_amd import lib as L
    from streamspeech_amd.engine import Scratch
    pcms = _synthetic(6, 950)
    sc = Scratch()
    m = hip_model.new_context(scratch=sc)
    enc, Tp = _encode(m, pcms)
    booked0, _ = sc.audit()
    ref, rf, rn = m.batch_mt_beam(enc, Tp, [12] * len(Tp), 8)
    booked, held = sc.audit()
    assert booked == held and booked > booked0
    sc.trim(0)
    sc.set_cap(sc.bytes() + (1 << 20))                                   # below what the beam call needs (enc is a torch tensor)
    with pytest.raises(L.StreamSpeechHipError) as e:
        m.batch_mt_beam(enc, Tp, [12] * len(Tp), 8)
    assert e.value.code == L.SS_ERR_SCRATCH_CAP
    booked, held = sc.audit()
    assert booked == held
    sc.set_cap(0)
    got, gf, gn = m.batch_mt_beam(enc, Tp, [12] * len(Tp), 8)
    assert got == ref and gn == rn
    assert all(torch.equal(gf[b, :gn[b]], rf[b, :rn[b]]) for b in range(len(Tp)))


def test_beam_argument_codes(hip_model):
    from streamspeech_amd import lib as L
    from streamspeech_amd.engine import Scratch
    sc = Scratch()
    m = hip_model.new_context(scratch=sc)
    enc, Tp = _encode(m, _synthetic(1, 990))
    lib = L.load()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    before = sc.bytes()
    feats = torch.zeros((1, 16, m.cfg.dec_dim), device="cuda")
    out = (C.c_int32 * (33 * 15 * 260))()
    n = (C.c_int32 * (33 * 260))()
    s = (C.c_float * (33 * 260))()

    def call(B, beam):
        tp = (C.c_int32 * B)(*([Tp[0]] * B))
        ml = (C.c_int32 * B)(*([10] * B))
        return lib.ss_batch_mt_beam(m.h, stream, B, beam, C.c_void_p(enc.data_ptr()), tp, ml, 1, 0.0, 1, out, 15, n, s, None,
                                    C.c_void_p(feats.data_ptr()), 16)
    assert call(1, 0) == L.SS_ERR_ARG
    assert call(1, 33) == L.SS_ERR_ARG
    assert call(0, 4) == L.SS_ERR_ARG
    assert call(65, 4) == 4                 # SS_ERR_CAPACITY: B * beam = 260 > 256
    assert call(9, 32) == 4
    torch.cuda.synchronize()
    assert sc.bytes() == before and torch.count_nonzero(feats) == 0
