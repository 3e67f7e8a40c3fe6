"""Writes tests/golden/offline_beam.json: the reference's offline generator (CTCMultiDecoderSequenceGenerator, built as
oracle/ref_offline.build_generator builds it but with beam_size_mt = k, --unkpen and --unnormalized) on seeded synthetic
utterances, B = 1 samples.  Per sample: the A-/S-/D- lines, the full first-pass n-best list (tokens, scores, positional
scores), the unit string and a decisive margin.  Run where the reference tree exists:
    python -m tests.make_golden_beam

Decisive margin: BeamSearch.step is wrapped (it still runs unmodified) to see, at every step, the candidate scores the search
sorts.  The smallest gap that decides an outcome is recorded: around the k-th candidate (which </s> candidates may finalise),
around the k-th non-</s> candidate (which hypotheses stay active), and between adjacent final hypothesis scores (their order).
An utterance is pinned when that margin exceeds tau = 1e-4 + 1e-6 * |score| (the largest score magnitude next to a gap):
no float32 difference of that size between two implementations can change its search.

Group (b) needs hypotheses that end before max_len; the seed-0 model never emits </s> early, so its state dict is perturbed
in one documented way: the </s> row of the tied target_unigram_decoder.embed_tokens.weight is multiplied by EOS_SCALE."""
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import kaldi_fbank as K  # noqa: E402
from oracle import ref_agent, ref_offline as RO  # noqa: E402
from streamspeech_amd import synth  # noqa: E402
from streamspeech_amd.config import ModelConfig  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "offline_beam.json")
EOS_KEY = "target_unigram_decoder.embed_tokens.weight"
# (name, beam, max_len_b_mt, unk_penalty, normalize, eos_scale)
GROUPS = [("beam4", 4, 10, 0.0, True, 1.0),
          ("beam10_early_eos", 10, 16, 0.0, True, 3.0),
          ("beam5_unnorm_unkpen", 5, 10, 0.5, False, 1.0)]
CANDIDATES = [(200 + i, 700 + i, 12800 + 3200 * (i % 7)) for i in range(16)]   # (sample id, pcm seed, samples)
MIN_PINNED = 6


def sample_pcm(seed, n):
    return synth.synth_pcm(seed, n)


def state_dict(eos_scale, cfg):
    sd = synth.make_model_state_dict(0, cfg)
    if eos_scale != 1.0:
        w = np.array(sd[EOS_KEY], copy=True)
        w[cfg.eos] *= np.float32(eos_scale)
        sd[EOS_KEY] = w
        sd[EOS_KEY.replace("embed_tokens", "output_projection")] = w      # the checkpoint ties the two (same array)
    return sd


def build_generator(sd, cfg, beam, max_len_b_mt, unk_penalty, normalize):
    """oracle/ref_offline.build_generator with the first-pass beam, --unkpen and --unnormalized (pred.offline-s2st.sh)."""
    RO._install()
    dicts = ref_agent.make_dicts(cfg)
    model = ref_agent.build_model(sd, cfg, False, dicts)
    from types import SimpleNamespace
    model.multitask_decoders = {k: SimpleNamespace(encoder=SimpleNamespace(dictionary=dicts[k]))
                                for k in ("source_unigram", "ctc_target_unigram")}
    Gen = RO._STATE["multi"].CTCMultiDecoderSequenceGenerator
    g = Gen([model], dicts["tgt"], dicts["target_unigram"], beam_size=1, beam_size_mt=beam, max_len_a=0, max_len_b=200,
            max_len_a_mt=0.0, max_len_b_mt=max_len_b_mt,
            max_len=model.max_decoder_positions() if hasattr(model, "max_decoder_positions") else 1024,
            min_len=1, normalize_scores=normalize, unk_penalty=unk_penalty, eos=dicts["tgt"].eos(),
            eos_mt=dicts["target_unigram"].eos(), symbols_to_strip_from_output={dicts["tgt"].eos()})
    return g, model, dicts


def tau(score):
    return 1e-4 + 1e-6 * abs(score)


class MarginProbe:
    """Wraps search.step (calls it unchanged) and collects the decisive gaps of every step."""

    def __init__(self, search, beam, eos):
        self.search, self.k, self.eos = search, beam, eos
        self.orig = search.step
        self.gaps = []          # (gap, score magnitude next to it)
        self.eos_steps = set()
        search.step = self

    def __call__(self, step, lprobs, scores, *a, **kw):
        out = self.orig(step, lprobs, scores, *a, **kw)
        bsz, beam, V = lprobs.size()
        lp = lprobs[:, ::beam, :] if step == 0 else lprobs + scores[:, :, step - 1].unsqueeze(-1)
        s, idx = torch.topk(lp.reshape(bsz, -1), k=min(4 * self.k, lp.reshape(bsz, -1).size(1) - 1))
        tok = idx.fmod(V)
        for b in range(bsz):
            sv, tv = s[b].tolist(), tok[b].tolist()
            self._gap(sv, self.k - 1)
            non = [x for x, t in zip(sv, tv) if t != self.eos]
            self._gap(non, self.k - 1)
            if any(t == self.eos and x != -math.inf for x, t in zip(sv[:self.k], tv[:self.k])):
                self.eos_steps.add(step)
        return out

    def _gap(self, v, i):
        if i + 1 < len(v) and v[i] != -math.inf:
            self.gaps.append((v[i] - v[i + 1], abs(v[i])))

    def margin(self, final_scores):
        gaps = list(self.gaps) + [(a - b, abs(a)) for a, b in zip(final_scores, final_scores[1:])]
        worst = min(gaps, key=lambda g: g[0] - tau(g[1]))
        return worst[0], tau(max(abs(x) for x in final_scores + [g[1] for g in gaps]))


def run(gen, dicts, sid, fb, beam):
    probe = MarginProbe(gen.generator_mt.search, beam, gen.generator_mt.eos)
    nbest = []
    orig = gen.generator_mt.generate_decoder

    def keep(*a, **kw):
        fin = orig(*a, **kw)
        nbest.append([{"tokens": h["tokens"].int().tolist(), "score": float(h["score"]),
                       "positional_scores": h["positional_scores"].float().tolist()} for h in fin[0]])
        return fin
    gen.generator_mt.generate_decoder = keep
    try:
        r = RO.run_sample(gen, dicts, sid, fb)
    finally:
        gen.generator_mt.generate_decoder = orig
        gen.generator_mt.search.step = probe.orig
    hyps = nbest[0]
    margin, t = probe.margin([h["score"] for h in hyps])
    return {"log": r["log"], "units": r["units"], "nbest": hyps, "margin": margin, "tau": t,
            "eos_steps": sorted(probe.eos_steps), "lengths": [len(h["tokens"]) for h in hyps]}


def main():
    cfg = ModelConfig()
    g = np.load(os.path.join(ROOT, "tests", "golden", "gcmvn_fr-en.npz"))
    torch.manual_seed(0)
    out = {"note": "reference offline generator with beam_size_mt = k (tests/make_golden_beam.py); regenerate with python -m tests.make_golden_beam",
           "eos_key": EOS_KEY, "groups": {}}
    for name, beam, mlb, unkpen, norm, scale in GROUPS:
        sd = state_dict(scale, cfg)
        gen, _, dicts = build_generator(sd, cfg, beam, mlb, unkpen, norm)
        recs, pinned = {}, 0
        for sid, seed, n in CANDIDATES:
            fb = K.global_cmvn(K.fbank(sample_pcm(seed, n) * np.float32(32768.0)), g["mean"], g["std"])
            rec = run(gen, dicts, sid, fb, beam)
            rec.update({"pcm_seed": seed, "n_samples": n})
            recs[str(sid)] = rec
            pinned += rec["margin"] > rec["tau"]
            print(name, sid, "margin %.3g tau %.3g" % (rec["margin"], rec["tau"]), "eos steps", rec["eos_steps"],
                  "lengths", rec["lengths"], flush=True)
            if pinned >= MIN_PINNED:
                break
        assert pinned >= MIN_PINNED, f"{name}: only {pinned} utterances above the margin"
        out["groups"][name] = {"beam": beam, "max_len_b_mt": mlb, "unk_penalty": unkpen, "normalize": norm, "eos_scale": scale,
                               "hypotheses": recs}
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump(out, f, indent=0, ensure_ascii=False)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
