"""Writes tests/golden/search_options.json: the reference's offline generator, built as tests/make_golden_beam.py builds it, with the
three search controls of its first-pass generator set -- len_penalty, temperature and no_repeat_ngram_size (what
speech_to_speech_ctc.build_generator passes on from --lenpen, --temperature and --no-repeat-ngram-size).  Run where the reference
tree exists:
    python -m tests.make_golden_search_options

The generator is built by make_golden_beam.build_generator and the controls are then set on its generator_mt the way its own
__init__ sets them (self.len_penalty, self.temperature, self.repeat_ngram_blocker = NGramRepeatBlock(n)).

One thing is not taken as it lies.  The reference's generator hands NGramRepeatBlock its whole token buffer, [rows, max_len + 2] and
pad-filled behind the current step.  The block's compiled extension indexes that buffer by `step` and so compares against
tokens[step - n + 2 .. step]; its Python path, the only one that runs without the extension, takes "the last n - 1 tokens" of the
row it is given, which are pads there, and bans nothing.  The rule the project implements is the extension's (and what the Python
path computes on a row that ends at the current step), so this script gives the reference's own NGramRepeatBlock(n,
use_extension=False) the rows cut to tokens[:, :step + 1].  The block's code runs unmodified.

Groups (beam, max_len_b_mt, eos_scale as in make_golden_beam):
    beam4_ngram2                          beam 4,  n = 2, max_len_b_mt 10
    beam5_ngram3_lenpen0.6                beam 5,  n = 3, len_penalty 0.6
    beam10_early_eos_lenpen1.5_temp1.7    beam 10, eos_scale 3, max_len_b_mt 16, len_penalty 1.5, temperature 1.7: hypotheses of
                                          different lengths compete and the penalty decides their order
    beam10_early_eos_lenpen0.5_temp1.7    the same search with len_penalty 0.5.  On this model the plain length division already
                                          ranks the longer hypothesis first, and 1.5 only widens that: with it no pinned list
                                          changes its order against len_penalty 1 (scores -2.07 / -2.39 / -2.45 ... for lengths
                                          8 / 7 / 7 ... against -5.84 / -6.32 / -6.47 ...), so the order check below could not be made
                                          on that group.  With 0.5 the lengths interleave (9, 10, 8, 11, 7, 12, 13, 6, 5, 4).
    beam1_ngram2                          beam 1,  n = 2
    prefix_beam4_ngram2                   beam 4,  n = 2 behind forced prefixes of 0, 1 and 3 tokens (the first tokens of the unforced
                                          best hypothesis of the same search), as make_golden_beam_prefix builds its `on` cases
Per utterance: the n-best list (tokens, scores, positional scores), the decisive margin of make_golden_beam.MarginProbe and its tau.
An utterance is pinned when margin > tau; every group holds at least MIN_PINNED pinned utterances (cases, in the prefix group).

The script checks its own inputs: in every n-gram group hypothesis 0 of at least 4 pinned utterances differs from the same search
with n = 0 (the synthetic model repeats one token, so the ban bites), and in the early-</s> group with len_penalty 0.5 the n-best
order of at least 2 pinned utterances differs from the same search with len_penalty 1."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import kaldi_fbank as K  # noqa: E402
from oracle.ref_loader import _load_file  # noqa: E402
from streamspeech_amd.config import ModelConfig  # noqa: E402
from tests.make_golden_beam import CANDIDATES, MIN_PINNED, build_generator, sample_pcm, state_dict  # noqa: E402
from tests.make_golden_beam_prefix import run as run_prefix  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "search_options.json")
# (name, beam, max_len_b_mt, eos_scale, no_repeat_ngram_size, len_penalty, temperature, the penalty must reorder n-best lists)
GROUPS = [("beam4_ngram2", 4, 10, 1.0, 2, 1.0, 1.0, False),
          ("beam5_ngram3_lenpen0.6", 5, 10, 1.0, 3, 0.6, 1.0, False),
          ("beam10_early_eos_lenpen1.5_temp1.7", 10, 16, 3.0, 0, 1.5, 1.7, False),
          ("beam10_early_eos_lenpen0.5_temp1.7", 10, 16, 3.0, 0, 0.5, 1.7, True),
          ("beam1_ngram2", 1, 10, 1.0, 2, 1.0, 1.0, False)]
PREFIX_GROUP = ("prefix_beam4_ngram2", 4, 10, 1.0, 2, 1.0, 1.0, False)
PREFIX_LENGTHS = (0, 1, 3)
# wider than make_golden_beam's: the ban leaves near-ties among the runners-up more often
CANDIDATES = CANDIDATES + [(200 + i, 700 + i, 12800 + 3200 * (i % 7)) for i in range(16, 40)]
MIN_CHANGED_BY_BAN, MIN_REORDERED = 4, 2


class CutToStep(torch.nn.Module):
    """Gives the reference's blocker the rows as they stand at `step` (see the module docstring); the blocker itself is untouched."""

    def __init__(self, block):
        super().__init__()
        self.block = block

    def forward(self, tokens, lprobs, bsz, beam_size, step):
        return self.block(tokens[:, :step + 1], lprobs, bsz, beam_size, step)


def set_options(gen, n, len_penalty, temperature):
    """What SequenceGenerator.__init__ does with the three arguments, on the built first-pass generator."""
    block = _load_file("fairseq.ngram_repeat_block", "fairseq/fairseq/ngram_repeat_block.py").NGramRepeatBlock
    g = gen.generator_mt
    g.len_penalty, g.temperature = float(len_penalty), float(temperature)
    g.repeat_ngram_blocker = CutToStep(block(n, use_extension=False)) if n > 0 else None


def slim(rec):
    return {"nbest": rec["nbest"], "margin": rec["margin"], "tau": rec["tau"]}


def tokens_of(rec):
    return [h["tokens"] for h in rec["nbest"]]


def main():
    cfg = ModelConfig()
    g = np.load(os.path.join(ROOT, "tests", "golden", "gcmvn_fr-en.npz"))
    torch.manual_seed(0)
    out = {"note": "reference offline generator with len_penalty / temperature / no_repeat_ngram_size set "
                   "(tests/make_golden_search_options.py); regenerate with python -m tests.make_golden_search_options",
           "groups": {}}

    def fbank(seed, n):
        return K.global_cmvn(K.fbank(sample_pcm(seed, n) * np.float32(32768.0)), g["mean"], g["std"])

    for name, beam, mlb, scale, n, lenpen, temp, must_reorder in GROUPS:
        gen, _, dicts = build_generator(state_dict(scale, cfg), cfg, beam, mlb, 0.0, True)
        recs, pinned, changed, reordered = {}, 0, 0, 0
        for sid, seed, ns in CANDIDATES:
            fb = fbank(seed, ns)
            set_options(gen, n, lenpen, temp)
            rec = run_prefix(gen, sid, fb, beam, None)
            pin = rec["margin"] > rec["tau"]
            if n > 0:
                set_options(gen, 0, lenpen, temp)
                changed += pin and run_prefix(gen, sid, fb, beam, None)["nbest"][0]["tokens"] != rec["nbest"][0]["tokens"]
            if lenpen != 1.0:
                set_options(gen, n, 1.0, temp)
                reordered += pin and tokens_of(run_prefix(gen, sid, fb, beam, None)) != tokens_of(rec)
            recs[str(sid)] = dict(slim(rec), pcm_seed=seed, n_samples=ns)
            pinned += pin
            print(name, sid, "margin %.3g tau %.3g" % (rec["margin"], rec["tau"]), "lengths", [len(t) for t in tokens_of(rec)],
                  "changed", changed, "reordered", reordered, flush=True)
            if pinned >= MIN_PINNED and (n == 0 or changed >= MIN_CHANGED_BY_BAN) and (not must_reorder or reordered >= MIN_REORDERED):
                break
        assert pinned >= MIN_PINNED, f"{name}: only {pinned} utterances above the margin"
        if n > 0:
            assert changed >= MIN_CHANGED_BY_BAN, f"{name}: the ban changes hypothesis 0 of only {changed} pinned utterances"
        if must_reorder:
            assert reordered >= MIN_REORDERED, f"{name}: the length penalty reorders only {reordered} pinned n-best lists"
        out["groups"][name] = {"beam": beam, "max_len_b_mt": mlb, "eos_scale": scale, "no_repeat_ngram_size": n, "len_penalty": lenpen,
                               "temperature": temp, "hypotheses": recs}

    name, beam, mlb, scale, n, lenpen, temp, _ = PREFIX_GROUP
    gen, _, dicts = build_generator(state_dict(scale, cfg), cfg, beam, mlb, 0.0, True)
    cases, pinned, changed = [], 0, 0
    for sid, seed, ns in CANDIDATES:
        fb = fbank(seed, ns)
        set_options(gen, n, lenpen, temp)
        best = run_prefix(gen, sid, fb, beam, None)["nbest"][0]["tokens"]
        for L in PREFIX_LENGTHS:
            pre = best[:L]
            if len(pre) < L or cfg.eos in pre:
                continue
            set_options(gen, n, lenpen, temp)
            rec = run_prefix(gen, sid, fb, beam, pre or None)
            assert all(h["tokens"][:L] == pre for h in rec["nbest"])
            pin = rec["margin"] > rec["tau"]
            set_options(gen, 0, lenpen, temp)
            changed += pin and run_prefix(gen, sid, fb, beam, pre or None)["nbest"][0]["tokens"] != rec["nbest"][0]["tokens"]
            cases.append(dict(slim(rec), sid=sid, pcm_seed=seed, n_samples=ns, prefix=pre))
            pinned += pin
            print(name, sid, "prefix", L, "margin %.3g tau %.3g" % (rec["margin"], rec["tau"]), "changed", changed, flush=True)
        if pinned >= MIN_PINNED and changed >= MIN_CHANGED_BY_BAN and {len(c["prefix"]) for c in cases
                                                                        if c["margin"] > c["tau"]} == set(PREFIX_LENGTHS):
            break
    assert pinned >= MIN_PINNED and changed >= MIN_CHANGED_BY_BAN, f"{name}: {pinned} pinned cases, {changed} changed by the ban"
    assert {len(c["prefix"]) for c in cases if c["margin"] > c["tau"]} == set(PREFIX_LENGTHS), f"{name}: a prefix length has no pinned case"
    out["groups"][name] = {"beam": beam, "max_len_b_mt": mlb, "eos_scale": scale, "no_repeat_ngram_size": n, "len_penalty": lenpen,
                           "temperature": temp, "cases": cases}
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump(out, f, indent=0, ensure_ascii=False)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
