"""Writes tests/golden/streaming_beam.json: the reference's offline generator, built as tests/make_golden_beam.py builds it, run with
``prefix_tokens`` (fairseq's _prefix_tokens: the first-pass beam search behind a forced prefix).  Run where the reference tree exists:
    python -m tests.make_golden_beam_prefix

Per group of make_golden_beam.GROUPS and per utterance of its CANDIDATES the unforced search runs first; two 3-token prefixes come
from its n-best list:
    on    the first three tokens of the best hypothesis (the prefix lies on the unforced best path)
    off   the first two tokens of the best hypothesis, then a token the best path does not have there (the streaming case: committed
          tokens come from a shorter encoder memory, so the search would not have chosen them): the first token, scanning the n-best
          list from the worst hypothesis up and each hypothesis from its third token on, that is neither the best hypothesis' third
          token nor </s> / <pad>.  An utterance whose n-best list holds no such token gives no `off` case; `off` never equals `on`.
and two more kinds, one pinned case per group where the group has one (at least one of each over all groups):
    full  the first max_len tokens of the best hypothesis where it is that long (n_prefix == max_len: the only continuation is the
          forced </s>)
    unk   `off` with <unk> as the third token, in the group with a non-zero unk_penalty (a forced <unk> carries the penalty)
Each case records the prefix, the full n-best list (tokens, scores, positional scores; prefix positions included) and the decisive
margin of make_golden_beam.MarginProbe with its tau.  A (group, kind) stops at its sixth pinned case (`full` / `unk`: at the first)."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import kaldi_fbank as K  # noqa: E402
from streamspeech_amd.config import ModelConfig  # noqa: E402
from tests.make_golden_beam import (CANDIDATES, GROUPS, MIN_PINNED, MarginProbe, build_generator, sample_pcm, state_dict,  # noqa: E402
                                    tau)

OUT = os.path.join(ROOT, "tests", "golden", "streaming_beam.json")
N_PREFIX = 3
KINDS = ("on", "off")
NO_GAP = 1e9           # margin of a search that never ranks two finite candidates (one forced path)


def run(gen, sid, fb, beam, prefix):
    """The first-pass n-best list of one B = 1 sample with `prefix` forced (None: unforced), its decisive margin and tau."""
    probe = MarginProbe(gen.generator_mt.search, beam, gen.generator_mt.eos)
    nbest = []
    orig = gen.generator_mt.generate_decoder

    def keep(*a, **kw):
        fin = orig(*a, **kw)
        nbest.append([{"tokens": h["tokens"].int().tolist(), "score": float(h["score"]),
                       "positional_scores": h["positional_scores"].float().tolist()} for h in fin[0]])
        return fin
    gen.generator_mt.generate_decoder = keep
    src = torch.as_tensor(fb, dtype=torch.float32).unsqueeze(0)
    sample = {"id": torch.tensor([int(sid)]), "target": None,
              "net_input": {"src_tokens": src, "src_lengths": torch.tensor([src.shape[1]])}}
    pt = None if prefix is None else torch.tensor([prefix], dtype=torch.long)
    try:
        with open(os.devnull, "w") as null, torch.no_grad():
            so, sys.stdout = sys.stdout, null
            try:
                gen.generate(None, sample, prefix_tokens=pt)
            finally:
                sys.stdout = so
    finally:
        gen.generator_mt.generate_decoder = orig
        gen.generator_mt.search.step = probe.orig
    hyps = nbest[0]
    scores = [h["score"] for h in hyps]
    if probe.gaps or len(hyps) > 1:
        margin, t = probe.margin(scores)
    else:
        margin, t = NO_GAP, tau(max(abs(x) for x in scores))
    return {"nbest": hyps, "margin": margin, "tau": t}


def prefixes(free, max_len, unk, with_unk, eos=2, pad=1):
    best = free[0]["tokens"]
    third = next((t for h in reversed(free[1:]) for t in h["tokens"][2:] if t not in (best[2], eos, pad)), None)
    p = {"on": best[:N_PREFIX], "full": best[:max_len]}
    if third is not None:
        p["off"] = best[:2] + [third]
        assert p["off"] != p["on"]
    if with_unk:
        p["unk"] = best[:2] + [unk]
    return p


def main():
    cfg = ModelConfig()
    g = np.load(os.path.join(ROOT, "tests", "golden", "gcmvn_fr-en.npz"))
    torch.manual_seed(0)
    out = {"note": "reference offline generator with beam_size_mt = k and prefix_tokens (tests/make_golden_beam_prefix.py); "
                   "regenerate with python -m tests.make_golden_beam_prefix", "groups": {}}
    total = {"full": 0, "unk": 0}
    for name, beam, mlb, unkpen, norm, scale in GROUPS:
        sd = state_dict(scale, cfg)
        gen, _, dicts = build_generator(sd, cfg, beam, mlb, unkpen, norm)
        want = {k: MIN_PINNED for k in KINDS}
        want["full"] = 1
        if unkpen:
            want["unk"] = 1
        cases, pinned = {k: [] for k in want}, {k: 0 for k in want}
        for sid, seed, n in CANDIDATES:
            if all(pinned[k] >= want[k] for k in want):
                break
            fb = K.global_cmvn(K.fbank(sample_pcm(seed, n) * np.float32(32768.0)), g["mean"], g["std"])
            free = run(gen, sid, fb, beam, None)["nbest"]
            if len(free[0]["tokens"]) <= N_PREFIX or len(free[-1]["tokens"]) <= N_PREFIX:
                continue
            for kind, pre in prefixes(free, mlb, cfg.unk, bool(unkpen), cfg.eos, cfg.pad).items():
                if pinned[kind] >= want[kind] or cfg.eos in pre:
                    continue
                rec = run(gen, sid, fb, beam, pre)
                assert all(h["tokens"][:len(pre)] == pre for h in rec["nbest"])
                assert all(len(h["positional_scores"]) == len(h["tokens"]) for h in rec["nbest"])
                rec.update({"sid": sid, "pcm_seed": seed, "n_samples": n, "prefix": pre})
                cases[kind].append(rec)
                pinned[kind] += rec["margin"] > rec["tau"]
                print(name, kind, sid, "margin %.3g tau %.3g" % (rec["margin"], rec["tau"]), "lengths",
                      [len(h["tokens"]) for h in rec["nbest"]], flush=True)
        for kind in KINDS:
            assert pinned[kind] >= want[kind], f"{name} / {kind}: only {pinned[kind]} cases above the margin"
        for kind in ("full", "unk"):
            total[kind] += pinned.get(kind, 0)
        out["groups"][name] = {"beam": beam, "max_len_b_mt": mlb, "unk_penalty": unkpen, "normalize": norm, "eos_scale": scale,
                               "cases": cases}
    assert total["full"] >= 1 and total["unk"] >= 1, f"pinned n_prefix == max_len / forced <unk> cases: {total}"
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump(out, f, indent=0, ensure_ascii=False)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
