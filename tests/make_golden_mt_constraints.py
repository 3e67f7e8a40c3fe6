"""Writes tests/golden/mt_constraints.json: the reference's offline generator, built as tests/make_golden_beam.py builds it, with the
search of its first-pass generator swapped for the reference's own LexicallyConstrainedBeamSearch(tgt_dict, "ordered")
(fairseq/fairseq/search.py, unmodified) and a packed constraints tensor (token_generation_constraints.pack_constraints) per
utterance.  Run where the reference tree exists:
    python -m tests.make_golden_mt_constraints

Two things of the harness, none of the search: the multi-decoder generator refuses constraints because its SECOND-pass search has
no support for them, and it initialises the first-pass search's constraints itself, so the tensor is handed to
search.init_constraints here, right before generate_decoder runs, and the generator's own call with None is ignored.

Groups (beam, max_len_b_mt, eos_scale as in make_golden_beam):
    beam4_one_token              beam 4,  one 1-token phrase
    beam5_two_phrases            beam 5,  two phrases of 2 and 3 tokens
    beam10_early_eos_lenpen0.6   beam 10, eos_scale 3, max_len_b_mt 16, len_penalty 0.6, one 2-token phrase
    beam1_two_tokens             beam 1,  one 2-token phrase
    beam4_mixed                  beam 4,  every other utterance without phrases (C = 0 through the constrained step), the others with
                                 a 1-token and a 2-token phrase: the utterances the GPU test runs as one pack
Phrases are drawn (seeded by the sample id) from tokens the unconstrained best hypothesis does not contain.  Per utterance: the
phrases, the n-best list (tokens, scores, positional scores), the decisive margin and its tau; for the first two pinned constrained
utterances of a group the trace of the selection stage over the first 6 steps: the states and the candidate list in, the
selection out (scores as float32 bit patterns).  An utterance that is not pinned keeps no n-best list.

Decisive margin: make_golden_beam.MarginProbe's gaps, and from every step of the constrained selection the gap between the 2k-th
and the next global candidate, between each row's best and second-best, and between neighbours of the same bank in the sorted,
de-duplicated candidate list (keys; the first of the pair could still be selected).  An utterance is pinned when margin > tau.

The script checks, at every step of every utterance, that tests/constraint_ref.py selects what the reference's step_sentence
returned (scores bit for bit, tokens, beams, new states) for BOTH orders of a row's next tokens, and for every pinned utterance
that the reference had no two distinct candidates with an equal finite key and no two equal stripe values.  Where the reference's
selection differs from the rule's only in -inf candidates and their places (the step at max_len, where every token but </s> is
-inf and its topk and unstable sort order the equal candidates as they please; the finite ones, in order, are asserted equal), the
generator is handed the outcome under the rule's tie-break, one of those the reference may produce, and goes on from it; the
steps are recorded per utterance (rule_tiebreak_steps).  The script checks its own
inputs too: hypothesis 0 of at least 4 pinned constrained utterances per group differs from the unconstrained search, and every
hypothesis of every constrained utterance contains every phrase in order."""
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
from tests import constraint_ref as CR  # noqa: E402
from tests.make_golden_beam import CANDIDATES, MIN_PINNED, MarginProbe, build_generator, sample_pcm, state_dict  # noqa: E402
from tests.make_golden_beam_prefix import run as run_plain  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "mt_constraints.json")
# (name, beam, max_len_b_mt, eos_scale, len_penalty, phrase lengths, every other utterance unconstrained); the early-</s> group
# draws its phrases from the runners-up of the unconstrained search (draw_phrases)
GROUPS = [("beam4_one_token", 4, 10, 1.0, 1.0, (1,), False),
          ("beam5_two_phrases", 5, 10, 1.0, 1.0, (2, 3), False),
          ("beam10_early_eos_lenpen0.6", 10, 16, 3.0, 0.6, (2,), False),
          ("beam1_two_tokens", 1, 10, 1.0, 1.0, (2,), False),
          ("beam4_mixed", 4, 10, 1.0, 1.0, (1, 2), True)]
CANDIDATES = CANDIDATES + [(200 + i, 700 + i, 12800 + 3200 * (i % 7)) for i in range(16, 40)]
MIN_CHANGED, N_TRACED, TRACE_STEPS = 4, 2, 6


def bits(x):
    return int(np.asarray(x, np.float32).view(np.int32))


class ConsProbe:
    """Wraps search.step_sentence (calls it unchanged): holds tests/constraint_ref.py against every call, collects the decisive gaps,
    the conditions under which the reference's own outcome is determined, and the trace."""

    def __init__(self, search, beam, phrases):
        self.search, self.k, self.cons = search, beam, CR.Constraints(phrases)
        self.orig = search.step_sentence
        self.gaps, self.undetermined, self.chance, self.trace = [], [], [], []
        search.step_sentence = self

    def __call__(self, step, sentno, lprobs, constraint_states, beams_buf, indices_buf, scores_buf):
        k, cons = self.k, self.cons
        states = [s.state for s in constraint_states]
        rows = lprobs.detach().numpy().astype(np.float32)
        given = list(zip(scores_buf.numpy().astype(np.float32).tolist(), indices_buf.tolist(), beams_buf.tolist()))
        out = self.orig(step, sentno, lprobs, constraint_states, beams_buf, indices_buf, scores_buf)
        ref = [(bits(s), int(t), int(b), st.state) for s, t, b, st in zip(out[0], out[1], out[2], out[3])]
        ninf = bits(-np.inf)

        def finite(sel):     # which -inf candidates the reference's topk and sort place where among equals is chance: the others, in order,
            return [(i < k,) + tuple(x) for i, x in enumerate(sel) if x[0] != ninf]     # and whether they may finalise
        for descending in (False, True):
            cands = CR.candidates(cons, rows, states, k, step, descending)
            assert finite([(bits(s), t, b) for s, t, b in cands[:len(given)]]) == finite([(bits(s), t, b) for s, t, b in given]), \
                f"step {step}: the candidate list differs from the reference's"
            mine = [(bits(s), t, b, st) for s, t, b, st in CR.select_from(cons, cands, states, k)]
            assert [x[1:] for x in finite(mine)] == [x[1:] for x in finite(ref)], \
                f"step {step}: selection differs from the reference (descending={descending})\n{mine}\n{ref}"
            if descending is False and mine != ref:
                # The reference's outcome hung on the order its topk and sort gave to equal (-inf) candidates.  The generator goes on
                # with the outcome under the rule's tie-break -- one of those its unstable sort may produce -- with states made by
                # the reference's own advance().
                self.chance.append(step)
                ref = mine
                sel = CR.select_from(cons, cands, states, k)
                out = (torch.tensor([float(s) for s, _, _, _ in sel], dtype=out[0].dtype),
                       torch.tensor([t for _, t, _, _ in sel], dtype=out[1].dtype),
                       torch.tensor([b for _, _, b, _ in sel], dtype=out[2].dtype),
                       [constraint_states[b].advance(t) for _, t, b, _ in sel])
                assert [st.state for st in out[3]] == [st for _, _, _, st in sel]
        cands = CR.candidates(cons, rows, states, k, step)
        # the reference's key, formed by its own expression on its own tensor types
        new = [cons.advance(states[b], t) for _, t, b in cands]
        banks = torch.tensor([n + 1 for n in new])
        key = ((cons.U - banks) * -100 + torch.tensor([float(s) for s, _, _ in cands], dtype=torch.float32)).tolist()
        ident = {}
        for kv, (_, t, b) in zip(key, cands):
            ident.setdefault(kv, set()).add((b, t))
        if any(len(v) > 1 and np.isfinite(kv) for kv, v in ident.items()):
            self.undetermined.append(f"step {step}: distinct candidates with equal key")
        order = sorted(range(len(cands)), key=lambda i: (-key[i], i))
        seen, uniq = set(), []
        for i in order:
            if (cands[i][2], cands[i][1]) not in seen:
                seen.add((cands[i][2], cands[i][1]))
                uniq.append(i)
        M, count, stripes = len(uniq), {}, []
        for i in uniq:                       # STEP 6 of step_sentence
            r = count.get(new[i], 0)
            count[new[i]] = r + 1
            stripes.append(cons.U - (new[i] + 1) + r * (M + 1))
        if len(set(stripes)) != len(stripes):
            self.undetermined.append(f"step {step}: equal stripe values")
        # decisive gaps
        # neighbours of one bank, the first of them selected.  -inf candidates need no gap: they are -inf in every implementation,
        # and the rule orders them by list position.
        last, rank, in_bank = {}, {}, {}
        for i in uniq:
            in_bank[i] = rank.get(new[i], 0)
            rank[new[i]] = in_bank[i] + 1
        chosen = set(sorted(uniq, key=lambda i: (in_bank[i], -new[i]))[:2 * k])
        for i in uniq:
            p = last.get(new[i])
            if p is not None and p in chosen and np.isfinite(key[p]) and np.isfinite(key[i]):
                self.gaps.append((key[p] - key[i], abs(key[i])))
            last[new[i]] = i
        nrow = 1 if step == 0 else k
        flat = np.sort(rows[:nrow].reshape(-1))[::-1]
        if np.isfinite(flat[2 * k]):
            self.gaps.append((float(flat[2 * k - 1] - flat[2 * k]), float(abs(flat[2 * k]))))
        if step > 0:
            for j in range(k):
                top = np.sort(rows[j])[::-1]
                if np.isfinite(top[1]):
                    self.gaps.append((float(top[0] - top[1]), float(abs(top[1]))))
        self.trace.append({"step": step, "states": states,
                           "cand_score_bits": [bits(s) for s, _, _ in cands], "cand_tok": [t for _, t, _ in cands],
                           "cand_beam": [b for _, _, b in cands],
                           "out_score_bits": [r[0] for r in ref], "out_tok": [r[1] for r in ref], "out_beam": [r[2] for r in ref],
                           "out_state": [r[3] for r in ref]})
        return out


def run(gen, search_cls, tgt_dict, sid, fb, beam, phrases):
    """The first-pass n-best list of one B = 1 sample under `phrases`, through the reference's constrained search."""
    from fairseq.token_generation_constraints import pack_constraints
    g = gen.generator_mt
    plain = g.search
    g.search = search_cls(tgt_dict, "ordered")
    packed = pack_constraints([[torch.tensor(p, dtype=torch.long) for p in phrases]])
    init = g.search.init_constraints
    g.search.init_constraints = lambda c, b: None if c is None else init(c, b)
    probe = MarginProbe(g.search, beam, g.eos)
    cprobe = ConsProbe(g.search, beam, phrases)
    nbest = []
    orig = g.generate_decoder

    def keep(encoder_outs, src_tokens, src_lengths, sample, prefix_tokens, constraints, *a, **kw):
        init(packed, beam)
        fin = orig(encoder_outs, src_tokens, src_lengths, sample, prefix_tokens, packed, *a, **kw)
        nbest.append([{"tokens": h["tokens"].int().tolist(), "score": float(h["score"]),
                       "positional_scores": h["positional_scores"].float().tolist()} for h in fin[0]])
        return fin
    g.generate_decoder = keep
    src = torch.as_tensor(fb, dtype=torch.float32).unsqueeze(0)
    sample = {"id": torch.tensor([int(sid)]), "target": None,
              "net_input": {"src_tokens": src, "src_lengths": torch.tensor([src.shape[1]])}}
    try:
        with open(os.devnull, "w") as null, torch.no_grad():
            so, sys.stdout = sys.stdout, null
            try:
                gen.generate(None, sample)
            finally:
                sys.stdout = so
    finally:
        g.generate_decoder = orig
        g.search = plain
    hyps = nbest[0]
    probe.gaps += cprobe.gaps
    margin, t = probe.margin([h["score"] for h in hyps])
    return {"nbest": hyps, "margin": margin, "tau": t, "rule_tiebreak_steps": cprobe.chance}, cprobe


def draw_phrases(sid, lengths, avoid, cfg, runners_up=None):
    """Seeded by the sample id: distinct ordinary tokens the unconstrained best hypothesis does not contain.  With runners_up (the
    rest of the unconstrained n-best list) the pool is what THEY hold of such tokens, where that is enough: phrases the model can
    afford before max_len, so that hypotheses still end at different lengths."""
    rng = np.random.RandomState(sid)
    pool = [t for t in range(4, cfg.tgt_vocab) if t not in set(avoid)]
    near = sorted({t for h in (runners_up or []) for t in h["tokens"]} & set(pool))
    if len(near) >= sum(lengths):
        pool = near
    toks = [int(t) for t in rng.choice(pool, size=sum(lengths), replace=False)]
    out, o = [], 0
    for n in lengths:
        out.append(toks[o:o + n])
        o += n
    return out


def main():
    cfg = ModelConfig()
    g = np.load(os.path.join(ROOT, "tests", "golden", "gcmvn_fr-en.npz"))
    torch.manual_seed(0)
    out = {"note": "reference offline generator with LexicallyConstrainedBeamSearch(ordered) as its first-pass search "
                   "(tests/make_golden_mt_constraints.py); regenerate with python -m tests.make_golden_mt_constraints",
           "groups": {}}
    for name, beam, mlb, scale, lenpen, lengths, mixed in GROUPS:
        gen, _, dicts = build_generator(state_dict(scale, cfg), cfg, beam, mlb, 0.0, True)
        gen.generator_mt.len_penalty = float(lenpen)
        search_cls = sys.modules["fairseq.search"].LexicallyConstrainedBeamSearch
        recs, pinned, changed, traced, n = {}, 0, 0, 0, 0
        for sid, seed, ns in CANDIDATES:
            fb = K.global_cmvn(K.fbank(sample_pcm(seed, ns) * np.float32(32768.0)), g["mean"], g["std"])
            free = run_plain(gen, sid, fb, beam, None)
            phrases = [] if (mixed and n % 2 == 1) else draw_phrases(sid, lengths, free["nbest"][0]["tokens"], cfg,
                                                                             free["nbest"][1:] if scale != 1.0 else None)
            n += 1
            rec, probe = run(gen, search_cls, dicts["target_unigram"], sid, fb, beam, phrases)
            pin = rec["margin"] > rec["tau"]
            for h in rec["nbest"]:
                assert None not in CR.contains_in_order(h["tokens"], phrases), f"{name} {sid}: a hypothesis misses a phrase"
            if not phrases:       # C = 0 through the constrained step: the plain search
                assert [h["tokens"] for h in rec["nbest"]] == [h["tokens"] for h in free["nbest"]]
                assert [h["score"] for h in rec["nbest"]] == [h["score"] for h in free["nbest"]]
            if pin:
                assert not probe.undetermined, f"{name} {sid}: {probe.undetermined}"
                changed += bool(phrases) and rec["nbest"][0]["tokens"] != free["nbest"][0]["tokens"]
            rec.update(pcm_seed=seed, n_samples=ns, phrases=phrases)
            if pin and phrases and traced < N_TRACED:
                rec["trace"] = [t for t in probe.trace if t["step"] < TRACE_STEPS]
                traced += 1
            best = rec["nbest"][0]["tokens"]
            if not pin:           # never compared: what it was run on and why it is not pinned is enough
                del rec["nbest"]
            recs[str(sid)] = rec
            pinned += pin
            print(name, sid, "phrases", phrases, "margin %.3g tau %.3g" % (rec["margin"], rec["tau"]), "best", best,
                  "changed", changed, flush=True)
            if pinned >= MIN_PINNED and changed >= MIN_CHANGED and traced >= N_TRACED:
                break
        assert pinned >= MIN_PINNED, f"{name}: only {pinned} utterances above the margin"
        assert changed >= MIN_CHANGED, f"{name}: the constraints change hypothesis 0 of only {changed} pinned utterances"
        assert traced >= N_TRACED
        out["groups"][name] = {"beam": beam, "max_len_b_mt": mlb, "eos_scale": scale, "len_penalty": lenpen, "hypotheses": recs}
    with open(OUT, "w", encoding="utf-8") as f:
        json.dump(out, f, indent=0, ensure_ascii=False)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
