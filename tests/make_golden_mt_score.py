"""Writes tests/golden/mt_score.npz: the reference's own score of given translations.  Run where the reference tree exists:
    python -m tests.make_golden_mt_score

fairseq's SequenceScorer.generate (fairseq/sequence_scorer.py) runs in place, unmodified, on a thin wrapper written here: its
``model(**net_input)`` is the reference model's encoder followed by its first-pass text decoder (``target_unigram_decoder``), its
``get_normalized_probs`` is that decoder's.  The model is oracle/ref_offline.build_generator's on the seed-0 synthetic checkpoint;
everything runs twice, on the float32 model and on the same model in .double() (fairseq's log_softmax is float32 in both, so both
runs answer float32 arrays; the second is the score with float64 logits).  4 seeded synthetic utterances of 12800-32000 samples
(the candidates of make_golden_mt_attention.py), each with three texts, one B = 1 sample per text:
  0  the reference generator's own greedy hypothesis (max_len_b_mt = 10; kept only if both models decode the same tokens);
  1  a seeded random text of 17 tokens (low probabilities, large ranks);
  2  the empty text (only </s>).
Per utterance u and text k the file holds fbank{u} [T, 80] float32, tokens{u}_{k} [L] int32 (final </s> included), pos32_{u}_{k} and
pos64_{u}_{k} [L] float32 (SequenceScorer's positional_scores, natural log), score32_{u}_{k} and score64_{u}_{k} (its score: the
mean with </s> counted); arrays only.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "mt_score.npz")
N_UTT = 4
N_RANDOM = 17


class FirstPass(torch.nn.Module):
    """What SequenceScorer calls: the reference model's encoder and first-pass text decoder, forwarded to."""

    def __init__(self, model):
        super().__init__()
        self.model = model
        self.decoder = getattr(model, f"{model.mt_task_name}_decoder")

    def forward(self, src_tokens, src_lengths, prev_output_tokens, **kw):
        enc = self.model.encoder(src_tokens, src_lengths=src_lengths)
        return self.decoder(prev_output_tokens, encoder_out=enc)

    def get_normalized_probs(self, net_output, log_probs, sample=None):
        return self.decoder.get_normalized_probs(net_output, log_probs, sample)


def score(scorer, wrapper, fbank, tokens, dtype, eos):
    """One B = 1 sample through SequenceScorer -> (positional_scores [L], score)."""
    src = torch.as_tensor(fbank, dtype=dtype).unsqueeze(0)
    tgt = torch.tensor([tokens], dtype=torch.long)
    prev = torch.tensor([[eos] + list(tokens[:-1])], dtype=torch.long)
    sample = {"net_input": {"src_tokens": src, "src_lengths": torch.tensor([src.shape[1]]), "prev_output_tokens": prev},
              "target": tgt}
    hyp = scorer.generate([wrapper], sample)[0][0]
    assert hyp["tokens"].tolist() == list(tokens)
    return hyp["positional_scores"].float().numpy(), np.float32(float(hyp["score"]))


def generate():
    """-> the fixture's arrays as a dict (what main() saves; tests/test_mt_score_cpu.py regenerates and compares)."""
    from oracle import ref_offline as RO
    from streamspeech_amd import synth
    from streamspeech_amd.config import ModelConfig
    from tests import make_golden_mt_attention as A
    cfg = ModelConfig()
    torch.manual_seed(0)
    sd = synth.make_model_state_dict(0, cfg)
    gen32, model32, dicts = RO.build_generator(sd, cfg, max_len_a_mt=0.0, max_len_b_mt=A.MAX_LEN_B_MT)
    gen64, model64, _ = RO.build_generator(sd, cfg, max_len_a_mt=0.0, max_len_b_mt=A.MAX_LEN_B_MT)
    model64.double()
    # the scorer's file runs where it lies, over the stub tree build_generator installed (oracle/ref_loader.py); the one symbol it
    # needs beyond that tree is utils.strip_pad (fairseq/utils.py: tensor[tensor.ne(pad)])
    from oracle import ref_loader
    sys.modules["fairseq.utils"].strip_pad = lambda tensor, pad: tensor[tensor.ne(pad)]
    SequenceScorer = ref_loader._load_file("fairseq.sequence_scorer", "fairseq/fairseq/sequence_scorer.py").SequenceScorer
    w32, w64 = FirstPass(model32), FirstPass(model64)
    scorer = SequenceScorer(dicts["target_unigram"])
    out, n = {}, 0
    for sid, seed, samples in A.CANDIDATES:
        fb = A.fbank_of(seed, samples)
        t32, _ = A.first_pass(gen32, sid, fb, torch.float32)
        t64, _ = A.first_pass(gen64, sid, fb, torch.float64)
        if t32.tolist() != t64.tolist():
            print(sid, "float32 and float64 searches differ: skipped", flush=True)
            continue
        rnd = [int(t) for t in synth.uniform(seed, "mt_score_text", (N_RANDOM,), 4, cfg.tgt_vocab)]
        texts = [[int(t) for t in t32], rnd + [cfg.eos], [cfg.eos]]
        assert texts[0][-1] == cfg.eos
        out[f"fbank{n}"] = fb
        for k, toks in enumerate(texts):
            p32, s32 = score(scorer, w32, fb, toks, torch.float32, cfg.eos)
            p64, s64 = score(scorer, w64, fb, toks, torch.float64, cfg.eos)
            out[f"tokens{n}_{k}"] = np.asarray(toks, dtype=np.int32)
            out[f"pos32_{n}_{k}"], out[f"pos64_{n}_{k}"] = p32.astype(np.float32), p64.astype(np.float32)
            out[f"score32_{n}_{k}"], out[f"score64_{n}_{k}"] = s32, s64
            print(sid, "text", k, "tokens", len(toks), "score %.4f" % s64, "float32 - float64 %.3e" % np.abs(p32 - p64).max(), flush=True)
        n += 1
        if n == N_UTT:
            break
    assert n == N_UTT, f"only {n} utterances"
    out["n"] = np.int32(n)
    return out


def main():
    out = generate()
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
