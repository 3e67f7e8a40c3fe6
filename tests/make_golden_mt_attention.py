"""Writes tests/golden/mt_attention.npz: the `attention` of the reference's first-pass text search.  Run where the reference tree
exists:
    python -m tests.make_golden_mt_attention

The reference's offline generator (CTCMultiDecoderSequenceGenerator, built as oracle/ref_offline.build_generator builds it, with
beam_size_mt = 1 and max_len_b_mt = 10, no prefix) runs on 4 seeded synthetic utterances of 12800-32000 samples with the seed-0
synthetic checkpoint, twice: the float32 model, and the same model in .double() on the same fbank.  Its first-pass generator's
generate_decoder is wrapped (it still runs unmodified) to keep hypothesis 0's tokens and `attention` -- [src_len, tgt_len], the
head-averaged cross-attention of the last decoder layer that agent/sequence_generator.py:383-392 / fairseq's finalize_hypos record.
In the .double() model everything up to the scores is float64; fairseq's soft-max (utils.softmax) and the generator's buffer are
float32 in both, so both arrays are float32 and the second one is the first-pass attention with float64 inputs to the soft-max.
An utterance is kept only if both models decode the same tokens.  Per utterance u the file holds fbank{u} [T, 80] float32,
tokens{u} [L] int32 (final </s> included), attn32_{u} and attn64_{u} [Tp, L] float32; arrays only.
"""
import contextlib
import io
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "mt_attention.npz")
CANDIDATES = [(300 + i, 900 + i, 12800 + 6400 * (i % 4)) for i in range(8)]   # (sample id, pcm seed, samples)
N_UTT = 4
MAX_LEN_B_MT = 10


def fbank_of(seed, n):
    from oracle import kaldi_fbank as K
    from streamspeech_amd import synth
    g = np.load(os.path.join(ROOT, "tests", "golden", "gcmvn_fr-en.npz"))
    return np.ascontiguousarray(K.global_cmvn(K.fbank(synth.synth_pcm(seed, n) * np.float32(32768.0)), g["mean"], g["std"]),
                                dtype=np.float32)


def first_pass(gen, sample_id, fbank, dtype):
    """One B = 1 sample through the reference generator -> (tokens [L], attention [src_len, tgt_len]) of hypothesis 0 of its
    first-pass search, as the search returned them."""
    kept = []
    orig = gen.generator_mt.generate_decoder

    def keep(*a, **kw):
        fin = orig(*a, **kw)
        kept.append((fin[0][0]["tokens"].clone(), fin[0][0]["attention"].clone()))
        return fin
    src = torch.as_tensor(fbank, dtype=dtype).unsqueeze(0)
    sample = {"id": torch.tensor([int(sample_id)]), "target": None,
              "net_input": {"src_tokens": src, "src_lengths": torch.tensor([src.shape[1]])}}
    gen.generator_mt.generate_decoder = keep
    try:
        with contextlib.redirect_stdout(io.StringIO()), torch.no_grad():
            gen.generate(None, sample)
    finally:
        gen.generator_mt.generate_decoder = orig
    tokens, attn = kept[0]
    assert attn.dim() == 2 and attn.shape[1] == tokens.numel(), "the reference's decoder handed no attention to the generator"
    return tokens.int().numpy(), attn.numpy()


def generate():
    """-> the fixture's arrays as a dict (what main() saves; tests/test_mt_attention_cpu.py regenerates and compares)."""
    from oracle import ref_offline as RO
    from streamspeech_amd import synth
    from streamspeech_amd.config import ModelConfig
    cfg = ModelConfig()
    torch.manual_seed(0)
    sd = synth.make_model_state_dict(0, cfg)
    gen32, _, _ = RO.build_generator(sd, cfg, max_len_a_mt=0.0, max_len_b_mt=MAX_LEN_B_MT)
    gen64, model64, _ = RO.build_generator(sd, cfg, max_len_a_mt=0.0, max_len_b_mt=MAX_LEN_B_MT)
    model64.double()
    out, n = {}, 0
    for sid, seed, samples in CANDIDATES:
        fb = fbank_of(seed, samples)
        t32, a32 = first_pass(gen32, sid, fb, torch.float32)
        t64, a64 = first_pass(gen64, sid, fb, torch.float64)
        if t32.tolist() != t64.tolist():
            print(sid, "float32 and float64 searches differ: skipped", flush=True)
            continue
        assert a32.dtype == np.float32 and a64.dtype == np.float32 and a32.shape == a64.shape
        out[f"fbank{n}"], out[f"tokens{n}"], out[f"attn32_{n}"], out[f"attn64_{n}"] = fb, t32.astype(np.int32), a32, a64
        print(sid, "samples", samples, "attention", a32.shape, "float32 - float64 %.3e" % np.abs(a32 - a64).max(), flush=True)
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
