"""Writes tests/golden/vocoder_multispkr.npz: the reference's CodeGenerator (agent/tts/codehifigan.py) with "multispkr": true, built
by oracle.ref_build.build_vocoder from the seeded multi-speaker state dict (synth.make_vocoder_state_dict(0, cfg) with the default
plan, 5 speakers), on three unit sequences x speakers 0, 2, 4 x with / without duration prediction.  Per case: `wav`, `dur`; the
codes and speaker ids once.  Run where the reference tree exists:
    python -m tests.make_golden_multispkr
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import ref_build  # noqa: E402
from streamspeech_amd import synth  # noqa: E402
from tests.multispkr_ref import multispkr_config  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "vocoder_multispkr.npz")
SEQUENCES = {"six": [3, 17, 999, 4, 4, 250], "one": [512], "two": [77, 901]}
SPEAKERS = (0, 2, 4)


def main():
    torch.set_grad_enabled(False)
    vcfg = multispkr_config(5)
    vsd = synth.make_vocoder_state_dict(0, vcfg)
    gen = ref_build.build_vocoder(vsd, vcfg)
    assert gen.multispkr and tuple(gen.spkr.weight.shape) == (5, vcfg.embedding_dim)
    out = {"speakers": np.array(SPEAKERS, np.int32), "names": np.array(sorted(SEQUENCES))}
    for name, codes in SEQUENCES.items():
        out[f"{name}/codes"] = np.array(codes, np.int32)
        for s in SPEAKERS:
            for dp in (True, False):
                wav, dur = gen(code=torch.tensor([codes]), spkr=torch.tensor([[s]]), dur_prediction=dp)
                key = f"{name}/s{s}/{'dur' if dp else 'nodur'}"
                out[key + "/wav"] = wav.reshape(-1).numpy().astype(np.float32)
                out[key + "/dur"] = (dur.view(-1).numpy() if dur is not None else np.ones(len(codes))).astype(np.int32)
    w0, w2 = out["six/s0/dur/wav"], out["six/s2/dur/wav"]
    print("signal rms %.3f, speaker 0 vs 2 rms %.3f" % (float(np.sqrt(np.mean(w0 ** 2))), float(np.sqrt(np.mean((w0 - w2) ** 2)))))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
