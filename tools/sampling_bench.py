"""What sampling costs against the beam search at the same k: HipModel.batch_mt_sample against HipModel.batch_mt_beam on the encoder
output of a 64-utterance pack at k = 4 (256 rows, one device call), for top-k 10, top-p 0.9 and plain sampling.

The decoder launches of the two are the same; a step of the beam search adds the top-2k kernel and the merge kernel, a step of the
sampling search sample_step_kernel (with top-k / top-p: a bitonic sort of the row's ids in LDS) and sample_advance_kernel.  One
process, one build: after a warm-up of every mode the passes alternate beam, top-k, top-p, plain for --reps rounds, each timed with
a host clock around a call that ends in a device synchronise.  Both searches run until every utterance is done, so the steps a call
took are reported beside its time (the longest hypothesis of the call) and the ratio is given per search and per step.
Prints one JSON line and writes profiles/sampling.json.

    python tools/sampling_bench.py
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = {"beam4": None, "sample_topk10": {"topk": 10}, "sample_topp0.9": {"topp": 0.9}, "sample_plain": {}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--utterances", type=int, default=64)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sampling.json"))
    a = ap.parse_args()
    import torch
    from streamspeech_amd import synth, workload
    from streamspeech_amd.config import ModelConfig
    from streamspeech_amd.engine import HipModel
    if not torch.cuda.is_available():
        raise SystemExit("sampling_bench needs a GPU")
    cfg = ModelConfig()
    g = np.load(os.path.join(ROOT, "tests", "golden", "gcmvn_fr-en.npz"))
    m = HipModel(synth.make_model_state_dict(0, cfg), cfg, cmvn_mean=g["mean"], cmvn_std=g["std"])
    utts = workload.make_utterances(a.utterances)
    pcm = torch.cat([torch.from_numpy(synth.synth_pcm(1234 + u.idx, u.n_samples)) for u in utts]).cuda()
    feat, T = m.batch_fbank_cmvn(pcm, [u.n_samples for u in utts])
    enc, Tp = m.batch_encoder_forward(feat, T)
    mx = [u.n_mt for u in utts]
    keys = list(range(a.utterances))

    def run(kw, seed):
        if kw is None:
            return m.batch_mt_beam(enc, Tp, mx, a.k)[0]
        return m.batch_mt_sample(enc, Tp, mx, a.k, keys, seed=seed, **kw)[0]
    for kw in MODES.values():
        run(kw, 1)
    torch.cuda.synchronize()
    ms = {k: [] for k in MODES}
    steps = {k: [] for k in MODES}
    for rep in range(a.reps):
        for name, kw in MODES.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            nbest = run(kw, 1 + rep)                  # a new seed every round: the sampled lengths vary as a user's would
            torch.cuda.synchronize()
            ms[name].append((time.perf_counter() - t) * 1e3)
            steps[name].append(max(len(h["tokens"]) for hyps in nbest for h in hyps))
    res = {"utterances": a.utterances, "k": a.k, "rows": a.utterances * a.k, "reps": a.reps, "max_len": max(mx), "modes": {}}
    base = float(np.median(ms["beam4"]))
    base_step = float(np.median(np.array(ms["beam4"]) / np.array(steps["beam4"])))
    for name in MODES:
        t, per = np.array(ms[name]), np.array(ms[name]) / np.array(steps[name])
        res["modes"][name] = {"ms_per_search_median": round(float(np.median(t)), 3), "ms_per_search_min": round(float(t.min()), 3),
                              "ms_per_search_max": round(float(t.max()), 3), "spread": round(float((t.max() - t.min()) / np.median(t)), 4),
                              "steps_median": float(np.median(steps[name])), "ms_per_step_median": round(float(np.median(per)), 4),
                              "vs_beam_per_search": round(float(np.median(t)) / base, 4),
                              "vs_beam_per_step": round(float(np.median(per)) / base_step, 4)}
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
