"""First-pass text search alone: greedy (ss_batch_mt_greedy) against the beam search (ss_batch_mt_beam) at beam 1, 4 and 10 on the
encoder output of one synthetic 128-utterance pack (the bench.py workload).  The modes run alternately, `--reps` rounds; per mode
the median milliseconds per search and per decoder step, the rows each step decodes, and the spread (max - min) / median.  Prints
one JSON line and writes profiles/beam_bench.json.  A pack with B * beam > 256 rows runs as consecutive calls of at most 256 rows
(engine.plan_beam_groups), as the offline driver runs it.

Kernel stats of the beam-10 search alone:
    rocprofv3 --kernel-trace --stats -d profiles/beam_rocprof -o beam -- python tools/beam_bench.py --only beam10 --reps 3
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from streamspeech_amd import synth, workload  # noqa: E402
from streamspeech_amd.config import ModelConfig  # noqa: E402
from streamspeech_amd.engine import HipModel, plan_beam_groups  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--utts", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only", default="", help="run one mode (greedy, beam1, beam4, beam10)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "beam_bench.json"))
    a = ap.parse_args()
    cfg = ModelConfig()
    g = np.load(os.path.join(ROOT, "tests", "golden", "gcmvn_fr-en.npz"))
    m = HipModel(synth.make_model_state_dict(0, cfg), cfg, cmvn_mean=g["mean"], cmvn_std=g["std"])
    utts = workload.make_utterances(a.utts)
    pcm = torch.cat([torch.from_numpy(synth.synth_pcm(1234 + u.idx, u.n_samples)) for u in utts]).cuda()
    feat, T = m.batch_fbank_cmvn(pcm, [u.n_samples for u in utts])
    enc, Tp = m.batch_encoder_forward(feat, T)
    mx = [u.n_mt for u in utts]
    steps = max(mx) + 1                 # the seed-0 model never ends early: every search runs to its max_len step
    modes = {"greedy": lambda: m.batch_mt_greedy(enc, Tp, mx),
             "beam1": lambda: m.batch_mt_beam(enc, Tp, mx, 1),
             "beam4": lambda: m.batch_mt_beam(enc, Tp, mx, 4),
             "beam10": lambda: m.batch_mt_beam(enc, Tp, mx, 10)}
    if a.only:
        modes = {a.only: modes[a.only]}
    for f in modes.values():            # warm-up: allocations, first launches
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in modes}
    for _ in range(a.reps):
        for k, f in modes.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t) * 1e3)
    res = {"utterances": len(utts), "max_len": max(mx), "steps": steps, "reps": a.reps, "modes": {}}
    for k, ts in times.items():
        beam = 1 if k == "greedy" else int(k[4:])
        med = float(np.median(ts))
        res["modes"][k] = {"ms_per_search": round(med, 3), "ms_per_step": round(med / steps, 4),
                           "rows_per_step": len(utts) * beam, "calls": len(plan_beam_groups(len(utts), beam)) if k != "greedy" else 1,
                           "spread": round((max(ts) - min(ts)) / med, 4), "ms_all": [round(x, 3) for x in ts]}
    if "greedy" in times:
        for k in ("beam4", "beam10"):
            if k in times:
                res["modes"][k]["step_vs_k_greedy_steps"] = round(res["modes"][k]["ms_per_step"] / (int(k[4:]) * res["modes"]["greedy"]["ms_per_step"]), 4)
    line = json.dumps(res)
    print(line)
    if not a.only:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
