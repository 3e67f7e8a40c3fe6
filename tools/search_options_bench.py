"""What the text search controls cost (ss_mt_search_opts: no-repeat n-grams, length penalty, temperature), on two calls:
    pack128_beam4   ss_batch_mt_beam on the encoder output of the 128-utterance bench pack at beam 4 (512 rows, 2 device calls)
    pool64_beam1    the continuation a 64-writer session-pool step makes at beam 1 with an option set: ss_batch_mt_beam_continue
                    behind 64 committed prefixes of 0 .. 3 tokens, max_len 24
and three settings: off, n = 3, and n = 3 with temperature 1.7 and len_penalty 0.6.

(a) Options off on this build against another build of the library (--parent-lib: the parent commit's, built with
    SS_OUT_LIB=... streamspeech_amd/csrc/build.sh from a checkout of it).  Every pass is a fresh process; the passes alternate parent,
    this build, parent, ... for --rounds rounds; a pass times --reps searches after a warm-up and reports their median.  The verdict:
    median over this build's passes minus median over the parent's passes, against the parent's own spread between passes
    (max - min of its pass medians).
(b) n = 3 and n = 3 + T + p against off on this build, in the same passes: median per search, per decoder step, and the difference
    per step.
Prints one JSON line and writes profiles/search_options.json.

    python tools/search_options_bench.py --parent-lib /path/to/parent/libstreamspeech_hip.so
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SETTINGS = {"off": {}, "ngram3": {"no_repeat_ngram_size": 3},
            "ngram3_temp1.7_lenpen0.6": {"no_repeat_ngram_size": 3, "temperature": 1.7, "len_penalty": 0.6}}


def one_pass(reps: int, parent: bool) -> dict:
    """Runs in a process of its own: the library is the one SS_HIP_LIB names (default: this tree's)."""
    import torch
    from streamspeech_amd import lib as L
    if parent:                                     # a build from before the option entry points: bind what it has
        for name in [n for n in L.SIGNATURES if n.endswith("_opts")]:
            del L.SIGNATURES[name]
    from streamspeech_amd import synth, workload
    from streamspeech_amd.config import ModelConfig
    from streamspeech_amd.engine import HipModel
    cfg = ModelConfig()
    g = np.load(os.path.join(ROOT, "tests", "golden", "gcmvn_fr-en.npz"))
    m = HipModel(synth.make_model_state_dict(0, cfg), cfg, cmvn_mean=g["mean"], cmvn_std=g["std"])
    utts = workload.make_utterances(128)
    pcm = torch.cat([torch.from_numpy(synth.synth_pcm(1234 + u.idx, u.n_samples)) for u in utts]).cuda()
    feat, T = m.batch_fbank_cmvn(pcm, [u.n_samples for u in utts])
    enc, Tp = m.batch_encoder_forward(feat, T)
    mx = [u.n_mt for u in utts]
    off = np.concatenate([[0], np.cumsum(Tp)])
    enc64, Tp64 = enc[:int(off[64])].contiguous(), Tp[:64]
    prefixes = [[10 + b, 80 + b, 150 + b][:b % 4] for b in range(64)]          # distinct tokens: no n-gram stands twice
    settings = {"off": {}} if parent else SETTINGS
    modes = {}
    for s, kw in settings.items():
        modes[f"pack128_beam4/{s}"] = lambda kw=kw: m.batch_mt_beam(enc, Tp, mx, 4, **kw)
        modes[f"pool64_beam1/{s}"] = lambda kw=kw: m.batch_mt_beam_continue(enc64, Tp64, prefixes, [24] * 64, 1, **kw)
    for f in modes.values():
        f()
    torch.cuda.synchronize()
    times = {k: [] for k in modes}
    for _ in range(reps):
        for k, f in modes.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            f()
            torch.cuda.synchronize()
            times[k].append((time.perf_counter() - t) * 1e3)
    return {"steps": {"pack128_beam4": max(mx) + 1, "pool64_beam1": 24 + 1}, "ms": {k: [round(x, 3) for x in v] for k, v in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default="", help="libstreamspeech_hip.so of the parent commit; without it only (b) is measured")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "search_options.json"))
    ap.add_argument("--one-pass", choices=["parent", "this"], default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one_pass:
        print("PASS " + json.dumps(one_pass(a.reps, a.one_pass == "parent")))
        return
    passes = {"parent": [], "this": []}
    for _ in range(a.rounds):
        for who in (["parent"] if a.parent_lib else []) + ["this"]:
            env = dict(os.environ)
            if who == "parent":
                env["SS_HIP_LIB"] = os.path.abspath(a.parent_lib)
            else:
                env.pop("SS_HIP_LIB", None)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--one-pass", who, "--reps", str(a.reps)], env=env,
                                 check=True, capture_output=True, text=True, timeout=600).stdout
            passes[who].append(json.loads(next(ln for ln in out.splitlines() if ln.startswith("PASS "))[5:]))
    steps = passes["this"][0]["steps"]
    res = {"rounds": a.rounds, "reps_per_pass": a.reps, "steps": steps, "calls": {}}
    for call in ("pack128_beam4", "pool64_beam1"):
        med = {who: [float(np.median(p["ms"][f"{call}/off"])) for p in passes[who]] for who in passes if passes[who]}
        rec = {"off_ms_pass_medians": {w: [round(x, 3) for x in v] for w, v in med.items()},
               "off_ms_all": {w: [p["ms"][f"{call}/off"] for p in passes[w]] for w in med}}
        if "parent" in med:
            spread = max(med["parent"]) - min(med["parent"])
            diff = float(np.median(med["this"]) - np.median(med["parent"]))
            rec["vs_parent"] = {"this_minus_parent_ms": round(diff, 3), "parent_spread_ms": round(spread, 3),
                                "not_slower_than_parent_beyond_its_spread": bool(diff <= spread)}
        base = float(np.median([x for p in passes["this"] for x in p["ms"][f"{call}/off"]]))
        rec["settings"] = {}
        for s in SETTINGS:
            ts = [x for p in passes["this"] for x in p["ms"][f"{call}/{s}"]]
            m_ = float(np.median(ts))
            rec["settings"][s] = {"ms_per_search": round(m_, 3), "ms_per_step": round(m_ / steps[call], 4),
                                  "vs_off_ms_per_step": round((m_ - base) / steps[call], 4), "vs_off": round(m_ / base - 1.0, 4),
                                  "spread": round((max(ts) - min(ts)) / m_, 4)}
        res["calls"][call] = rec
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
