"""What a hotword set costs inside the CTC prefix beam search, and that the plain search costs what it did.  One 128-utterance pack
of the bench workload goes through the encoder once; then, on one text head and the same packed encoder output at beam 8 (cand
the default, 9), in ALTERNATING passes (plain, bias100, bias4000, lm, lm_bias, parent, plain, ...) so that clock and thermal drift
fall on all sides:
  plain     batch_ctc_beam(head, enc, Tp, 8)                                       this tree
  bias100   batch_ctc_beam(..., bias=100 phrases, bias_scale 1)
  bias4000  batch_ctc_beam(..., bias=4000 phrases, bias_scale 1)
  lm        batch_ctc_beam(..., lm=order-3 model of about 4 * 10^5 entries, lm_weight 0.5)
  lm_bias   batch_ctc_beam(..., lm=the same, bias=4000 phrases)
  parent    batch_ctc_beam(head, enc, Tp, 8)                                       the parent build (--parent-lib), in a child process
                                                                                   that stays up for the whole run
Each call is timed on the host, synchronised before and after (head GEMM, table fill, both kernels, the device-to-host copy and the
host unpacking).  Per side: the median call in each pass, the median over passes and the run-to-run spread (highest / lowest pass
median).  Reported: bias100 / plain, bias4000 / plain and lm_bias / lm, each beside the spreads of its two sides, and plain / parent
beside the parent's own spread -- the plain search's code path is meant to be untouched, so that ratio has to lie inside the
spread (`plain_inside_parent_spread`).

The sets: 20 bigrams of the plain search's own best hypotheses whose first token lies in the lower half of the vocabulary (so the
set bears on the search: `best_differs_from_plain`), the rest seeded random phrases of 2 .. 5 tokens, the first from the lower half
of the vocabulary and the others from the upper half (no phrase inside another), per-token boosts in [0.5, 3).

  python tools/ctc_bias_bench.py --out profiles/ctc_bias.json [--parent-lib PARENT.so]     SS_BENCH_PASSES passes per side (default 7)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ctc_lm_bench import _setup, _side, _timed, synthetic_lm  # noqa: E402

HEAD, BEAM, CALLS = 0, 8, 5
NEW_SYMBOLS = ("ss_ctc_bias_create", "ss_ctc_bias_destroy", "ss_ctc_bias_info", "ss_ctc_bias_score_host", "ss_op_ctc_bias_score",
               "ss_batch_ctc_beam_bias", "ss_ctc_beam_bias_host", "ss_op_ctc_beam_bias", "ss_ctc_stream_create_bias",
               "ss_debug_ctc_stream_create_bias")


def hotword_set(V, n, hyps, seed):
    """-> (phrases, boosts): up to 20 bigrams of `hyps` (first token below V / 2), then seeded random phrases up to n in all."""
    import numpy as np
    rng = np.random.default_rng(seed)
    seen, phrases = set(), []
    for h in hyps:
        for p in zip(h.tokens, h.tokens[1:]):
            if len(phrases) < 20 and 4 <= p[0] < V // 2 and p not in seen:
                seen.add(p)
                phrases.append(list(p))
    while len(phrases) < n:
        p = (int(rng.integers(4, V // 2)),) + tuple(int(v) for v in rng.integers(V // 2, V, int(rng.integers(1, 5))))
        if p not in seen:
            seen.add(p)
            phrases.append(list(p))
    return phrases, rng.uniform(0.5, 3.0, len(phrases)).astype(np.float32).tolist()


def child():
    """The parent build's side: `pass` on stdin -> the pass median in ms on stdout; `quit` ends."""
    from streamspeech_amd import lib as L
    for name in NEW_SYMBOLS:                                     # the parent build has none of them
        L.SIGNATURES.pop(name, None)
    m, enc, Tp = _setup()
    print("ready", flush=True)
    for line in sys.stdin:
        f = line.split()
        if not f or f[0] == "quit":
            break
        if f[0] == "warm":
            m.batch_ctc_beam(HEAD, enc, Tp, BEAM)
            print("ok", flush=True)
        else:
            print(statistics.median(_timed(lambda: m.batch_ctc_beam(HEAD, enc, Tp, BEAM)) for _ in range(CALLS)), flush=True)


def measure(out_path, parent_lib):
    import torch
    from streamspeech_amd.hotwords import CtcBias
    from streamspeech_amd.ngram import NgramLM
    m, enc, Tp = _setup()
    V = m.cfg.src_vocab if HEAD == 0 else m.cfg.tgt_vocab
    passes = int(os.environ.get("SS_BENCH_PASSES", "7"))
    plain_hyps = [hs[0] for hs in m.batch_ctc_beam(HEAD, enc, Tp, BEAM) if hs]
    t0 = time.perf_counter()
    sets = {n: CtcBias(*hotword_set(V, n, plain_hyps, n), V, m.cfg.pad, m.cfg.unk) for n in (100, 4000)}
    set_build_s = time.perf_counter() - t0
    lm = NgramLM(synthetic_lm(V, 3, 200000, 1))
    par = None
    if parent_lib:
        par = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                               text=True, env=dict(os.environ, SS_HIP_LIB=os.path.abspath(parent_lib)))
        assert par.stdout.readline().strip() == "ready", "the parent build's process did not come up"

    def ask(cmd):
        par.stdin.write(cmd + "\n")
        par.stdin.flush()
        return par.stdout.readline().strip()
    try:
        sides = {"plain": lambda: m.batch_ctc_beam(HEAD, enc, Tp, BEAM),
                 "bias100": lambda: m.batch_ctc_beam(HEAD, enc, Tp, BEAM, bias=sets[100]),
                 "bias4000": lambda: m.batch_ctc_beam(HEAD, enc, Tp, BEAM, bias=sets[4000]),
                 "lm": lambda: m.batch_ctc_beam(HEAD, enc, Tp, BEAM, lm=lm, lm_weight=0.5),
                 "lm_bias": lambda: m.batch_ctc_beam(HEAD, enc, Tp, BEAM, lm=lm, lm_weight=0.5, bias=sets[4000])}
        got = {k: fn() for k, fn in sides.items()}               # warm-up: scratch growth, first launches, the tables' upload
        if par:
            assert ask("warm") == "ok"
        med = {k: [] for k in list(sides) + (["parent"] if par else [])}
        for _ in range(passes):
            for k, fn in sides.items():
                med[k].append(statistics.median(_timed(fn) for _ in range(CALLS)))
            if par:
                med["parent"].append(float(ask("pass")))
    finally:
        if par:
            par.stdin.write("quit\n")
            par.stdin.flush()
            par.wait(timeout=60)
    row = {"head": HEAD, "beam": BEAM, "cand": BEAM + 1, "nbest": BEAM, "utterances": len(Tp), "frames": sum(Tp), "longest_frames": max(Tp),
           "passes_per_side": passes, "calls_per_pass": CALLS, **{k: _side(v) for k, v in med.items()}}
    for k, base in (("bias100", "plain"), ("bias4000", "plain"), ("lm_bias", "lm")):
        row[f"ratio_{k}_over_{base}"] = round(row[k]["call_ms_median"] / row[base]["call_ms_median"], 4)
        row[f"best_differs_from_{base}_in_{k}"] = sum(a[0].tokens != b[0].tokens for a, b in zip(got[k], got[base]))
    if par:
        r = row["plain"]["call_ms_median"] / row["parent"]["call_ms_median"]
        row["ratio_plain_over_parent"] = round(r, 4)
        row["plain_inside_parent_spread"] = bool(1.0 / row["parent"]["spread"] <= r <= row["parent"]["spread"])
    print(json.dumps(row), flush=True)
    res = {"tool": "tools/ctc_bias_bench.py", "device": torch.cuda.get_device_name(0),
           "order": "alternating passes: plain, bias100, bias4000, lm, lm_bias, parent, plain, ...", "bias_scale": 1.0, "finish": True,
           "lm_weight": 0.5, "sets": {str(n): {"phrases": b.n_phrases, "states": b.states, "slots": b.slots, "device_bytes": b.device_bytes}
                                      for n, b in sets.items()},
           "sets_host_build_s": round(set_build_s, 3), "model": {"order": lm.order, "entries": lm.entries, "device_bytes": lm.device_bytes},
           "parent_lib": bool(parent_lib), "result": row}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="libstreamspeech_hip.so of the parent commit: its plain search is timed beside this tree's")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child()
    else:
        measure(a.out, a.parent_lib)
