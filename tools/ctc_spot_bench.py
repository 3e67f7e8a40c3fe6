"""What keyword spotting on a CTC head costs, and that the paths without keywords cost what they did.  One 128-utterance pack of the
bench workload goes through the encoder once; then, on head 0 and the same packed encoder output, in ALTERNATING passes (greedy,
spot100, spot4000, parent, greedy, ...) so that clock and thermal drift fall on all sides:
  greedy    batch_ctc_greedy(head, enc, Tp, return_scores=True)                    this tree: the scored greedy call
  spot100   batch_ctc_spot(head, enc, Tp, 100 keywords, max_hits 256)
  spot4000  batch_ctc_spot(head, enc, Tp, 4000 keywords, max_hits 256)
  parent    batch_ctc_greedy(..., return_scores=True)                              the parent build (--parent-lib), in a child process
                                                                                   that stays up for the whole run
Each call is timed on the host, synchronised before and after (head GEMM, the kernels, the device-to-host copy and the host
unpacking).  Per side: the median call in each pass, the median over passes and the run-to-run spread (highest / lowest pass
median).  Reported: spot / greedy, and greedy / parent beside the parent's own spread -- the greedy call's code path is untouched,
so that ratio has to lie inside the spread (`greedy_inside_parent_spread`).
The kernels apart: ss_op_ctc_spot on the pack's own logits with ss_debug_ctc_spot_phases at 1 (the gather kernel and the call's
two small uploads and memset), 2 (the DP kernel) and 7 (all three), per set.
The pool: N = 1, 16 and 64 ASR sessions (TextSessionPool, 320-ms segments, 10 s of history, then 5 timed steps; tools/
ctc_stream_bench.py's feed), without and with spot=the 100-keyword set, and the pool without spot on the parent build.

The sets: 20 bigrams of the pack's own greedy transcripts (so the set bears on the audio), the rest seeded random phrases of
1 .. 6 tokens over the whole vocabulary; tau 1.0, the shipped default.

  python tools/ctc_spot_bench.py --out profiles/ctc_spot.json [--parent-lib PARENT.so]     SS_BENCH_PASSES passes per side (default 7)"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from ctc_lm_bench import _setup, _side, _timed  # noqa: E402
from ctc_stream_bench import MAX_ROWS, TIMED_STEPS, _args, _segments  # noqa: E402

HEAD, CALLS, MAX_HITS, POOL_N = 0, 5, 256, (1, 16, 64)
NEW_SYMBOLS = ("ss_ctc_spot_set_create", "ss_ctc_spot_set_destroy", "ss_ctc_spot_set_info", "ss_batch_ctc_spot", "ss_ctc_spot_host",
               "ss_op_ctc_spot", "ss_ctc_spot_stream_create", "ss_ctc_spot_stream_destroy", "ss_ctc_spot_stream_reset",
               "ss_ctc_spot_stream_advance", "ss_ctc_spot_stream_advance_host", "ss_debug_ctc_spot_stream_create",
               "ss_op_ctc_spot_stream_advance", "ss_debug_ctc_spot_trace_host", "ss_debug_ctc_spot_phases")


def keyword_set(V, n, transcripts, pad, seed):
    import numpy as np
    rng = np.random.default_rng(seed)
    seen, phrases = set(), []
    for toks in transcripts:
        for p in zip(toks, toks[1:]):
            if len(phrases) < 20 and pad not in p and p not in seen:
                seen.add(p)
                phrases.append(list(p))
    while len(phrases) < n:
        p = tuple(int(v) for v in rng.integers(4, V, int(rng.integers(1, 7))))
        if p not in seen:
            seen.add(p)
            phrases.append(list(p))
    return phrases


class PoolSide:
    """N ASR sessions of one pool, a pass over the whole feed -> the median of the timed steps in ms."""

    def __init__(self, model, N, segs, spot=None):
        from streamspeech_amd.text_pool import TextSessionPool
        self.segs = segs
        self.pool = TextSessionPool(model, N, MAX_ROWS, spot=spot) if spot is not None else TextSessionPool(model, N, MAX_ROWS)
        args = _args()
        self.sids = [self.pool.open("asr", args) for _ in range(N)]

    def run(self):
        import torch
        for sid in self.sids:
            self.pool.reset(sid)
        ms = []
        for k in range(len(self.segs[0])):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            self.pool.step({sid: self.segs[i][k] for i, sid in enumerate(self.sids)})
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ms[-TIMED_STEPS:])


def child():
    """The parent build's side: `pass` -> the scored greedy call's pass median in ms; `pool N` -> a pool pass; `quit` ends."""
    from streamspeech_amd import lib as L
    for name in NEW_SYMBOLS:                                     # the parent build has none of them
        L.SIGNATURES.pop(name, None)
    m, enc, Tp = _setup()
    segs = {N: _segments(N) for N in POOL_N}
    pools = {N: PoolSide(m, N, segs[N]) for N in POOL_N}
    print("ready", flush=True)
    for line in sys.stdin:
        f = line.split()
        if not f or f[0] == "quit":
            break
        if f[0] == "warm":
            m.batch_ctc_greedy(HEAD, enc, Tp, return_scores=True)
            for p in pools.values():
                p.run()
            print("ok", flush=True)
        elif f[0] == "pool":
            print(pools[int(f[1])].run(), flush=True)
        else:
            print(statistics.median(_timed(lambda: m.batch_ctc_greedy(HEAD, enc, Tp, return_scores=True)) for _ in range(CALLS)), flush=True)


def measure(out_path, parent_lib):
    import torch
    from streamspeech_amd import lib as L
    from streamspeech_amd.keywords import CtcKeywords
    m, enc, Tp = _setup()
    V = m.cfg.src_vocab
    passes = int(os.environ.get("SS_BENCH_PASSES", "7"))
    greedy = m.batch_ctc_greedy(HEAD, enc, Tp, return_scores=True)
    logits = m.last_logits().clone()
    sets = {n: CtcKeywords(keyword_set(V, n, [g[0] for g in greedy], m.cfg.pad, n), 1.0, V, m.cfg.pad, m.cfg.unk) for n in (100, 4000)}
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
        sides = {"greedy": lambda: m.batch_ctc_greedy(HEAD, enc, Tp, return_scores=True),
                 "spot100": lambda: m.batch_ctc_spot(HEAD, enc, Tp, sets[100], MAX_HITS),
                 "spot4000": lambda: m.batch_ctc_spot(HEAD, enc, Tp, sets[4000], MAX_HITS)}
        got = {k: fn() for k, fn in sides.items()}               # warm-up: scratch growth, first launches, the tables' upload
        segs = {N: _segments(N) for N in POOL_N}
        pools = {(N, k): PoolSide(m, N, segs[N], spot=sets[100] if k == "spot" else None) for N in POOL_N for k in ("plain", "spot")}
        for p in pools.values():
            p.run()
        if par:
            assert ask("warm") == "ok"
        med = {k: [] for k in list(sides) + (["parent"] if par else [])}
        pmed = {f"{k}_{N}": [] for N in POOL_N for k in ("plain", "spot", "parent") if k != "parent" or par}
        for _ in range(passes):
            for k, fn in sides.items():
                med[k].append(statistics.median(_timed(fn) for _ in range(CALLS)))
            if par:
                med["parent"].append(float(ask("pass")))
            for N in POOL_N:
                for k in ("plain", "spot"):
                    pmed[f"{k}_{N}"].append(pools[(N, k)].run())
                if par:
                    pmed[f"parent_{N}"].append(float(ask(f"pool {N}")))
        # the kernels apart, on the pack's own logits
        B, ld = len(Tp), int(logits.shape[1])
        hbuf = torch.empty((B * MAX_HITS * 24 + B * 16,), dtype=torch.uint8, device=m.device)
        tp = (C.c_int32 * B)(*Tp)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        kern = {}
        for n, kw in sets.items():
            def op():
                L.check(m.lib.ss_op_ctc_spot(s, C.c_void_p(logits.data_ptr()), ld, B, tp, kw.h, MAX_HITS, C.c_void_p(hbuf.data_ptr()),
                                             C.c_void_p(hbuf.data_ptr() + B * MAX_HITS * 24)), "ss_op_ctc_spot")
            op()
            for name, mask in (("gather", 1), ("dp", 2), ("all", 7)):
                L.check(m.lib.ss_debug_ctc_spot_phases(mask))
                kern[f"{name}_{n}_ms"] = round(statistics.median(_timed(op) for _ in range(3 * CALLS)), 4)
            L.check(m.lib.ss_debug_ctc_spot_phases(7))
    finally:
        if par:
            par.stdin.write("quit\n")
            par.stdin.flush()
            par.wait(timeout=60)
    row = {"head": HEAD, "utterances": len(Tp), "frames": sum(Tp), "longest_frames": max(Tp), "max_hits": MAX_HITS,
           "passes_per_side": passes, "calls_per_pass": CALLS, **{k: _side(v) for k, v in med.items()},
           "hits": {k: sum(len(h) for h in got[k]) for k in ("spot100", "spot4000")}, "kernels": kern,
           "pool": {k: _side(v) for k, v in pmed.items()}}
    for k in ("spot100", "spot4000"):
        row[f"ratio_{k}_over_greedy"] = round(row[k]["call_ms_median"] / row["greedy"]["call_ms_median"], 4)
    for N in POOL_N:
        row[f"pool_ratio_spot_over_plain_{N}"] = round(row["pool"][f"spot_{N}"]["call_ms_median"] / row["pool"][f"plain_{N}"]["call_ms_median"], 4)
    if par:
        r = row["greedy"]["call_ms_median"] / row["parent"]["call_ms_median"]
        row["ratio_greedy_over_parent"] = round(r, 4)
        row["greedy_inside_parent_spread"] = bool(1.0 / row["parent"]["spread"] <= r <= row["parent"]["spread"])
        for N in POOL_N:
            r = row["pool"][f"plain_{N}"]["call_ms_median"] / row["pool"][f"parent_{N}"]["call_ms_median"]
            row[f"pool_ratio_plain_over_parent_{N}"] = round(r, 4)
            sp = row["pool"][f"parent_{N}"]["spread"]
            row[f"pool_plain_inside_parent_spread_{N}"] = bool(1.0 / sp <= r <= sp)
    print(json.dumps(row), flush=True)
    res = {"tool": "tools/ctc_spot_bench.py", "device": torch.cuda.get_device_name(0),
           "order": "alternating passes: greedy, spot100, spot4000, parent, then the pools plain / spot / parent at each N",
           "tau": 1.0, "sets": {str(n): {"keywords": k.n_keywords, "labels": k.n_labels, "states": k.states, "workgroups": k.workgroups,
                                         "device_bytes": k.device_bytes} for n, k in sets.items()},
           "pool_feed": "320-ms segments, 10 s of history, the median of the last 5 steps (pool entries: call_ms = step_ms)",
           "parent_lib": bool(parent_lib), "result": row}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="libstreamspeech_hip.so of the parent commit: its greedy call and pool are timed beside this tree's")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child()
    else:
        measure(a.out, a.parent_lib)
