"""Front-end time of a TextSessionPool step against the length of the history: 1 / 16 / 64 ASR sessions, all at 48 kHz, a 16 / 44.1 /
48-kHz mix and all at 16 kHz, fed 320-ms segments in lock step up to 20 s, and the single S2TT agent's READ pushpop at 48 kHz (a gate
that never writes before the source ends: front-end + encoder step + CTC heads, no search).  The front-end time of a step is what the
pool's own clock brackets (the sessions' staging, the fbank rows, no admission) closed by a device synchronisation: the segments are
pushed first, then step() is timed up to the entry of the batched encoder step, where the tool synchronises.  Each pass runs all
sessions from silence to 20 s; a cell (sessions, mix, history) takes the median of the five steps that end at 2 / 10 / 20 s of history,
one value per pass.  The tool touches the pool through open / push / step / reset only, so the same file measures an older tree.

  python tools/pooled_frontend_bench.py --out run.json          one process: every cell, SS_BENCH_PASSES passes (default 5)
  python tools/pooled_frontend_bench.py --merge new*.json --parent old*.json   -> profiles/pooled_frontend.json
Runs of the two trees alternate in separate processes; the merge pools the passes of each tree, reports median and
spread (max - min) / median per cell and checks the acceptance rules written there."""
import argparse
import json
import os
import statistics
import sys
import time

SEG_MS, MAX_ROWS, SECONDS = 320, 512, 20
HISTORIES = (2, 10, 20)
MIXES = {"48k": (48000,), "mix": (16000, 44100, 48000), "16k": (16000,)}
SESSIONS = (1, 16, 64)
WINDOW = 5                                             # steps per cell and pass


def _windows():
    """{history seconds: the step indices (0-based) of the WINDOW steps that end where the history reaches it}."""
    return {h: list(range(h * 1000 // SEG_MS - WINDOW, h * 1000 // SEG_MS)) for h in HISTORIES}


def measure(out_path):
    import numpy as np
    import torch
    from streamspeech_amd import synth
    from streamspeech_amd.agent_text import StreamSpeechASRAgent, StreamSpeechS2TTAgent
    from streamspeech_amd.config import ModelConfig
    from streamspeech_amd.engine import HipModel
    from streamspeech_amd.modules import StreamSpeechModel
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.text_pool import TextSessionPool

    def args_of(cls, sr, **over):
        p = argparse.ArgumentParser()
        cls.add_args(p)
        a = p.parse_args(["--model-path", "synthetic:0", "--data-bin", "/nonexistent", "--sample-rate", str(sr)])
        a.source_segment_size = SEG_MS
        for k, v in over.items():
            setattr(a, k, v)
        return a

    cfg = ModelConfig()
    m = HipModel(synth.make_model_state_dict(0, cfg), cfg)
    n_steps = SECONDS * 1000 // SEG_MS
    passes = int(os.environ.get("SS_BENCH_PASSES", "5"))
    segs = {}                                          # one segment list per rate, shared by the sessions at that rate
    for sr in (16000, 44100, 48000):
        step = sr * SEG_MS // 1000
        pcm = np.resize(synth.synth_pcm(900 + sr % 7, 16000 * 4), n_steps * step)
        segs[sr] = [SpeechSegment(content=pcm[k * step:(k + 1) * step].tolist(), sample_rate=sr, finished=False) for k in range(n_steps)]
    win = _windows()
    cells = []
    # the host share of the front-end: the sessions' staging (list -> float32 -> the device history), timed around the extractor's own
    # stage(); what is left of a step's front-end time is its launches, their allocations and the synchronisation
    from streamspeech_amd.frontend import OnlineFeatureExtractor
    staged, real_stage = {"s": 0.0}, OnlineFeatureExtractor.stage

    def stage(self, samples):
        t = time.perf_counter()
        r = real_stage(self, samples)
        staged["s"] += time.perf_counter() - t
        return r
    OnlineFeatureExtractor.stage = stage

    def save():                                        # after every group of cells: a run that dies late keeps what it measured
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump({"segment_ms": SEG_MS, "passes": passes, "window_steps": WINDOW, "cells": cells}, f, indent=1)
    for N in [int(x) for x in os.environ.get("SS_BENCH_N", ",".join(map(str, SESSIONS))).split(",")]:
        for mix, rates in MIXES.items():
            pool = TextSessionPool(m, N, MAX_ROWS)
            sr_of = [rates[i % len(rates)] for i in range(N)]
            sids = [pool.open("asr", args_of(StreamSpeechASRAgent, sr)) for sr in sr_of]
            mark, real = {}, pool.pool.forward

            def forward(*a, _real=real, _mark=mark, **k):
                torch.cuda.synchronize()
                _mark["t"] = time.perf_counter()
                return _real(*a, **k)
            pool.pool.forward = forward
            vals, rest = {h: [] for h in HISTORIES}, {h: [] for h in HISTORIES}
            for p in range(passes + 1):                # pass 0 warms every shape up
                for sid in sids:
                    pool.reset(sid)
                t_step, t_rest = [], []
                for k in range(n_steps):
                    for sid, sr in zip(sids, sr_of):
                        pool.push(sid, segs[sr][k])
                    torch.cuda.synchronize()
                    staged["s"] = 0.0
                    t0 = time.perf_counter()
                    pool.step()
                    t_step.append(mark["t"] - t0)
                    t_rest.append(mark["t"] - t0 - staged["s"])
                torch.cuda.synchronize()
                if p:
                    for h in HISTORIES:
                        vals[h].append(statistics.median(t_step[k] for k in win[h]))
                        rest[h].append(statistics.median(t_rest[k] for k in win[h]))
            for h in HISTORIES:
                rec = {"cell": f"pool/{N}/{mix}/{h}s", "sessions": N, "mix": mix, "history_s": h, "frontend_ms": [round(1e3 * v, 4) for v in vals[h]],
                       "after_staging_ms": [round(1e3 * v, 4) for v in rest[h]], "frontend_calls": pool.last_step.get("frontend_calls")}
                print(json.dumps(rec), flush=True)
                cells.append(rec)
            save()
            del pool
            torch.cuda.empty_cache()
    # the single agent's READ call at 48 kHz (lagging_k1 past any source: the gate reads until the source ends)
    agent = StreamSpeechS2TTAgent(args_of(StreamSpeechS2TTAgent, 48000, lagging_k1=1 << 20), model=StreamSpeechModel.from_engine(m))
    vals = {h: [] for h in HISTORIES}
    for p in range(passes + 1):
        agent.reset()
        t_step = []
        for k in range(n_steps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            o = agent.pushpop(segs[48000][k])
            torch.cuda.synchronize()
            t_step.append(time.perf_counter() - t0)
            assert o.is_empty, "the gate wrote"
        if p:
            for h in HISTORIES:
                vals[h].append(statistics.median(t_step[k] for k in win[h]))
    for h in HISTORIES:
        rec = {"cell": f"agent/48k/{h}s", "sessions": 1, "mix": "agent48k", "history_s": h, "read_call_ms": [round(1e3 * v, 4) for v in vals[h]]}
        print(json.dumps(rec), flush=True)
        cells.append(rec)
    save()


def _pool_cells(paths, key=None):
    """{cell: every pass value of the runs in `paths`} (`key`: another series of the pool cells)"""
    out = {}
    for p in paths:
        for c in json.load(open(p))["cells"]:
            if key is None or key in c:
                out.setdefault(c["cell"], []).extend(c[key] if key else c.get("frontend_ms") or c["read_call_ms"])
    return out


def _stat(v):
    med = statistics.median(v)
    return {"median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 3), "n": len(v)}


def merge(new_paths, parent_paths, out_path):
    new, old = _pool_cells(new_paths), _pool_cells(parent_paths)
    new_rest, old_rest = _pool_cells(new_paths, "after_staging_ms"), _pool_cells(parent_paths, "after_staging_ms")
    rows, verdict = [], {"slower": [], "not_faster": [], "grows_with_history": [], "changed_16k": []}
    for cell in new:
        a, b = _stat(new[cell]), _stat(old[cell])
        kind, n, mix, h = (cell.split("/") + [""])[:4] if cell.startswith("pool") else ("agent", "1", "agent48k", cell.split("/")[2])
        both = a["spread"] * a["median_ms"] + b["spread"] * b["median_ms"]     # the two spreads together, in ms
        row = {"cell": cell, "parent": b, "new": a, "speedup": round(b["median_ms"] / a["median_ms"], 2)}
        if cell in new_rest and cell in old_rest:                          # the same cell without the sessions' host staging
            row["after_staging"] = {"parent": _stat(old_rest[cell]), "new": _stat(new_rest[cell])}
        rows.append(row)
        if kind != "pool":
            continue
        n, h = int(n), int(h.rstrip("s"))
        if mix == "16k":
            if abs(a["median_ms"] - b["median_ms"]) > both:
                verdict["changed_16k"].append(cell)
            continue
        if a["median_ms"] > b["median_ms"] + both:
            verdict["slower"].append(cell)
        if (n >= 16 or h >= 10) and not a["median_ms"] < b["median_ms"] - both:
            verdict["not_faster"].append(cell)
        if h == HISTORIES[-1]:
            first = _stat(new[cell.rsplit("/", 1)[0] + f"/{HISTORIES[0]}s"])
            if abs(a["median_ms"] - first["median_ms"]) > max(a["spread"], first["spread"]) * first["median_ms"]:
                verdict["grows_with_history"].append(cell)
    res = {"workload": __doc__.split("\n\n")[0].replace("\n", " "), "segment_ms": SEG_MS, "window_steps": WINDOW,
           "runs": {"new": len(new_paths), "parent": len(parent_paths)}, "cells": rows, "acceptance_misses": verdict}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    for r in rows:
        print(f'{r["cell"]:22s} parent {r["parent"]["median_ms"]:9.3f} ms ({r["parent"]["spread"]:.2f})   new {r["new"]["median_ms"]:9.3f} ms '
              f'({r["new"]["spread"]:.2f})   x{r["speedup"]}' + (f'   after staging {r["after_staging"]["parent"]["median_ms"]:.3f} -> '
                                                                  f'{r["after_staging"]["new"]["median_ms"]:.3f} ms' if "after_staging" in r else ""))
    print(json.dumps(verdict))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "pooled_frontend_run.json"))
    ap.add_argument("--merge", nargs="+", help="runs of this tree")
    ap.add_argument("--parent", nargs="+", help="runs of the tree measured against")
    ap.add_argument("--table", default=os.path.join("profiles", "pooled_frontend.json"))
    a = ap.parse_args()
    if a.merge:
        merge(a.merge, a.parent or [], a.table)
    else:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        measure(a.out)
