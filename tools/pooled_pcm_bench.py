"""Raw PCM in and out of the session pools against the list-fed pools of the parent tree.  Two workloads:
  front-end   the workload of tools/pooled_frontend_bench.py -- 1 / 16 / 64 ASR sessions, all at 48 kHz, a 16 / 44.1 / 48-kHz mix and all
              at 16 kHz, fed 320-ms segments in lock step from silence to 20 s -- timed the same way: the segments are pushed first, then
              step() is timed up to the entry of the batched encoder step, where the tool synchronises.  A cell takes the median of the
              five steps that end at 20 s of history, one value per pass.
  s2st        the schedule of tools/pooled_speech_bench.py at 960 ms, N = 1 / 8 / 32 / 64 / 128: per pass the whole schedule's wall time
              per step (closed by a synchronise) and the hand-over -- from the vocoder tails ready to the contents the segments carry
              (lists or bytes) -- per writing step.  The tool synchronises when HipVocoder.batch_tail returns, on every tree alike, and
              takes the hand-over as the pool's vocoder_s minus the time inside batch_tail, so the same file measures a tree that has no
              handover_s key.
Audio is seeded synthetic PCM quantised to int16 once; a list-fed session gets s / 32768 as a Python list, a PCM-fed session the int16
bytes (and answers 16-bit PCM bytes).  --route list touches the pools through open / push / step / reset only and runs on an older tree.

  python tools/pooled_pcm_bench.py --route list|pcm --out run.json       one process: every cell, SS_BENCH_PASSES passes (default 6)
  python tools/pooled_pcm_bench.py --merge PCM*.json --list LIST*.json --parent PARENT*.json     -> profiles/pooled_pcm.json
Runs of the trees alternate in separate processes; the merge pools the passes of each side, reports median and spread
(max - min) / median per cell and applies the rule of §7c: a difference counts when it is larger than the two spreads together."""
import argparse
import json
import os
import statistics
import sys
import time

SEG_MS, MAX_ROWS, SECONDS, WINDOW = 320, 512, 20, 5
MIXES = {"48k": (48000,), "mix": (16000, 44100, 48000), "16k": (16000,)}
SESSIONS = (1, 16, 64)
S2ST_SEG_MS, S2ST_N, S2ST_MAX_ROWS, S2ST_MAX_SECONDS, SR = 960, (1, 8, 32, 64, 128), 384, 8, 16000


def _s16(seed, n):
    import numpy as np
    from streamspeech_amd import synth
    return np.round(synth.synth_pcm(seed, n) * 32767.0).astype("<i2")


def _args_of(cls, sr, seg_ms, extra=()):
    p = argparse.ArgumentParser()
    cls.add_args(p)
    a = p.parse_args(["--model-path", "synthetic:0", "--data-bin", "/nonexistent", "--sample-rate", str(sr), *extra])
    a.source_segment_size = seg_ms
    return a


def measure(route, out_path):
    import numpy as np
    import torch
    from streamspeech_amd import synth
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.agent_text import StreamSpeechASRAgent
    from streamspeech_amd.config import ModelConfig, VocoderConfig
    from streamspeech_amd.engine import HipModel, HipVocoder
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.speech_pool import SpeechSessionPool
    from streamspeech_amd.text_pool import TextSessionPool
    from streamspeech_amd.workload import make_utterances
    if not torch.cuda.is_available():
        raise SystemExit("pooled_pcm_bench measures on the GPU; a CPU run provides no timing")
    pcm_route = route == "pcm"
    if pcm_route:
        from streamspeech_amd.pcm import PcmFormat
        fmt = PcmFormat("s16le")
    cfg, vcfg = ModelConfig(), VocoderConfig()
    m = HipModel(synth.make_model_state_dict(0, cfg), cfg)
    passes = int(os.environ.get("SS_BENCH_PASSES", "6"))
    cells = []

    def save():                                        # after every group of cells: a run that dies late keeps what it measured
        os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
        with open(out_path, "w") as f:
            json.dump({"route": route, "passes": passes, "cells": cells}, f, indent=1)

    def feed(pool, sid, item, fin=False):
        if pcm_route:
            pool.push_pcm(sid, item, finished=fin)
        else:
            pool.push(sid, item)

    # ---- front-end ----------------------------------------------------------------------------------------------------------------
    n_steps = SECONDS * 1000 // SEG_MS
    win = list(range(n_steps - WINDOW, n_steps))
    items = {}
    for sr in (16000, 44100, 48000):
        step = sr * SEG_MS // 1000
        s = np.resize(_s16(900 + sr % 7, 16000 * 4), n_steps * step)
        if pcm_route:
            items[sr] = [s[k * step:(k + 1) * step].tobytes() for k in range(n_steps)]
        else:
            items[sr] = [SpeechSegment(content=(s[k * step:(k + 1) * step].astype(np.float64) / 32768).tolist(), sample_rate=sr,
                                       finished=False) for k in range(n_steps)]
    for N in [int(x) for x in os.environ.get("SS_BENCH_N", ",".join(map(str, SESSIONS))).split(",") if x]:
        for mix, rates in MIXES.items():
            pool = TextSessionPool(m, N, MAX_ROWS)
            sr_of = [rates[i % len(rates)] for i in range(N)]
            kw = {"pcm_in": fmt} if pcm_route else {}
            sids = [pool.open("asr", _args_of(StreamSpeechASRAgent, sr, SEG_MS), **kw) for sr in sr_of]
            mark, real = {}, pool.pool.forward

            def forward(*a, _real=real, _mark=mark, **k):
                torch.cuda.synchronize()
                _mark["t"] = time.perf_counter()
                return _real(*a, **k)
            pool.pool.forward = forward
            vals = []
            for p in range(passes + 1):                # pass 0 warms every shape up
                for sid in sids:
                    pool.reset(sid)
                t_step = []
                for k in range(n_steps):
                    for sid, sr in zip(sids, sr_of):
                        feed(pool, sid, items[sr][k])
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    pool.step()
                    t_step.append(mark["t"] - t0)
                torch.cuda.synchronize()
                if p:
                    vals.append(statistics.median(t_step[k] for k in win))
            rec = {"cell": f"frontend/{N}/{mix}", "frontend_ms": [round(1e3 * v, 4) for v in vals],
                   "pcm_uploads": pool.last_step.get("pcm_uploads"), "pcm_scatter_calls": pool.last_step.get("pcm_scatter_calls")}
            print(json.dumps(rec), flush=True)
            cells.append(rec)
            save()
            del pool
            torch.cuda.empty_cache()

    # ---- s2st ---------------------------------------------------------------------------------------------------------------------
    voc = HipVocoder(synth.make_vocoder_state_dict(0, vcfg), vcfg)
    tail_t, real_tail = {"s": 0.0}, HipVocoder.batch_tail

    def batch_tail(self, *a, **k):                     # the tails are READY when this returns, on every tree alike
        t = time.perf_counter()
        r = real_tail(self, *a, **k)
        torch.cuda.synchronize()
        tail_t["s"] += time.perf_counter() - t
        return r
    HipVocoder.batch_tail = batch_tail
    args = _args_of(StreamSpeechS2STAgent, SR, S2ST_SEG_MS, ("--vocoder", "synthetic:0", "--dur-prediction"))
    for N in [int(x) for x in os.environ.get("SS_BENCH_S2ST_N", ",".join(map(str, S2ST_N))).split(",") if x]:
        utts = make_utterances(N, 1234)
        step = SR * S2ST_SEG_MS // 1000
        segs = []
        for i, u in enumerate(utts):
            n = min(int(u.n_samples), S2ST_MAX_SECONDS * SR)
            s = _s16(700 + i, n)
            if pcm_route:
                segs.append([(s[p:p + step].tobytes(), p + step >= n) for p in range(0, n, step)])
            else:
                segs.append([(SpeechSegment(content=(s[p:p + step].astype(np.float64) / 32768).tolist(), sample_rate=SR,
                                            finished=p + step >= n), p + step >= n) for p in range(0, n, step)])
        start = [i % 8 for i in range(N)]
        steps, k = [], 0
        while True:
            row = [(i, segs[i][k - start[i]]) for i in range(N) if 0 <= k - start[i] < len(segs[i])]
            if not row and k > max(start):
                break
            if row:
                steps.append(row)
            k += 1
        pool = SpeechSessionPool(m, N, S2ST_MAX_ROWS, vocoder=voc)
        kw = {"pcm_in": fmt, "pcm_out": "s16le"} if pcm_route else {}
        sids = [pool.open("s2st", args, **kw) for _ in range(N)]
        total, hand, keyed, out_bytes = [], [], [], 0
        for p in range(passes + 1):
            for sid in sids:
                pool.reset(sid)
            h, hk = [], []
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for row in steps:
                for i, (item, fin) in row:
                    feed(pool, sids[i], item, fin)
                tail_t["s"] = 0.0
                out = pool.step()
                ls = pool.last_step
                if ls.get("speech_writers"):
                    h.append(ls["vocoder_s"] - tail_t["s"])
                    if "handover_s" in ls:
                        hk.append(ls["handover_s"])
                if p == 1:
                    out_bytes += sum(len(o.content) * (1 if pcm_route else 2) for o in out.values() if not o.is_empty)
            torch.cuda.synchronize()
            if p:
                total.append((time.perf_counter() - t0) / len(steps))
                hand.append(statistics.mean(h) if h else float("nan"))
                if hk:
                    keyed.append(statistics.mean(hk))
        rec = {"cell": f"s2st/{N}", "steps": len(steps), "writing_steps": len(h), "pcm16_bytes_out_per_pass": out_bytes,
               "step_ms": [round(1e3 * v, 4) for v in total], "handover_ms": [round(1e3 * v, 4) for v in hand]}
        if keyed:
            rec["handover_s_key_ms"] = [round(1e3 * v, 4) for v in keyed]
        print(json.dumps(rec), flush=True)
        cells.append(rec)
        save()
        del pool
        torch.cuda.empty_cache()


SERIES = ("frontend_ms", "step_ms", "handover_ms")


def _series(paths):
    """{(cell, series): every pass value of the runs in `paths`}"""
    out = {}
    for p in paths:
        with open(p) as f:
            for c in json.load(f)["cells"]:
                for k in SERIES:
                    if k in c:
                        out.setdefault((c["cell"], k), []).extend(c[k])
    return out


def _stat(v):
    med = statistics.median(v)
    return {"median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 3), "n": len(v)}


def merge(pcm_paths, list_paths, parent_paths, out_path):
    new, lst, old = _series(pcm_paths), _series(list_paths), _series(parent_paths)
    rows = []
    verdict = {"gated_not_faster": [], "pcm_slower_than_parent": [], "list_slower_than_parent": []}
    for key in sorted(old, key=lambda k: (k[0].split("/")[0], k[1], int(k[0].split("/")[1]), k[0])):
        cell, series = key
        b = _stat(old[key])
        row = {"cell": cell, "metric": series, "parent_list": b}
        for name, side, slow in (("pcm", new, "pcm_slower_than_parent"), ("list", lst, "list_slower_than_parent")):
            if key not in side:
                continue
            a = _stat(side[key])
            both = a["spread"] * a["median_ms"] + b["spread"] * b["median_ms"]      # the two spreads together, in ms
            row[name] = a
            row[name + "_speedup"] = round(b["median_ms"] / a["median_ms"], 2)
            if a["median_ms"] > b["median_ms"] + both:
                verdict[slow].append(f"{cell}:{series}")
            n = int(cell.split("/")[1])
            gated = (series == "frontend_ms" and n >= 16) or (series == "handover_ms" and n >= 32)
            if name == "pcm" and gated and not a["median_ms"] < b["median_ms"] - both:
                verdict["gated_not_faster"].append(f"{cell}:{series}")
        rows.append(row)
    res = {"workload": " ".join(__doc__.split("\n\n")[0].split()), "runs": {"pcm": len(pcm_paths), "list": len(list_paths),
                                                                            "parent": len(parent_paths)},
           "rule": "a difference counts when it is larger than the two spreads (max - min of the pooled passes) together",
           "cells": rows, "acceptance_misses": verdict}
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
    for r in rows:
        line = f'{r["cell"]:16s} {r["metric"]:12s} parent {r["parent_list"]["median_ms"]:9.3f} ms ({r["parent_list"]["spread"]:.2f})'
        for name in ("list", "pcm"):
            if name in r:
                line += f'   {name} {r[name]["median_ms"]:9.3f} ms ({r[name]["spread"]:.2f}) x{r[name + "_speedup"]}'
        print(line)
    print(json.dumps(verdict))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--route", choices=("list", "pcm"), default="pcm")
    ap.add_argument("--out", default=os.path.join("profiles", "pooled_pcm_run.json"))
    ap.add_argument("--merge", nargs="+", help="runs of this tree, --route pcm")
    ap.add_argument("--list", nargs="+", default=[], help="runs of this tree, --route list")
    ap.add_argument("--parent", nargs="+", default=[], help="runs of the parent tree, --route list")
    ap.add_argument("--table", default=os.path.join("profiles", "pooled_pcm.json"))
    a = ap.parse_args()
    if a.merge:
        merge(a.merge, a.list, a.parent, a.table)
    else:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        measure(a.route, a.out)
