"""What endpointing costs a pool step.  1 / 16 / 64 S2ST sessions of the synthetic checkpoint are fed 8-kHz mu-law in 320-ms chunks
and answer mu-law at 8 kHz: eight seconds of line noise with two speech bursts each, the sessions staggered by up to 2.2 s so that
speakers and silent sessions share steps.  Two sides per size, on the same audio:
  endpointed   the sessions are opened with endpoint=Endpoint(): one ss_vad_scan and one synchronised download of its result records
               per step, silent sessions hold no slot
  caller-cut   plain pcm_in sessions fed, step for step, exactly the slices and finished flags the endpointed run committed (a caller
               that knew the utterance ranges and ran its own detector for free); steps in which nobody is inside an utterance push
               nothing and cost nothing
Per side: wall time of a step (synchronised before and after; median and p95 over the steps of all passes in which somebody is inside
an utterance), the front-end share of it (the pool's frontend_s: staging, scatter, scan and its synchronisation, fbank), and for the
endpointed side the steps in which everybody is silent (the scan alone) and the slots held over the steps of a pass.

  python tools/pooled_endpoint_bench.py --out profiles/pooled_endpoint.json      SS_BENCH_PASSES passes (default 3)
  python tools/pooled_endpoint_bench.py --merge RUN1.json RUN2.json --out profiles/pooled_endpoint.json    pools the passes of runs"""
import argparse
import json
import os
import statistics
import sys
import time

SIZES, SR, CHUNK_MS, TOTAL_MS, MAX_ROWS = (1, 16, 64), 8000, 320, 8000, 384
BURSTS = ((400, 1600), (3000, 4200))


def _args_of(cls, sr, seg_ms, extra=()):
    p = argparse.ArgumentParser()
    cls.add_args(p)
    a = p.parse_args(["--model-path", "synthetic:0", "--data-bin", "/nonexistent", "--sample-rate", str(sr), *extra])
    a.source_segment_size = seg_ms
    return a


def _p95(v):
    s = sorted(v)
    return s[min(len(s) - 1, int(0.95 * len(s)))]


def _stream(i):
    """Session i's line: noise at -70 dBFS, two bursts at -25 dBFS shifted by (i mod 8) chunks, as mu-law bytes."""
    import numpy as np
    from streamspeech_amd import pcm
    rng = np.random.default_rng(4000 + i)
    x = rng.standard_normal(SR * TOTAL_MS // 1000) * 10.0 ** (-70 / 20.0)
    for a, b in BURSTS:
        lo, hi = ((a + (i % 8) * CHUNK_MS) * SR // 1000, (b + (i % 8) * CHUNK_MS) * SR // 1000)
        x[lo:hi] += rng.standard_normal(hi - lo) * 10.0 ** (-25 / 20.0)
    return pcm.encode_host(x.astype(np.float32), "ulaw")


def _summary(t, fe):
    if not t:
        return {"steps": 0}
    return {"steps": len(t), "step_ms_median": round(1e3 * statistics.median(t), 4), "step_ms_p95": round(1e3 * _p95(t), 4),
            "frontend_ms_median": round(1e3 * statistics.median(fe), 4),
            "frontend_share": round(sum(fe) / sum(t), 4)}


def measure(out_path):
    import torch
    from streamspeech_amd import synth
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.config import ModelConfig, VocoderConfig
    from streamspeech_amd.endpoint import Endpoint
    from streamspeech_amd.engine import HipModel, HipVocoder
    from streamspeech_amd.pcm import PcmFormat, PcmOut
    from streamspeech_amd.speech_pool import SpeechSessionPool
    if not torch.cuda.is_available():
        raise SystemExit("pooled_endpoint_bench measures on the GPU; a CPU run provides no timing")
    cfg, vcfg = ModelConfig(), VocoderConfig()
    m = HipModel(synth.make_model_state_dict(0, cfg), cfg)
    voc = HipVocoder(synth.make_vocoder_state_dict(0, vcfg), vcfg)
    passes = int(os.environ.get("SS_BENCH_PASSES", "3"))
    args = _args_of(StreamSpeechS2STAgent, SR, CHUNK_MS, ("--vocoder", "synthetic:0", "--dur-prediction"))
    per = SR * CHUNK_MS // 1000
    runs = []
    for n in SIZES:
        data = [_stream(i) for i in range(n)]
        n_steps = -(-len(data[0]) // per)
        # ---- endpointed ----
        pool = SpeechSessionPool(m, n, MAX_ROWS, vocoder=voc)
        sids = [pool.open("s2st", args, pcm_in=PcmFormat("ulaw"), pcm_out=PcmOut("ulaw", SR), endpoint=Endpoint()) for _ in range(n)]
        busy_t, busy_fe, idle_t, idle_fe, commits, slots, utts = [], [], [], [], [], [], 0
        for p in range(passes + 1):                   # pass 0 warms every shape up
            for sid in sids:
                pool.reset(sid)
            k = 0
            while k < n_steps or any(s.pending for s in pool.sessions.values()):
                if k < n_steps:
                    for i, sid in enumerate(sids):
                        pool.push_pcm(sid, data[i][k * per:(k + 1) * per])
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pool.step()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                ls = pool.last_step
                if p == 1:
                    commits.append({i: ls["endpoint_commits"][sid] for i, sid in enumerate(sids) if sid in ls["endpoint_commits"]})
                    slots.append(n - len(pool.free))
                if p:
                    (busy_t if ls["endpoint_commits"] else idle_t).append(dt)
                    (busy_fe if ls["endpoint_commits"] else idle_fe).append(ls["frontend_s"])
                k += 1
            if p == 1:
                utts = sum(len(pool.utterances(sid)) for sid in sids)
        rec = {"sessions": n, "side": "endpointed", "steps_per_pass": len(commits), "utterances_per_pass": utts,
               "speaking_steps": _summary(busy_t, busy_fe), "silent_steps": _summary(idle_t, idle_fe),
               "slots_held_per_step": slots, "slots_held_max": max(slots), "_t": busy_t, "_fe": busy_fe, "_ti": idle_t, "_fi": idle_fe}
        print(json.dumps({k: v for k, v in rec.items() if not k.startswith("_")}), flush=True)
        runs.append(rec)
        del pool
        # ---- the same audio, cut by the caller at the ranges the first run reported ----
        pool = SpeechSessionPool(m, n, MAX_ROWS, vocoder=voc)
        sids = [pool.open("s2st", args, pcm_in=PcmFormat("ulaw"), pcm_out=PcmOut("ulaw", SR)) for _ in range(n)]
        t, fe = [], []
        for p in range(passes + 1):
            for sid in sids:
                pool.reset(sid)
            for row in commits:
                if not row:
                    continue                          # nobody inside an utterance: this caller pushes nothing
                for i, (a, cnt, fin) in row.items():
                    pool.push_pcm(sids[i], data[i][a:a + cnt], finished=fin)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                pool.step()
                torch.cuda.synchronize()
                dt = time.perf_counter() - t0
                if p:
                    t.append(dt)
                    fe.append(pool.last_step["frontend_s"])
                for i, (a, cnt, fin) in row.items():
                    if fin:
                        pool.reset(sids[i])
        rec = {"sessions": n, "side": "caller-cut", "speaking_steps": _summary(t, fe), "_t": t, "_fe": fe}
        print(json.dumps({k: v for k, v in rec.items() if not k.startswith("_")}), flush=True)
        runs.append(rec)
        del pool
        torch.cuda.empty_cache()
    write(out_path, {"workload": " ".join(__doc__.split("\n\n")[0].split()), "device": torch.cuda.get_device_name(0),
                     "passes": passes, "runs": runs})


def write(out_path, doc):
    """The table, and the raw step times next to each run so that --merge can pool them."""
    for a, b in zip(doc["runs"][0::2], doc["runs"][1::2]):
        if a["speaking_steps"].get("steps") and b["speaking_steps"].get("steps"):
            a["extra_ms_per_speaking_step_median"] = round(a["speaking_steps"]["step_ms_median"] - b["speaking_steps"]["step_ms_median"], 4)
    os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
    with open(out_path, "w") as f:
        json.dump(doc, f, indent=1)


def merge(paths, out_path):
    docs = []
    for p in paths:
        with open(p) as f:
            docs.append(json.load(f))
    doc = docs[0]
    for other in docs[1:]:
        for r, o in zip(doc["runs"], other["runs"]):
            assert (r["sessions"], r["side"]) == (o["sessions"], o["side"])
            for k in ("_t", "_fe", "_ti", "_fi"):
                if k in r:
                    r[k] += o[k]
        doc["passes"] += other["passes"]
    for r in doc["runs"]:
        r["speaking_steps"] = _summary(r["_t"], r["_fe"])
        if "_ti" in r:
            r["silent_steps"] = _summary(r["_ti"], r["_fi"])
    doc["merged_runs"] = len(docs)
    write(out_path, doc)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "pooled_endpoint.json"))
    ap.add_argument("--merge", nargs="+", help="run files of --out to pool into one table")
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    if a.merge:
        merge(a.merge, a.out)
    else:
        measure(a.out)
