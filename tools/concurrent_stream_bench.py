"""Read path of N concurrent streaming sessions (320-ms chunks: attention / conv chunk 8, 32 new fbank frames per step): the encoder
step and both CTC heads of every live session, as ONE batched step of a session pool (engine.StreamPool) against the same sessions
round-robin through N standalone contexts (one HipModel context + scratch set per session, encoder_stream_forward + both heads, one
session after the other on one stream).  Utterance lengths of the seeded synthetic CVSS-shaped workload (workload.make_utterances),
starts staggered over 8 steps so the sessions sit at different lengths and chunk phases.  The batched step is also timed with a
synchronisation between the encoder and the heads, for the encoder / heads split.  Whole schedules are
timed (every shape warmed up by an untimed pass first), batched and round-robin runs alternate in one process, medians reported.
Covers the read path only: the write path (MT, T2U, unit decoder, vocoder) stays per session and is not measured here.
Run on the GPU box: python tools/concurrent_stream_bench.py  -> profiles/concurrent_streams.json"""
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from streamspeech_amd import synth  # noqa: E402
from streamspeech_amd.config import ModelConfig  # noqa: E402
from streamspeech_amd.engine import HipModel  # noqa: E402
from streamspeech_amd.workload import make_utterances  # noqa: E402

CHUNK, STEP_FRAMES, MAX_ROWS = 8, 32, 384


def schedule(N, seed=1234):
    secs = np.array([u.seconds for u in make_utterances(N, seed)])
    L = [max(40, int(u.n_samples - 400) // 160 + 1) for u in make_utterances(N, seed)]      # fbank frames of the utterance
    start = [i % 8 for i in range(N)]
    steps, k = [], 0
    while True:
        row = []
        for i in range(N):
            j = k - start[i]
            if j < 0:
                continue
            T = 40 + STEP_FRAMES * j
            if T - STEP_FRAMES >= L[i]:
                continue
            row.append((i, min(T, L[i])))
        if not row and k > max(start):
            break
        if row:
            steps.append(row)
        k += 1
    return float(np.sum(secs)), L, steps


def run_pool(pool, fb, steps, split=None):
    for s in range(pool.max_sessions):
        pool.reset(s)
    for row in steps:
        slots = [i for i, _ in row]
        t0 = time.perf_counter()
        pool.forward(slots, [fb[i][T] for i, T in row], [CHUNK] * len(row), [CHUNK] * len(row))
        if split is not None:
            torch.cuda.synchronize()
            t1 = time.perf_counter()
        pool.ctc_both()                            # both heads, one device-to-host copy
        if split is not None:
            split[0] += t1 - t0
            split[1] += time.perf_counter() - t1
    torch.cuda.synchronize()


def run_rr(ctxs, fb, steps):
    for c in ctxs:
        c.encoder_stream_reset()
    for row in steps:
        for i, T in row:
            enc = ctxs[i].encoder_stream_forward(fb[i][T], CHUNK, CHUNK)
            ctxs[i].ctc_greedy(0, enc)
            ctxs[i].ctc_greedy(1, enc)
    torch.cuda.synchronize()


def main():
    cfg = ModelConfig()
    m = HipModel(synth.make_model_state_dict(0, cfg), cfg)
    res = {"workload": __doc__.split("\n\n")[0].replace("\n", " "), "chunk_rows": CHUNK,
           "pool_ffn_form": "two-launch", "runs": []}
    Ns = [int(x) for x in os.environ.get("SS_BENCH_N", "1,8,32,64,128").split(",")]
    for N in Ns:
        audio_s, L, steps = schedule(N)
        full = [torch.from_numpy(synth.synth_fbank(500 + i, L[i])).cuda() for i in range(N)]
        fbv = [{} for _ in range(N)]               # every prefix a session is fed, made once (the front-end is not timed here)
        for row in steps:
            for i, T in row:
                fbv[i][T] = full[i][:T].contiguous()
        pool = m.stream_pool(N, MAX_ROWS)
        ctxs = [m.new_context() for _ in range(N)]
        for c in ctxs:
            c.ctc_speculate = True
        run_pool(pool, fbv, steps)                 # warm-up: every shape once
        run_rr(ctxs, fbv, steps)
        tp, tr = [], []
        l0 = pool.stats()[0]
        reps = 3 if N <= 32 else 2
        for _ in range(reps):                      # alternate batched and round-robin
            t0 = time.perf_counter(); run_pool(pool, fbv, steps); tp.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); run_rr(ctxs, fbv, steps); tr.append(time.perf_counter() - t0)
        launches = (pool.stats()[0] - l0) / (reps * len(steps))
        p, r = statistics.median(tp), statistics.median(tr)
        split = [0.0, 0.0]
        run_pool(pool, fbv, steps, split)
        rec = {"N": N, "steps": len(steps), "session_steps": sum(len(x) for x in steps), "audio_s": round(audio_s, 2),
               "batched_ms_per_step": round(1e3 * p / len(steps), 3), "batched_launches_per_step": round(launches, 1),
               "batched_rtf": round(audio_s / p, 1),
               "batched_encoder_ms_per_step": round(1e3 * split[0] / len(steps), 3),
               "batched_heads_ms_per_step": round(1e3 * split[1] / len(steps), 3),
               "round_robin_ms_per_step": round(1e3 * r / len(steps), 3), "round_robin_rtf": round(audio_s / r, 1),
               "speedup": round(r / p, 2), "timed_reps": reps}
        print(json.dumps(rec), flush=True)
        res["runs"].append(rec)
        del pool, ctxs
        torch.cuda.empty_cache()
    os.makedirs("profiles", exist_ok=True)
    with open(os.environ.get("SS_BENCH_OUT", os.path.join("profiles", "concurrent_streams.json")), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
