"""MP3 streams into the session pools against the same audio pushed as 16-bit PCM, on one tree and one machine.
1 / 16 / 64 ASR sessions are fed 320-ms chunks in lock step from silence to the end of their clip: the two example clips (48 kHz, 64
kbit/s: 2560 bytes per chunk) and streams written by tests/mp3_writer.py at 16 and 24 kHz (MPEG-2; random spectra, so the Huffman work
is that of a dense stream).  The PCM route gets, step by step, exactly as many samples as the MP3 sessions released at that step, as
s16le.  Both routes run in ONE process, a pass of one after a pass of the other (pass 0 of each warms every shape up), so clocks and
allocator state are shared and the order is interleaved.  Per step and route:
  host_ms      the pushes of all sessions (MP3: the bitstream parse, Huffman included; PCM: a view of the bytes)
  frontend_ms  step() up to the entry of the batched encoder step, where the tool synchronises: staging, upload, decode / scatter, fbank
  mp3_stage_ms of that, the MP3 route's own part -- arena copies, upload, ss_mp3_stream_synthesize -- closed by a synchronise
  encoder_ms   from there to the end of step() (encoder step, CTC heads, host gate)
A cell reports the median over the steps of a pass, one value per pass, then median and spread (max - min) / median over passes.

  python tools/pooled_mp3_bench.py [--out profiles/pooled_mp3.json]        SS_BENCH_PASSES passes (default 5), SS_BENCH_N sessions"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG_MS, MAX_ROWS, SESSIONS = 320, 512, (1, 16, 64)


def _args_of(cls, sr):
    p = argparse.ArgumentParser()
    cls.add_args(p)
    a = p.parse_args(["--model-path", "synthetic:0", "--data-bin", "/nonexistent", "--sample-rate", str(sr)])
    a.source_segment_size = SEG_MS
    return a


def _sources():
    """name -> (sample rate, [MP3 bytes of a clip, ...])"""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mp3_writer as Wr
    gold = os.path.join(ROOT, "tests", "golden", "mp3")
    out = {"examples_48k": (48000, [open(os.path.join(gold, f), "rb").read() for f in sorted(os.listdir(gold)) if f.endswith(".mp3")])}
    for sr in (16000, 24000):
        rng = np.random.default_rng(sr)
        frames = 4 * sr // 576                         # MPEG-2: one granule per frame; four seconds
        blocks = [(0, False), (1, False), (2, False), (3, False)]
        clips = [Wr.write_stream(Wr.sequence(rng, frames, 1, 1, blocks, lsf=True), sr)[0]]     # the writer's top bitrate, 160 kbit/s
        out[f"writer_{sr // 1000}k"] = (sr, clips)
    return out


def _stat(v):
    med = statistics.median(v)
    return {"median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 3) if med else 0.0, "n": len(v)}


def measure(out_path):
    import numpy as np
    import torch
    from streamspeech_amd import mp3, synth
    from streamspeech_amd.agent_text import StreamSpeechASRAgent
    from streamspeech_amd.config import ModelConfig
    from streamspeech_amd.engine import HipModel
    from streamspeech_amd.pcm import PcmFormat
    from streamspeech_amd.text_pool import TextSessionPool
    if not torch.cuda.is_available():
        raise SystemExit("pooled_mp3_bench measures on the GPU; a CPU run provides no timing")
    cfg = ModelConfig()
    m = HipModel(synth.make_model_state_dict(0, cfg), cfg)
    passes = int(os.environ.get("SS_BENCH_PASSES", "5"))
    cells = []
    for src, (sr, clips) in _sources().items():
        pcm16 = [np.round(np.clip(t.cpu().numpy(), -1, 1) * 32767.0).astype("<i2") for t, _ in mp3.decode_batch(clips, m.device)]
        nbytes = [max(1, round(len(c) * SEG_MS / 1000 / (len(p) / sr))) for c, p in zip(clips, pcm16)]      # bytes of 320 ms
        n_steps = min(-(-len(c) // b) for c, b in zip(clips, nbytes))
        for N in [int(x) for x in os.environ.get("SS_BENCH_N", ",".join(map(str, SESSIONS))).split(",") if x]:
            pools = {r: TextSessionPool(m, N, MAX_ROWS) for r in ("mp3", "s16le")}
            sids = {"mp3": [pools["mp3"].open("asr", _args_of(StreamSpeechASRAgent, sr), mp3_in=True) for _ in range(N)],
                    "s16le": [pools["s16le"].open("asr", _args_of(StreamSpeechASRAgent, sr), pcm_in=PcmFormat("s16le")) for _ in range(N)]}
            mark, stage_t = {}, {"s": 0.0}
            for pool in pools.values():
                def forward(*a, _real=pool.pool.forward, **k):
                    torch.cuda.synchronize()
                    mark["t"] = time.perf_counter()
                    return _real(*a, **k)
                pool.pool.forward = forward

            def mp3_stage(sessions, _real=pools["mp3"]._mp3_stage):
                t = time.perf_counter()
                r = _real(sessions)
                torch.cuda.synchronize()
                stage_t["s"] = time.perf_counter() - t
                return r
            pools["mp3"]._mp3_stage = mp3_stage
            series = {r: {"host_ms": [], "frontend_ms": [], "encoder_ms": []} for r in pools}
            series["mp3"]["mp3_stage_ms"] = []
            gained = None                              # samples each session released per step, learnt from the MP3 pass
            for p in range(passes + 1):
                for route in ("mp3", "s16le"):
                    pool = pools[route]
                    for sid in sids[route]:
                        pool.reset(sid)
                    host, front, enc, stg, gain = [], [], [], [], []
                    pos = [0] * N
                    for k in range(n_steps):
                        t0 = time.perf_counter()
                        for i, sid in enumerate(sids[route]):
                            c = i % len(clips)
                            if route == "mp3":
                                pool.push_mp3(sid, clips[c][k * nbytes[c]:(k + 1) * nbytes[c]])
                            else:
                                n = gained[k][i]
                                pool.push_pcm(sid, pcm16[c][pos[i]:pos[i] + n])
                                pos[i] += n
                        host.append(time.perf_counter() - t0)
                        if route == "mp3":
                            gain.append([pool.sessions[sid].mp3_chunk.released for sid in sids[route]])
                        torch.cuda.synchronize()
                        mark["t"] = None
                        t0 = time.perf_counter()
                        pool.step()
                        t1 = time.perf_counter()
                        if mark["t"] is not None:      # steps that encode
                            front.append(mark["t"] - t0)
                            enc.append(t1 - mark["t"])
                            if route == "mp3":
                                stg.append(stage_t["s"])
                    torch.cuda.synchronize()
                    if route == "mp3":
                        gained = gain
                    if p:
                        series[route]["host_ms"].append(1e3 * statistics.median(host))
                        series[route]["frontend_ms"].append(1e3 * statistics.median(front))
                        series[route]["encoder_ms"].append(1e3 * statistics.median(enc))
                        if route == "mp3":
                            series[route]["mp3_stage_ms"].append(1e3 * statistics.median(stg))
            ls = pools["mp3"].last_step
            rec = {"cell": f"{src}/{N}", "sample_rate": sr, "steps": n_steps, "chunk_bytes": nbytes,
                   "mp3_uploads": ls["mp3_uploads"], "mp3_synth_calls": ls["mp3_synth_calls"], "mp3_granules_last_step": ls["mp3_granules"]}
            for route in pools:
                rec[route] = {k: _stat(v) for k, v in series[route].items()}
            rec["mp3_stage_over_encoder"] = round(rec["mp3"]["mp3_stage_ms"]["median_ms"] / rec["mp3"]["encoder_ms"]["median_ms"], 3)
            print(json.dumps(rec), flush=True)
            cells.append(rec)
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "w") as f:             # after every cell: a run that dies late keeps what it measured
                json.dump({"workload": " ".join(__doc__.split("\n\n")[0].split()), "passes": passes, "device": torch.cuda.get_device_name(0),
                           "cells": cells}, f, indent=1)
            del pools
            torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "pooled_mp3.json"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    measure(a.out)
