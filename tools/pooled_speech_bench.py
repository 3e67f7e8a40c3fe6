"""N concurrent simultaneous S2ST sessions at 320 and 960 ms: one SpeechSessionPool (streamspeech_amd/speech_pool.py) against N
single-session StreamSpeechS2STAgent instances, each on a model and vocoder context of its own, served round-robin on one stream.  Utterance lengths of the seeded
synthetic CVSS-shaped workload (workload.make_utterances) cut at 8 s, 16-kHz synthetic PCM, starts staggered over 8 steps as in
tools/concurrent_stream_bench.py.  Both sides get the same SpeechSegment objects; whole schedules are timed after an untimed warm-up
pass, pooled and round-robin runs alternate in one process, medians reported.  Per step of the pool: the total, the split into
front-end / encoder + CTC heads / MT search / units (MT feature pass + T2U + unit decoder) / vocoder tail, the sessions that wrote
speech, and audio seconds per wall second.
Run on the GPU box: python tools/pooled_speech_bench.py  -> profiles/pooled_speech.json  (SS_BENCH_N=64 SS_BENCH_SEG=960 for one size)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from streamspeech_amd import synth  # noqa: E402
from streamspeech_amd.agent import StreamSpeechS2STAgent  # noqa: E402
from streamspeech_amd.config import ModelConfig, VocoderConfig  # noqa: E402
from streamspeech_amd.engine import HipModel, HipVocoder  # noqa: E402
from streamspeech_amd.modules import StreamSpeechModel  # noqa: E402
from streamspeech_amd.simuleval_shim import SpeechSegment  # noqa: E402
from streamspeech_amd.speech_pool import SpeechSessionPool  # noqa: E402
from streamspeech_amd.workload import make_utterances  # noqa: E402

SR, MAX_ROWS = 16000, 384
MAX_SECONDS = 8                       # as tools/pooled_text_bench.py: the same cut of the workload's utterances


def agent_args(seg_ms):
    p = argparse.ArgumentParser()
    StreamSpeechS2STAgent.add_args(p)
    a = p.parse_args(["--model-path", "synthetic:0", "--data-bin", "/nonexistent", "--vocoder", "synthetic:0", "--dur-prediction",
                      "--sample-rate", str(SR)])
    a.source_segment_size = seg_ms
    return a


def schedule(N, seg_ms, seed=1234):
    """-> (audio seconds, steps): steps[k] = [(session, SpeechSegment)] of the sessions live at step k."""
    utts = make_utterances(N, seed)
    step = SR * seg_ms // 1000
    segs = []
    for i, u in enumerate(utts):
        n = min(int(u.n_samples), MAX_SECONDS * SR)                    # the final search of a longer source passes the decoder's positions
        pcm = synth.synth_pcm(700 + i, n)
        segs.append([SpeechSegment(content=pcm[p:p + step].tolist(), sample_rate=SR, finished=p + step >= n)
                     for p in range(0, n, step)])
    start = [i % 8 for i in range(N)]
    steps, k = [], 0
    while True:
        row = [(i, segs[i][k - start[i]]) for i in range(N) if 0 <= k - start[i] < len(segs[i])]
        if not row and k > max(start):
            break
        if row:
            steps.append(row)
        k += 1
    audio = sum(len(s) for ss in segs for s in (x.content for x in ss)) / SR
    return audio, steps


class _Voc:
    """CodeHiFiGANVocoderWithDur call surface over a HipVocoder context."""

    def __init__(self, hv):
        self.hip = hv

    def __call__(self, x, dur_prediction=False):
        from streamspeech_amd.modules import CodeHiFiGANVocoderWithDur
        return CodeHiFiGANVocoderWithDur.__call__(self, x, dur_prediction)


def run_pool(pool, sids, steps, stats=None):
    for sid in sids:
        pool.reset(sid)
    for row in steps:
        pool.step({sids[i]: seg for i, seg in row})
        if stats is not None:
            stats.append(dict(pool.last_step))
    torch.cuda.synchronize()


def run_rr(agents, steps):
    for a in agents:
        a.reset()
    for row in steps:
        for i, seg in row:
            agents[i].pushpop(seg)
    torch.cuda.synchronize()


def main():
    cfg, vcfg = ModelConfig(), VocoderConfig()
    m = HipModel(synth.make_model_state_dict(0, cfg), cfg)
    voc = HipVocoder(synth.make_vocoder_state_dict(0, vcfg), vcfg)
    res = {"workload": __doc__.split("\n\n")[0].replace("\n", " "), "runs": []}
    Ns = [int(x) for x in os.environ.get("SS_BENCH_N", "1,8,32,64,128").split(",")]
    segs = [int(x) for x in os.environ.get("SS_BENCH_SEG", "320,960").split(",")]
    for seg_ms, N in [(s, n) for s in segs for n in Ns]:
        args = agent_args(seg_ms)
        audio_s, steps = schedule(N, seg_ms)
        pool = SpeechSessionPool(m, N, MAX_ROWS, vocoder=voc)
        sids = [pool.open("s2st", args) for _ in range(N)]
        agents = [StreamSpeechS2STAgent(args, model=StreamSpeechModel.from_engine(m.new_context()), vocoder=_Voc(voc.new_context()))
                  for _ in range(N)]
        run_pool(pool, sids, steps)                # warm-up: every shape once (each pass runs every utterance to its end)
        run_rr(agents, steps)
        tp, tr = [], []
        reps = int(os.environ.get("SS_BENCH_REPS", "3" if N <= 8 else "1"))
        for _ in range(reps):                      # alternate pooled and round-robin
            t0 = time.perf_counter(); run_pool(pool, sids, steps); tp.append(time.perf_counter() - t0)
            t0 = time.perf_counter(); run_rr(agents, steps); tr.append(time.perf_counter() - t0)
        st = []
        run_pool(pool, sids, steps, st)
        p, r = statistics.median(tp), statistics.median(tr)
        n = len(steps)
        mean = lambda k: float(np.mean([x.get(k, 0.0) for x in st]))    # noqa: E731  (write-side keys: steps with speech writers)
        rec = {"segment_ms": seg_ms, "N": N, "steps": n, "session_steps": sum(len(x) for x in steps), "audio_s": round(audio_s, 2),
               "pool_ms_per_step": round(1e3 * p / n, 3),
               "pool_frontend_ms_per_step": round(1e3 * mean("frontend_s"), 3),
               "pool_encoder_ctc_ms_per_step": round(1e3 * mean("encoder_ctc_s"), 3),
               "pool_mt_ms_per_step": round(1e3 * mean("mt_s"), 3),
               "pool_units_ms_per_step": round(1e3 * (mean("mt_features_s") + mean("units_s")), 3),
               "pool_vocoder_ms_per_step": round(1e3 * mean("vocoder_s"), 3),
               "writers_per_step": round(mean("writers"), 2), "max_writers": int(max(x["writers"] for x in st)),
               "speech_writers_per_step": round(mean("speech_writers"), 2),
               "mt_lockstep_steps_mean": round(mean("mt_steps"), 2), "mt_lockstep_steps_max": int(max(x["mt_steps"] for x in st)),
               "pool_audio_s_per_s": round(audio_s / p, 1),
               "round_robin_ms_per_step": round(1e3 * r / n, 3), "round_robin_audio_s_per_s": round(audio_s / r, 1),
               "speedup": round(r / p, 2), "timed_reps": reps}
        print(json.dumps(rec), flush=True)
        res["runs"].append(rec)
        del pool, agents
        torch.cuda.empty_cache()
    os.makedirs("profiles", exist_ok=True)
    with open(os.environ.get("SS_BENCH_OUT", os.path.join("profiles", "pooled_speech.json")), "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
