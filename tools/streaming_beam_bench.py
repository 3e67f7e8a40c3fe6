"""Beam search behind a forced prefix (ss_batch_mt_beam_continue), one process, every shape warmed up first, host clock around
synchronising calls, the modes of a pair alternating, `--reps` repetitions (at least 20), median and spread (max - min) / median.
Writes profiles/streaming_beam.json and prints it as one JSON line.

  forced      B = 1 and 32, beam 4 and 10, total length 40: ss_batch_mt_beam_continue with a prefix of 0 / 10 / 30 tokens against
              ss_batch_mt_beam over the same total length at the same B and beam.  (The offline call of THIS build: its launches are
              the parent's)  The seed-0 model never ends early, so the unforced call runs 41 lock-step steps and the
              forced one 41 - n_prefix plus one ragged pass.  The prefix is the greedy search's own first tokens.
  agents      the S2TT agent's time per writing policy() call at --beam-mt 1 / 4 / 10 over the streaming utterances.
  pools       TextSessionPool step time at beam_mt = 1 / 4 with 16 sessions.

Kernel stats of the B = 32, beam 10, prefix 10 case alone:
    rocprofv3 --kernel-trace --stats --output-format csv -d profiles/streaming_beam_rocprof -o sb -- python tools/streaming_beam_bench.py --only-case 32,10,10
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from streamspeech_amd import synth, workload  # noqa: E402
from streamspeech_amd.config import ModelConfig  # noqa: E402
from streamspeech_amd.engine import HipModel  # noqa: E402

TOTAL = 40


def timed(f):
    torch.cuda.synchronize()
    t = time.perf_counter()
    f()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) * 1e3


def stats(v):
    med = statistics.median(v)
    return {"median_ms": round(med, 4), "spread": round((max(v) - min(v)) / med, 4), "n": len(v)}


def forced_pairs(m, reps, only=None):
    utts = sorted(workload.make_utterances(64), key=lambda u: u.seconds)[16:48]
    pcm = torch.cat([torch.from_numpy(synth.synth_pcm(1234 + u.idx, u.n_samples)) for u in utts]).cuda()
    feat, T = m.batch_fbank_cmvn(pcm, [u.n_samples for u in utts])
    enc_all, Tp_all = m.batch_encoder_forward(feat, T)
    free, _, _ = m.batch_mt_greedy(enc_all, Tp_all, [TOTAL] * len(Tp_all))
    out = []
    for B in (1, 32):
        Tp = Tp_all[:B]
        enc = enc_all[:sum(Tp)]
        mx = [TOTAL] * B
        for k in (4, 10):
            modes = {"unforced": lambda: m.batch_mt_beam(enc, Tp, mx, k)}
            for n in (0, 10, 30):
                pre = [[t for t in free[b] if t != m.cfg.eos][:n] for b in range(B)]
                modes[f"prefix{n}"] = (lambda pre=pre: m.batch_mt_beam_continue(enc, Tp, pre, mx, k))
            if only is not None:
                if (B, k) != only[:2]:
                    continue
                modes = {f"prefix{only[2]}": modes[f"prefix{only[2]}"]}
            for f in modes.values():
                f()
            times = {name: [] for name in modes}
            for _ in range(reps):
                for name, f in modes.items():
                    times[name].append(timed(f))
            rec = {"B": B, "beam": k, "total_len": TOTAL}
            rec.update({name: stats(v) for name, v in times.items()})
            out.append(rec)
    return out


def agent_writes(m, cfg, reps_utts=8):
    from streamspeech_amd.agent_text import StreamSpeechS2TTAgent
    from streamspeech_amd.modules import StreamSpeechModel
    from streamspeech_amd.simuleval_shim import SpeechSegment
    utts = sorted(workload.make_utterances(16), key=lambda u: u.seconds)[:reps_utts]
    out = {}
    for k in (1, 4, 10):
        ap = argparse.ArgumentParser()
        StreamSpeechS2TTAgent.add_args(ap)
        a = ap.parse_args(["--model-path", "synthetic:0", "--data-bin", "/nonexistent", "--sample-rate", "16000", "--beam-mt", str(k)])
        a.source_segment_size, a.device = 320, "gpu"
        agent = StreamSpeechS2TTAgent(a, model=StreamSpeechModel.from_engine(m.new_context()))
        writes = []
        for rnd in range(2):                     # the first pass over the utterances warms every shape up
            for u in utts:
                pcm = synth.synth_pcm(1234 + u.idx, min(u.n_samples, 16000 * 4))
                for pos in range(0, len(pcm), 5120):
                    seg = SpeechSegment(content=pcm[pos:pos + 5120].tolist(), sample_rate=16000, finished=pos + 5120 >= len(pcm))
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    o = agent.pushpop(seg)
                    torch.cuda.synchronize()
                    if rnd and not o.is_empty and not seg.finished:
                        writes.append((time.perf_counter() - t) * 1e3)
        out[f"beam{k}"] = stats(writes) if len(writes) > 1 else "not measured"
    return out


def pool_steps(m, cfg):
    from streamspeech_amd.agent import load_dictionaries
    from streamspeech_amd.agent_text import StreamSpeechS2TTAgent
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.text_pool import TextSessionPool
    utts = sorted(workload.make_utterances(32), key=lambda u: u.seconds)[:16]
    out = {}
    for k in (1, 4):
        steps = []
        for rnd in range(5):                     # the first round warms every shape up
            pool = TextSessionPool(m, 16, 256, beam_mt=k)
            ap = argparse.ArgumentParser()
            StreamSpeechS2TTAgent.add_args(ap)
            a = ap.parse_args(["--model-path", "synthetic:0", "--data-bin", "/nonexistent", "--sample-rate", "16000"])
            a.source_segment_size, a.device = 320, "gpu"
            d = load_dictionaries(a, cfg)
            pcms = [synth.synth_pcm(1234 + u.idx, min(u.n_samples, 16000 * 3)) for u in utts]
            sids = [pool.open("s2tt", a, dicts=d) for _ in pcms]
            n = min(len(p) for p in pcms) // 5120            # non-final steps only: every session still streaming
            for s in range(n):
                segs = {sid: SpeechSegment(content=p[s * 5120:(s + 1) * 5120].tolist(), sample_rate=16000, finished=False)
                        for sid, p in zip(sids, pcms)}
                ms = timed(lambda: pool.step(segs))
                if rnd:
                    steps.append(ms)
        out[f"beam_mt{k}"] = stats(steps) if len(steps) > 1 else "not measured"
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only-case", default="", help="B,beam,prefix: run that forced call alone (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "streaming_beam.json"))
    a = ap.parse_args()
    cfg = ModelConfig()
    g = np.load(os.path.join(ROOT, "tests", "golden", "gcmvn_fr-en.npz"))
    m = HipModel(synth.make_model_state_dict(0, cfg), cfg, cmvn_mean=g["mean"], cmvn_std=g["std"])
    if a.only_case:
        print(json.dumps({"forced": forced_pairs(m, max(a.reps, 3), tuple(int(x) for x in a.only_case.split(",")))}))
        return
    res = {"tool": "tools/streaming_beam_bench.py", "clock": "host clock around synchronising calls", "reps": max(a.reps, 20),
           "forced": forced_pairs(m, max(a.reps, 20)), "agent_write_call": agent_writes(m, cfg), "pool_step_16_sessions": pool_steps(m, cfg)}
    with open(a.out, "w", encoding="utf-8") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
