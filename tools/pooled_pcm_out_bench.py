"""Speech out of the session pool at the caller's rate and format (PcmOut) against the "s16le" string route and against what a caller
does today on the host.  64 S2ST sessions of the synthetic checkpoint on the schedule of tools/pooled_pcm_bench.py (960-ms segments,
utterances of up to 8 s, eight staggered starts), fed the same s16le bytes on every route; the routes differ in pcm_out only:
  string          pcm_out="s16le": one ss_pcm_pack_s16 launch and one download per writing step
  s16le@16000     PcmOut("s16le", 16000): the same work through ss_pcm_emit (no filter, no state)
  ulaw@8000, s16le@48000, f32le@44100     one ratio and format each
  mix             the sessions cycle through the four PcmOut settings above
  host-today      the string route, then per session on the host scipy.signal.resample_poly to 8 kHz of the step's chunk and
                  audioop.lin2ulaw -- per chunk, WITHOUT the carried state a correct streaming resampler needs, so a lower bound of
                  the host work PcmOut("ulaw", 8000) replaces
Per route: wall time of the writing steps (synchronised before and after; median and p95 over all writing steps of all passes), the
pool's handover_s (from the vocoder tails in hand to the contents the segments carry), bytes out per pass, emit / pack calls per step.
The routes run one after the other in two rounds, so drift over the run shows as the difference between a route's two rounds.

  python tools/pooled_pcm_out_bench.py --out profiles/pooled_pcm_out.json      SS_BENCH_PASSES passes per round (default 4)"""
import argparse
import json
import os
import statistics
import sys
import time

N, SEG_MS, MAX_ROWS, MAX_SECONDS, SR = 64, 960, 384, 8, 16000
SETTINGS = (("s16le", 16000), ("ulaw", 8000), ("s16le", 48000), ("f32le", 44100))
ROUTES = ("string", "s16le@16000", "ulaw@8000", "s16le@48000", "f32le@44100", "mix", "host-today")


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


def _p95(v):
    s = sorted(v)
    return s[min(len(s) - 1, int(0.95 * len(s)))]


def measure(out_path, n_sessions):
    import numpy as np
    import torch
    from streamspeech_amd import synth
    from streamspeech_amd.agent import StreamSpeechS2STAgent
    from streamspeech_amd.config import ModelConfig, VocoderConfig
    from streamspeech_amd.engine import HipModel, HipVocoder
    from streamspeech_amd.pcm import PcmFormat, PcmOut
    from streamspeech_amd.speech_pool import SpeechSessionPool
    from streamspeech_amd.workload import make_utterances
    if not torch.cuda.is_available():
        raise SystemExit("pooled_pcm_out_bench measures on the GPU; a CPU run provides no timing")
    import audioop
    from scipy.signal import resample_poly
    cfg, vcfg = ModelConfig(), VocoderConfig()
    m = HipModel(synth.make_model_state_dict(0, cfg), cfg)
    voc = HipVocoder(synth.make_vocoder_state_dict(0, vcfg), vcfg)
    passes = int(os.environ.get("SS_BENCH_PASSES", "4"))
    args = _args_of(StreamSpeechS2STAgent, SR, SEG_MS, ("--vocoder", "synthetic:0", "--dur-prediction"))
    utts = make_utterances(n_sessions, 1234)
    step = SR * SEG_MS // 1000
    segs = []
    for i, u in enumerate(utts):
        n = min(int(u.n_samples), MAX_SECONDS * SR)
        s = _s16(700 + i, n)
        segs.append([(s[p:p + step].tobytes(), p + step >= n) for p in range(0, n, step)])
    start = [i % 8 for i in range(n_sessions)]
    steps, k = [], 0
    while True:
        row = [(i, segs[i][k - start[i]]) for i in range(n_sessions) if 0 <= k - start[i] < len(segs[i])]
        if not row and k > max(start):
            break
        if row:
            steps.append(row)
        k += 1

    def pcm_out_of(route, i):
        if route in ("string", "host-today"):
            return "s16le"
        fmt, rate = SETTINGS[i % len(SETTINGS)] if route == "mix" else (route.split("@")[0], int(route.split("@")[1]))
        return PcmOut(fmt, rate)

    rounds = []
    for rnd in range(2):
        for route in ROUTES:
            pool = SpeechSessionPool(m, n_sessions, MAX_ROWS, vocoder=voc)
            sids = [pool.open("s2st", args, pcm_in=PcmFormat("s16le"), pcm_out=pcm_out_of(route, i)) for i in range(n_sessions)]
            t_write, hand, host_s, out_bytes, emit_calls, pack_calls = [], [], [], 0, 0, 0
            for p in range(passes + 1):                # pass 0 warms every shape up
                for sid in sids:
                    pool.reset(sid)
                for row in steps:
                    for i, (item, fin) in row:
                        pool.push_pcm(sids[i], item, finished=fin)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    out = pool.step()
                    th = time.perf_counter()
                    if route == "host-today":
                        for o in out.values():
                            if not o.is_empty and o.content:
                                x = np.frombuffer(o.content, "<i2").astype(np.float32) / 32768.0
                                y = np.clip(resample_poly(x, 1, 2), -1.0, 1.0)
                                o.content = audioop.lin2ulaw(np.round(y * 32767.0).astype("<i2").tobytes(), 2)
                    torch.cuda.synchronize()
                    t1 = time.perf_counter()
                    ls = pool.last_step
                    if p and ls.get("speech_writers"):
                        t_write.append(t1 - t0)
                        hand.append(ls["handover_s"])
                        host_s.append(t1 - th)
                        emit_calls, pack_calls = max(emit_calls, ls["pcm_emit_calls"]), max(pack_calls, ls["pcm_pack_calls"])
                    if p == 1:
                        out_bytes += sum(len(o.content) for o in out.values() if not o.is_empty)
            rec = {"route": route, "round": rnd, "sessions": n_sessions, "steps": len(steps), "writing_steps": len(t_write) // passes,
                   "step_ms_median": round(1e3 * statistics.median(t_write), 4), "step_ms_p95": round(1e3 * _p95(t_write), 4),
                   "handover_ms_median": round(1e3 * statistics.median(hand), 4), "handover_ms_p95": round(1e3 * _p95(hand), 4),
                   "bytes_out_per_pass": out_bytes, "pcm_emit_calls_per_step": emit_calls, "pcm_pack_calls_per_step": pack_calls}
            if route == "host-today":
                rec["host_resample_ulaw_ms_median"] = round(1e3 * statistics.median(host_s), 4)
            print(json.dumps(rec), flush=True)
            rounds.append(rec)
            del pool
            torch.cuda.empty_cache()
            os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
            with open(out_path, "w") as f:
                json.dump({"workload": " ".join(__doc__.split("\n\n")[0].split()), "device": torch.cuda.get_device_name(0),
                           "passes_per_round": passes, "runs": rounds}, f, indent=1)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "pooled_pcm_out.json"))
    ap.add_argument("--sessions", type=int, default=N)
    a = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    measure(a.out, a.sessions)
