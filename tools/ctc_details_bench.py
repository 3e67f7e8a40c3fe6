"""What word details cost a pool step.  1 / 16 / 64 ASR sessions of the synthetic checkpoint are fed 16-kHz audio in 320-ms chunks
for four seconds; two sides per size, on the same audio, in ALTERNATING passes (off, on, off, on, ...) so that clock and thermal
drift fall on both:
  off   TextSessionPool(...)                 the step's CTC call is ss_stream_pool_ctc
  on    TextSessionPool(..., details=True)   the scored call (one launch more per head, a D2H copy twice the size) plus the host's
                                             words_from_ctc for both heads of every session
Per side and size: the median wall time of a step (synchronised before and after) in each pass, the median over passes, and the
run-to-run spread (lowest and highest pass median).  The ratio on / off is only meaningful beside that spread.

  python tools/ctc_details_bench.py --out profiles/ctc_details.json      SS_BENCH_PASSES passes per side (default 5)"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZES, SR, CHUNK_MS, TOTAL_MS, MAX_ROWS = (1, 16, 64), 16000, 320, 4000, 128


def _args_of(cls, sr, seg_ms):
    p = argparse.ArgumentParser()
    cls.add_args(p)
    a = p.parse_args(["--model-path", "synthetic:0", "--data-bin", "/nonexistent", "--vocoder", "synthetic:0", "--sample-rate", str(sr)])
    a.source_segment_size = seg_ms
    return a


def _one_pass(m, args, dicts, pcm, details):
    """All steps of one pool over the sessions' audio -> (wall seconds per step, words answered at the end)."""
    import torch
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.text_pool import TextSessionPool
    n = len(pcm)
    pool = TextSessionPool(m, n, MAX_ROWS, details=True) if details else TextSessionPool(m, n, MAX_ROWS)
    sids = [pool.open("asr", args, dicts=dicts) for _ in range(n)]
    per, times = SR * CHUNK_MS // 1000, []
    n_steps = -(-len(pcm[0]) // per)
    for st in range(n_steps):
        segs = {sid: SpeechSegment(content=pcm[i][st * per:(st + 1) * per].tolist(), sample_rate=SR, finished=st == n_steps - 1)
                for i, sid in enumerate(sids)}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pool.step(segs)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    words = sum(len(pool.details(sid).source_words) for sid in sids) if details else 0
    return times, words


def measure(out_path):
    import torch
    from streamspeech_amd import synth
    from streamspeech_amd.agent import load_dictionaries
    from streamspeech_amd.agent_text import StreamSpeechASRAgent
    from streamspeech_amd.config import ModelConfig
    from streamspeech_amd.engine import HipModel
    if not torch.cuda.is_available():
        raise SystemExit("ctc_details_bench measures on the GPU; a CPU run provides no timing")
    cfg = ModelConfig()
    m = HipModel(synth.make_model_state_dict(0, cfg), cfg)
    args = _args_of(StreamSpeechASRAgent, SR, CHUNK_MS)
    dicts = load_dictionaries(args, cfg)
    passes = int(os.environ.get("SS_BENCH_PASSES", "5"))
    runs = []
    for n in SIZES:
        pcm = [synth.synth_pcm(9000 + i, SR * TOTAL_MS // 1000) for i in range(n)]
        _one_pass(m, args, dicts, pcm, True)               # warm-up: scratch growth, first launches
        _one_pass(m, args, dicts, pcm, False)
        med = {"off": [], "on": []}
        words = 0
        for _ in range(passes):
            for side in ("off", "on"):
                t, w = _one_pass(m, args, dicts, pcm, side == "on")
                med[side].append(1e3 * statistics.median(t))
                words = max(words, w)
        row = {"sessions": n, "steps_per_pass": -(-len(pcm[0]) // (SR * CHUNK_MS // 1000)), "passes_per_side": passes,
               "source_words_at_end": words}
        for side in ("off", "on"):
            row[side] = {"step_ms_median": round(statistics.median(med[side]), 4), "step_ms_pass_min": round(min(med[side]), 4),
                         "step_ms_pass_max": round(max(med[side]), 4), "pass_medians_ms": [round(v, 4) for v in med[side]]}
        row["ratio_on_over_off"] = round(row["on"]["step_ms_median"] / row["off"]["step_ms_median"], 4)
        row["spread_off"] = round(row["off"]["step_ms_pass_max"] / row["off"]["step_ms_pass_min"], 4)
        row["spread_on"] = round(row["on"]["step_ms_pass_max"] / row["on"]["step_ms_pass_min"], 4)
        runs.append(row)
        print(json.dumps(row), flush=True)
    res = {"tool": "tools/ctc_details_bench.py", "device": torch.cuda.get_device_name(0), "chunk_ms": CHUNK_MS, "audio_ms": TOTAL_MS,
           "kind": "asr", "order": "alternating passes: off, on, off, on, ...", "runs": runs}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    measure(ap.parse_args().out)
