"""What the MT alignment costs a pool step.  1 / 16 / 64 S2TT sessions of the synthetic checkpoint are fed 16-kHz audio in 320-ms
chunks for four seconds; two sides per size, on the same audio, in ALTERNATING passes (off, on, off, on, ...) so that clock and
thermal drift fall on both:
  off   TextSessionPool(...)               the step as it always was
  on    TextSessionPool(..., align=True)   after the step's writes ONE batch_mt_attention (a ragged teacher-forced decoder pass over
                                           every writer's committed tokens, the attention kernel answering only the new positions,
                                           one device-to-host copy of peaks and statistics) plus the host's words_from_attention
Only steps in which a session writes pay anything, so per side and size the tool reports the wall time of a WHOLE pass (all steps,
each synchronised before and after) next to the median step: the median over passes and the run-to-run spread (lowest and highest
pass).  The ratio on / off is only meaningful beside that spread.

  python tools/mt_attention_bench.py --out profiles/mt_attention.json      SS_BENCH_PASSES passes per side (default 5)"""
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


def _one_pass(m, args, dicts, pcm, align):
    """All steps of one pool over the sessions' audio -> (wall seconds per step, attention calls, words answered at the end)."""
    import torch
    from streamspeech_amd.simuleval_shim import SpeechSegment
    from streamspeech_amd.text_pool import TextSessionPool
    n = len(pcm)
    pool = TextSessionPool(m, n, MAX_ROWS, align=True) if align else TextSessionPool(m, n, MAX_ROWS)
    sids = [pool.open("s2tt", args, dicts=dicts) for _ in range(n)]
    per, times, calls = SR * CHUNK_MS // 1000, [], 0
    n_steps = -(-len(pcm[0]) // per)
    for st in range(n_steps):
        segs = {sid: SpeechSegment(content=pcm[i][st * per:(st + 1) * per].tolist(), sample_rate=SR, finished=st == n_steps - 1)
                for i, sid in enumerate(sids)}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pool.step(segs)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        calls += pool.last_step["mt_attention"]
    words = sum(len(pool.alignment(sid) or []) for sid in sids) if align else 0
    return times, calls, words


def _kernel_us(n, rows=10, k_len=100, reps=50):
    """The attention probabilities kernel alone (ss_op_attention_probs, peaks only as the pools take it): n segments of `rows`
    answered rows over `k_len` keys, 8 heads -> microseconds per launch (device events around `reps` back-to-back launches)."""
    import ctypes as C
    import torch
    from streamspeech_amd import lib as L
    lib = L.load()
    dev = "cuda:0"
    Q = torch.randn(n * rows, 512, device=dev) * 0.125
    K = torch.randn(n * k_len, 512, device=dev)
    segs = torch.tensor([[s * rows, rows, s * k_len, k_len] for s in range(n)], dtype=torch.int32, device=dev).reshape(-1)
    qf = torch.zeros(n, dtype=torch.int32, device=dev)
    ro = torch.arange(n, dtype=torch.int32, device=dev) * rows
    peak = torch.empty(n * rows, dtype=torch.int32, device=dev)
    stat = torch.empty(n * rows, 2, device=dev)
    a = L.SSOpAttnProbsArgs()
    a.Q, a.K, a.ldq, a.ldk, a.H, a.scale = Q.data_ptr(), K.data_ptr(), 512, 512, 8, 1.0
    a.segs, a.nseg, a.q_first, a.row_off, a.p_off = segs.data_ptr(), n, qf.data_ptr(), ro.data_ptr(), None
    a.P, a.peak, a.stat, a.max_rows = None, peak.data_ptr(), stat.data_ptr(), rows
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for _ in range(5):
        assert lib.ss_op_attention_probs(st, C.byref(a)) == 0
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        lib.ss_op_attention_probs(st, C.byref(a))
    e1.record()
    torch.cuda.synchronize()
    return round(1e3 * e0.elapsed_time(e1) / reps, 3)


def measure(out_path):
    import torch
    from streamspeech_amd import synth
    from streamspeech_amd.agent import load_dictionaries
    from streamspeech_amd.agent_text import StreamSpeechS2TTAgent
    from streamspeech_amd.config import ModelConfig
    from streamspeech_amd.engine import HipModel
    if not torch.cuda.is_available():
        raise SystemExit("mt_attention_bench measures on the GPU; a CPU run provides no timing")
    cfg = ModelConfig()
    m = HipModel(synth.make_model_state_dict(0, cfg), cfg)
    args = _args_of(StreamSpeechS2TTAgent, SR, CHUNK_MS)
    dicts = load_dictionaries(args, cfg)
    passes = int(os.environ.get("SS_BENCH_PASSES", "5"))
    runs = []
    for n in SIZES:
        pcm = [synth.synth_pcm(9000 + i, SR * TOTAL_MS // 1000) for i in range(n)]
        _one_pass(m, args, dicts, pcm, True)               # warm-up: scratch growth, first launches
        _one_pass(m, args, dicts, pcm, False)
        med = {"off": [], "on": []}
        tot = {"off": [], "on": []}
        words = calls = 0
        for _ in range(passes):
            for side in ("off", "on"):
                t, c, w = _one_pass(m, args, dicts, pcm, side == "on")
                med[side].append(1e3 * statistics.median(t))
                tot[side].append(1e3 * sum(t))
                words, calls = max(words, w), max(calls, c)
        row = {"sessions": n, "steps_per_pass": -(-len(pcm[0]) // (SR * CHUNK_MS // 1000)), "passes_per_side": passes,
               "attention_calls_per_pass": calls, "words_at_end": words}
        for side in ("off", "on"):
            row[side] = {"pass_ms_median": round(statistics.median(tot[side]), 4), "pass_ms_min": round(min(tot[side]), 4),
                         "pass_ms_max": round(max(tot[side]), 4), "step_ms_median": round(statistics.median(med[side]), 4),
                         "pass_totals_ms": [round(v, 4) for v in tot[side]]}
        row["ratio_on_over_off"] = round(row["on"]["pass_ms_median"] / row["off"]["pass_ms_median"], 4)
        row["spread_off"] = round(row["off"]["pass_ms_max"] / row["off"]["pass_ms_min"], 4)
        row["spread_on"] = round(row["on"]["pass_ms_max"] / row["on"]["pass_ms_min"], 4)
        row["kernel_us_10_rows_x_100_keys_per_session"] = _kernel_us(n)
        if calls:
            row["ms_per_attention_call"] = round((row["on"]["pass_ms_median"] - row["off"]["pass_ms_median"]) / calls, 4)
        runs.append(row)
        print(json.dumps(row), flush=True)
    res = {"tool": "tools/mt_attention_bench.py", "device": torch.cuda.get_device_name(0), "chunk_ms": CHUNK_MS, "audio_ms": TOTAL_MS,
           "kind": "s2tt", "order": "alternating passes: off, on, off, on, ...", "runs": runs}
    if out_path:
        prev = {}
        if os.path.exists(out_path):                       # keep what other tools recorded in the same file (the fixture distances)
            with open(out_path) as f:
                prev = {k: v for k, v in json.load(f).items() if k not in res}
        res.update(prev)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    measure(ap.parse_args().out)
