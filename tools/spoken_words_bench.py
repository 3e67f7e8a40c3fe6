"""What spoken words cost a pool step.  1 / 16 / 64 S2ST sessions of the synthetic checkpoint are fed 16-kHz audio in 320-ms chunks
for four seconds; two pools per size hold the same sessions over the same audio, stepped in ALTERNATING passes (off, on, off, on,
...) in one process so that clock and thermal drift fall on both:
  off   SpeechSessionPool(...)                the write side as it is
  on    SpeechSessionPool(..., spoken=True)   the unit pass keeps its device arg-max ids, and ONE ss_batch_unit_spans call (one
                                              upload, one launch, one download) follows each vocoder tail call, plus the host's
                                              spoken_from_segments for every writer
Only steps in which a session writes can differ, so both are reported per side and size: the median wall time of ALL steps and of the
WRITING steps (synchronised before and after) in each pass, the median over passes, and the run-to-run spread (lowest and highest
pass median).  A ratio on / off is only meaningful beside that spread.  The on side also reports its span calls, tail calls and the
seconds spent in the span calls (host and device, synchronised by the call's download).

  python tools/spoken_words_bench.py --out profiles/spoken_words.json      SS_BENCH_PASSES passes per side (default 5)"""
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
    a = p.parse_args(["--model-path", "synthetic:0", "--data-bin", "/nonexistent", "--vocoder", "synthetic:0", "--dur-prediction",
                      "--sample-rate", str(sr)])
    a.source_segment_size = seg_ms
    return a


def _one_pass(pool, sids, pcm):
    """One utterance through every session of the pool -> per step (wall seconds, writers, span calls, tail calls, spans seconds)."""
    import torch
    from streamspeech_amd.simuleval_shim import SpeechSegment
    per, rows = SR * CHUNK_MS // 1000, []
    for sid in sids:                                       # a fresh utterance, also where the last one ended without a final write
        pool.reset(sid)
    n_steps = -(-len(pcm[0]) // per)
    for st in range(n_steps):
        segs = {sid: SpeechSegment(content=pcm[i][st * per:(st + 1) * per].tolist(), sample_rate=SR, finished=st == n_steps - 1)
                for i, sid in enumerate(sids)}
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        pool.step(segs)
        torch.cuda.synchronize()
        ls = pool.last_step
        rows.append((time.perf_counter() - t0, int(ls.get("speech_writers", 0)), int(ls.get("span_calls", 0)),
                     int(ls.get("vocoder_tail_calls", 0)), float(ls.get("spans_s", 0.0))))
    return rows


def measure(out_path):
    import torch
    from streamspeech_amd import synth
    from streamspeech_amd.agent import StreamSpeechS2STAgent, load_dictionaries
    from streamspeech_amd.config import ModelConfig, VocoderConfig
    from streamspeech_amd.engine import HipModel, HipVocoder
    from streamspeech_amd.speech_pool import SpeechSessionPool
    if not torch.cuda.is_available():
        raise SystemExit("spoken_words_bench measures on the GPU; a CPU run provides no timing")
    cfg, vcfg = ModelConfig(), VocoderConfig()
    m = HipModel(synth.make_model_state_dict(0, cfg), cfg)
    voc = HipVocoder(synth.make_vocoder_state_dict(0, vcfg), vcfg)
    args = _args_of(StreamSpeechS2STAgent, SR, CHUNK_MS)
    dicts = load_dictionaries(args, cfg)
    passes = int(os.environ.get("SS_BENCH_PASSES", "5"))
    runs = []
    for n in SIZES:
        pcm = [synth.synth_pcm(9000 + i, SR * TOTAL_MS // 1000) for i in range(n)]
        pools = {"off": SpeechSessionPool(m, n, MAX_ROWS, vocoder=voc), "on": SpeechSessionPool(m, n, MAX_ROWS, vocoder=voc, spoken=True)}
        sids = {side: [p.open("s2st", args, dicts=dicts) for _ in range(n)] for side, p in pools.items()}
        for side in ("on", "off"):                         # warm-up: scratch growth, first launches
            _one_pass(pools[side], sids[side], pcm)
        med = {side: {"all": [], "writing": []} for side in pools}
        counts = {"span_calls": 0, "vocoder_tail_calls": 0, "spans_ms": 0.0, "writing_steps": 0, "writers": 0}
        for _ in range(passes):
            for side in ("off", "on"):
                rows = _one_pass(pools[side], sids[side], pcm)
                med[side]["all"].append(1e3 * statistics.median(r[0] for r in rows))
                wr = [r[0] for r in rows if r[1] > 0]
                if wr:
                    med[side]["writing"].append(1e3 * statistics.median(wr))
                if side == "on":
                    counts["span_calls"] += sum(r[2] for r in rows)
                    counts["vocoder_tail_calls"] += sum(r[3] for r in rows)
                    counts["spans_ms"] += 1e3 * sum(r[4] for r in rows)
                    counts["writing_steps"] += len(wr)
                    counts["writers"] += sum(r[1] for r in rows)
        words = sum(len(pools["on"].spoken(sid).words) for sid in sids["on"] if pools["on"].spoken(sid) is not None)
        row = {"sessions": n, "steps_per_pass": -(-len(pcm[0]) // (SR * CHUNK_MS // 1000)), "passes_per_side": passes,
               "spoken_words_at_end": words, "on_counts": {k: (round(v, 4) if isinstance(v, float) else v) for k, v in counts.items()}}
        if counts["span_calls"]:
            row["on_counts"]["ms_per_span_call"] = round(counts["spans_ms"] / counts["span_calls"], 4)
        for side in ("off", "on"):
            row[side] = {}
            for kind in ("all", "writing"):
                v = med[side][kind]
                if v:
                    row[side][kind] = {"step_ms_median": round(statistics.median(v), 4), "step_ms_pass_min": round(min(v), 4),
                                       "step_ms_pass_max": round(max(v), 4), "pass_medians_ms": [round(x, 4) for x in v]}
        for kind in ("all", "writing"):
            if kind in row["on"] and kind in row["off"]:
                row[f"ratio_on_over_off_{kind}"] = round(row["on"][kind]["step_ms_median"] / row["off"][kind]["step_ms_median"], 4)
                for side in ("off", "on"):
                    row[f"spread_{side}_{kind}"] = round(row[side][kind]["step_ms_pass_max"] / row[side][kind]["step_ms_pass_min"], 4)
        runs.append(row)
        print(json.dumps(row), flush=True)
        for side, p in pools.items():
            for sid in sids[side]:
                p.close(sid)
    res = {"tool": "tools/spoken_words_bench.py", "device": torch.cuda.get_device_name(0), "chunk_ms": CHUNK_MS, "audio_ms": TOTAL_MS,
           "kind": "s2st", "order": "alternating passes: off, on, off, on, ...", "runs": runs}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    measure(ap.parse_args().out)
