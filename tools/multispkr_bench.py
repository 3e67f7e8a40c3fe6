"""What the speaker term costs: one 128-utterance CVSS-C-shaped pack (workload.make_utterances: ~37 units and ~50 frames per
second of speech, the workload's forced durations) through HipVocoder.batch_forward on a single-speaker vocoder and on a multi-speaker
one of the same seed -- one voice for all rows, and the rows cycling through all voices.  5 warm-ups of every variant, then 20 timed
repeats each, alternating; every repeat is event-timed around the whole call (which synchronises once inside).  The one launch the
speaker path adds (launch_spkr_pre_add over frames x C0 floats) is timed on its own on the pack's shape as well.

Writes medians and spreads to profiles/multispkr.json (--out).  Bar: the multi-speaker median is no slower than the single-speaker
median by more than the spread (max - min) of the single-speaker repeats plus the added pass."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--speakers", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "multispkr.json"))
    a = ap.parse_args()

    import torch
    from streamspeech_amd import lib as L
    from streamspeech_amd import synth, workload
    from streamspeech_amd.config import VocoderConfig
    from streamspeech_amd.engine import HipVocoder, _ptr, _stream

    scfg = VocoderConfig()
    mcfg = VocoderConfig(model_in_dim=2 * scfg.embedding_dim, multispkr=True, num_speakers=a.speakers)
    single = HipVocoder(synth.make_vocoder_state_dict(0, scfg), scfg)
    multi = HipVocoder(synth.make_vocoder_state_dict(0, mcfg), mcfg)
    utts = workload.make_utterances(a.batch)
    codes = [[int(u) for u in synth.uniform(7, f"multispkr_bench/{u.idx}", (u.n_units,), 0, scfg.num_embeddings)] for u in utts]
    forced = [u.durations for u in utts]
    frames = sum(sum(d) for d in forced)
    one_voice = [3 % a.speakers] * a.batch
    cycling = [b % a.speakers for b in range(a.batch)]
    variants = {
        "single_speaker": lambda: single.batch_forward(codes, dur_prediction=True, forced_dur=forced),
        "multi_one_voice": lambda: multi.batch_forward(codes, dur_prediction=True, forced_dur=forced, speakers=one_voice),
        "multi_cycling_voices": lambda: multi.batch_forward(codes, dur_prediction=True, forced_dur=forced, speakers=cycling),
    }

    def ev_time(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(a.warmup):
        for fn in variants.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    names = list(variants)
    for r in range(a.reps):
        for k in names[r % 3:] + names[:r % 3]:             # alternating, the order rotating
            ms[k].append(ev_time(variants[k]))

    # the added launch alone, on the pack's shape (the first up-conv reads a pre-activated input at 512 channels)
    lib, C0 = L.load(), mcfg.upsample_initial_channel
    Fr = [sum(d) for d in forced]
    start = [sum(Fr[:b]) for b in range(a.batch)]
    segs = torch.tensor([[s, n, s, n] for s, n in zip(start, Fr)], dtype=torch.int32, device="cuda")
    spk = torch.tensor(cycling, dtype=torch.int32, device="cuda")
    x, y = torch.randn((frames, C0), device="cuda"), torch.empty((frames, C0), device="cuda")
    names_, offs, numels, blob = multi._packed
    i = names_.index("voc.spkr.table")
    table = blob[offs[i]:offs[i] + numels[i]]

    def add_pass():
        L.check(lib.ss_op_spkr_pre_add(_stream(), _ptr(x), _ptr(y), C0, C0, _ptr(table), _ptr(spk), 0, _ptr(segs), a.batch, max(Fr),
                                       frames, 1, 0.1), "ss_op_spkr_pre_add")

    for _ in range(a.warmup):
        add_pass()
    add_ms = [ev_time(add_pass) for _ in range(a.reps)]

    def stats(v):
        q = statistics.quantiles(v, n=4)
        return {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                "iqr_ms": round(q[2] - q[0], 4)}

    st = {k: stats(v) for k, v in ms.items()}
    add = stats(add_ms)
    spread = st["single_speaker"]["max_ms"] - st["single_speaker"]["min_ms"]
    allowed = spread + add["median_ms"]
    res = {
        "workload": f"one pack of {a.batch} utterances of workload.make_utterances ({sum(u.seconds for u in utts):.1f} s of speech, "
                    f"{sum(len(c) for c in codes)} units, {frames} frames), HipVocoder.batch_forward with the workload's forced "
                    f"durations; synthetic seed-0 weights, {a.speakers} speakers; {a.warmup} warm-ups, {a.reps} alternating repeats",
        "batch_forward": st,
        "added_pass_alone": {**add, "bytes": 2 * frames * C0 * 4,
                             "gbytes_per_s": round(2 * frames * C0 * 4 / (add["median_ms"] * 1e-3) / 1e9, 1)},
        "speaker_table_bytes": int(numels[i]) * 4,
        "single_speaker_spread_ms": round(spread, 4),
        "slower_than_single_ms": {k: round(st[k]["median_ms"] - st["single_speaker"]["median_ms"], 4)
                                  for k in ("multi_one_voice", "multi_cycling_voices")},
        "allowed_ms": round(allowed, 4),
        "within_bar": all(st[k]["median_ms"] - st["single_speaker"]["median_ms"] <= allowed
                          for k in ("multi_one_voice", "multi_cycling_voices")),
        "within_iqr_plus_pass": all(st[k]["median_ms"] - st["single_speaker"]["median_ms"]
                                    <= st["single_speaker"]["iqr_ms"] + add["median_ms"]
                                    for k in ("multi_one_voice", "multi_cycling_voices")),
        "runs_ms": {k: [round(x_, 4) for x_ in v] for k, v in ms.items()},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: v for k, v in res.items() if k != "runs_ms"}))


if __name__ == "__main__":
    main()
