"""FP32 against the opt-in FP16 vocoder convs (ss_vocoder_set_f16) on the bench workload: packs of 128 utterances of
workload.make_utterances through workload.run_batch (the path bench.py times).

Reports, as one JSON object (--out, default profiles/vocoder_f16.json):
  * per kernel class: event-timed kernel ms, launches and algorithmic TFLOP/s of one vocoder pass over the pack, FP32 and FP16;
  * the vocoder pass alone (event-timed, median) and end-to-end offline S2ST x real time (audio seconds per wall second), switch
    off and on, as medians of alternating runs;
  * waveform RMS of the FP16 pack against the FP32 pack (worst and mean over the utterances), durations from the duration predictor
    compared between the two (the timed passes use the workload's forced durations, as bench.py does).
Kernel time is compared over the same launches on both sides: all classes of the pass, the ResBlock convs, and the f32 convs that
feed the wide stages (conv_pre and three up-convs: conv_sk2 in the f32 path, the pack-invariant LDS-tiled kernel while FP16 is on).
bench.py's own line stays the FP32 headline (FP16 is off by default)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5, help="alternating end-to-end runs per mode")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vocoder_f16.json"))
    a = ap.parse_args()

    import torch
    from streamspeech_amd import synth, workload
    from streamspeech_amd import lib as L
    from streamspeech_amd.config import ModelConfig, VocoderConfig
    from streamspeech_amd.engine import HipModel, HipVocoder
    from streamspeech_amd.pipeline import units_from_tokens

    cfg, vcfg = ModelConfig(), VocoderConfig()
    model = HipModel(synth.make_model_state_dict(0, cfg), cfg)
    v32 = HipVocoder(synth.make_vocoder_state_dict(0, vcfg), vcfg)
    v16 = v32.new_context()
    v16.set_fp16(True)
    lib = L.load()
    utts = workload.make_utterances(a.batch)
    pcm = torch.cat([torch.from_numpy(synth.synth_pcm(1234 + u.idx, u.n_samples)) for u in utts]).cuda()
    audio_s = sum(u.seconds for u in utts)

    # the pack's unit sequences, as run_batch hands them to the vocoder
    feat, T = model.batch_fbank_cmvn(pcm, [u.n_samples for u in utts])
    enc, Tp = model.batch_encoder_forward(feat, T)
    toks, feats, n = model.batch_mt_greedy(enc, Tp, [u.n_mt for u in utts])
    unit_toks = model.batch_t2u_units(feats, n)
    codes = [workload.resize_units(units_from_tokens(t, cfg), u.n_units, u.idx) for t, u in zip(unit_toks, utts)]
    forced = [u.durations for u in utts]

    def voc_pass(v):
        return v.batch_forward(codes, dur_prediction=True, forced_dur=forced)

    for v in (v32, v16, v32, v16):                  # warm-up (workspaces, FP16 fragments, LDS limits)
        voc_pass(v)
        workload.run_batch(model, v, pcm, utts)
    torch.cuda.synchronize()

    # accuracy, with the duration predictor (not the forced durations) so that the durations of the two paths are compared
    w32, d32, _ = v32.batch_forward(codes, dur_prediction=True)
    w16, d16, _ = v16.batch_forward(codes, dur_prediction=True)
    torch.cuda.synchronize()
    rms = [float(torch.sqrt(torch.mean((x.double() - y.double()) ** 2))) for x, y in zip(w16, w32)]
    same_dur = d16.cpu().tolist() == d32.cpu().tolist()

    # per-class kernel time of one vocoder pass
    ncls = lib.ss_prof_num_classes()
    names = [lib.ss_prof_class_name(c).decode() for c in range(ncls)]

    def classes(v):
        lib.ss_prof_reset()
        lib.ss_prof_enable(-1)
        lib.ss_prof_enable_hi((1 << max(0, ncls - 32)) - 1)
        voc_pass(v)
        torch.cuda.synchronize()
        out = {}
        for c in range(ncls):
            ms, fl, nl, by = C.c_double(), C.c_double(), C.c_int64(), C.c_double()
            lib.ss_prof_read(c, C.byref(ms), C.byref(fl), C.byref(nl), C.byref(by))
            if nl.value:
                out[names[c]] = {"launches": int(nl.value), "us": round(ms.value * 1e3, 1),
                                 "algo_tflops": round(fl.value / (ms.value * 1e-3) / 1e12, 1) if ms.value > 0 else None}
        lib.ss_prof_enable(0)
        lib.ss_prof_enable_hi(0)
        lib.ss_prof_reset()
        return out

    cls32, cls16 = classes(v32), classes(v16)

    # timing: vocoder pass alone (events) and end to end (wall), alternating
    def ev_time(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    voc_ms = {"f32": [], "f16": []}
    e2e_s = {"f32": [], "f16": []}
    for r in range(a.reps):
        order = (("f32", v32), ("f16", v16)) if r % 2 == 0 else (("f16", v16), ("f32", v32))
        for tag, v in order:
            voc_ms[tag].append(ev_time(lambda: voc_pass(v)))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            workload.run_batch(model, v, pcm, utts)
            torch.cuda.synchronize()
            e2e_s[tag].append(time.perf_counter() - t0)

    med = {k: statistics.median(x) for k, x in voc_ms.items()}
    rt = {k: audio_s / statistics.median(x) for k, x in e2e_s.items()}

    def us(cls, *prefixes):
        return sum(v["us"] for k, v in cls.items() if k.startswith(prefixes))

    def launches(cls, *prefixes):
        return sum(v["launches"] for k, v in cls.items() if k.startswith(prefixes))

    # The same launches on both sides.  ResBlock convs: the Winograd classes and the dilation-5 convs on conv_c64 in the f32 pass,
    # conv_f16 in the FP16 pass; the 64 -> 32 up-conv runs on conv_c64 in BOTH passes, so the f32 side's conv_c64 time less the FP16
    # side's conv_c64 time (that one launch, same shape and inputs) is the f32 ResBlock share of conv_c64.
    up64 = cls16.get("conv_c64<256,64>", {"us": 0.0, "launches": 0})
    rb32 = us(cls32, "conv_c64w", "conv_c128w", "conv_c256w") + us(cls32, "conv_c64<") - up64["us"]
    rb16 = us(cls16, "conv_f16")
    feed_cls = ("conv_sk2", "conv_gemm")
    assert launches(cls32, "conv_f16") == 0 and launches(cls16, "conv_c64w", "conv_c128w", "conv_c256w") == 0
    assert launches(cls32, *feed_cls) == launches(cls16, *feed_cls), "the feeding convs must be the same launches on both sides"
    res = {
        "workload": f"one pack of {a.batch} utterances of workload.make_utterances ({audio_s:.1f} s of audio), workload.run_batch; "
                    "synthetic seed-0 weights; timed passes with the workload's forced durations, the accuracy pass with predicted ones",
        "waveform_rms_vs_f32": {"worst": max(rms), "mean": statistics.mean(rms), "bar": 1e-3},
        "durations_identical": same_dur,
        "durations_compared": sum(len(c) for c in codes),
        "vocoder_pass_ms_median": {k: round(v, 3) for k, v in med.items()},
        "vocoder_pass_speedup": round(med["f32"] / med["f16"], 3),
        "end_to_end_x_realtime_median": {k: round(v, 1) for k, v in rt.items()},
        "end_to_end_speedup": round(rt["f16"] / rt["f32"], 3),
        "runs": {"voc_ms": voc_ms, "e2e_s": e2e_s},
        "kernel_classes_f32": cls32,
        "kernel_classes_f16": cls16,
        "kernel_us_all_classes": {"f32": round(us(cls32, ""), 1), "f16": round(us(cls16, ""), 1)},
        "kernel_us_resblock_convs": {"f32": round(rb32, 1), "f16": round(rb16, 1), "speedup": round(rb32 / rb16, 3),
                                     "launches": {"f32": launches(cls32, "conv_c64w", "conv_c128w", "conv_c256w", "conv_c64<") - up64["launches"],
                                                  "f16": launches(cls16, "conv_f16")}},
        "kernel_us_feeding_f32_convs": {"f32": round(us(cls32, *feed_cls), 1), "f16": round(us(cls16, *feed_cls), 1),
                                        "launches": launches(cls32, *feed_cls),
                                        "note": "conv_pre + the up-convs into the 256/128/64 stages: conv_sk2 in the f32 path; the pack-"
                                                "invariant (CANON_SEQ) LDS-tiled kernel while FP16 is on"},
    }
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: res[k] for k in ("waveform_rms_vs_f32", "durations_identical", "vocoder_pass_ms_median", "vocoder_pass_speedup",
                                          "end_to_end_x_realtime_median", "end_to_end_speedup", "kernel_us_all_classes",
                                          "kernel_us_resblock_convs", "kernel_us_feeding_f32_convs")}))


if __name__ == "__main__":
    main()
