"""What scoring a given translation costs.  Two measurements on the synthetic checkpoint, each with its two sides in ALTERNATING
passes (a, b, a, b, ...) so that clock and thermal drift fall on both; per side the median over passes and the lowest and highest
pass are kept -- a ratio is only meaningful beside that spread.

  pack     128 synthetic utterances (1 .. 4 s), one seeded 30-token text each: HipModel.batch_mt_score against
           HipModel.batch_mt_features (n_tail_pad 0) on the same rows -- the pass the score rides on, whose launches are the parent's
           when no score is asked for.  Wall time of the whole call, synchronised before and after (the score call includes its one
           device-to-host copy).  In a run of its own the library's launch census brackets every GEMM launch with events: the GEMM
           time of the score call minus that of the features call is the vocabulary projection (and the launch difference its chunks);
           the token score kernel is timed alone on the same number of rows x V through ss_op_mt_token_scores.
  kernel   ss_op_mt_token_scores on 7680 x 6000 logits against ss_log_softmax on the same buffer (which also writes 7680 x 6000
           log-probabilities): device events around `reps` back-to-back launches.

  python tools/mt_score_bench.py --out profiles/mt_score.json        SS_BENCH_PASSES passes per side (default 7)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

N_UTT, N_TOK, KERNEL_ROWS, KERNEL_V = 128, 30, 7680, 6000


def _side(vals):
    return {"ms_median": round(statistics.median(vals), 4), "ms_min": round(min(vals), 4), "ms_max": round(max(vals), 4),
            "passes_ms": [round(v, 4) for v in vals]}


def _wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _events_ms(fn, reps):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _gemm_census(lib, fn):
    """fn() with every GEMM class bracketed by events -> (ms, launches) summed over the classes."""
    import torch
    lib.ss_prof_reset()
    lib.ss_prof_enable(-1)
    lib.ss_prof_enable_hi(-1)
    fn()
    torch.cuda.synchronize()
    ms_total, launches = 0.0, 0
    for cls in range(lib.ss_prof_num_classes()):
        ms, fl, n, by = C.c_double(0), C.c_double(0), C.c_int64(0), C.c_double(0)
        if lib.ss_prof_read(cls, C.byref(ms), C.byref(fl), C.byref(n), C.byref(by)) == 0:
            ms_total += ms.value
            launches += n.value
    lib.ss_prof_enable(0)
    lib.ss_prof_enable_hi(0)
    lib.ss_prof_reset()
    return ms_total, launches


def measure(out_path):
    import torch
    from streamspeech_amd import lib as L
    from streamspeech_amd import synth, workload
    from streamspeech_amd.config import ModelConfig
    from streamspeech_amd.engine import HipModel
    if not torch.cuda.is_available():
        raise SystemExit("mt_score_bench measures on the GPU; a CPU run provides no timing")
    lib = L.load()
    cfg = ModelConfig()
    m = HipModel(synth.make_model_state_dict(0, cfg), cfg)
    passes = int(os.environ.get("SS_BENCH_PASSES", "7"))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    # ---- pack ----
    utts = workload.make_utterances(N_UTT)
    pcm = torch.cat([torch.from_numpy(synth.synth_pcm(1234 + u.idx, u.n_samples)) for u in utts]).to(m.device)
    feat, T = m.batch_fbank_cmvn(pcm, [u.n_samples for u in utts])
    enc, Tp = m.batch_encoder_forward(feat, T)
    toks = [[int(t) for t in synth.uniform(700 + b, "mt_score_bench", (N_TOK,), 4, cfg.tgt_vocab)] for b in range(N_UTT)]
    rows = N_UTT * (N_TOK + 1)
    score = lambda: m.batch_mt_score(enc, Tp, toks)                            # noqa: E731
    feats = lambda: m.batch_mt_features(enc, Tp, toks, [0] * N_UTT)            # noqa: E731
    for _ in range(3):
        score(), feats()
    t = {"features": [], "score": []}
    for _ in range(passes):
        t["features"].append(_wall_ms(feats))
        t["score"].append(_wall_ms(score))
    g_feat, n_feat = _gemm_census(lib, feats)
    g_score, n_score = _gemm_census(lib, score)
    x = torch.randn(rows, cfg.tgt_vocab, device=m.device)
    tgt = torch.randint(0, cfg.tgt_vocab, (rows,), dtype=torch.int32, device=m.device)
    stat, idx = torch.empty(rows, 2, device=m.device), torch.empty(rows, 2, dtype=torch.int32, device=m.device)
    P = lambda a: C.c_void_p(a.data_ptr())                                     # noqa: E731
    k_pack = lambda: lib.ss_op_mt_token_scores(st, P(x), cfg.tgt_vocab, rows, cfg.tgt_vocab, P(tgt), P(stat), P(idx))   # noqa: E731
    assert k_pack() == 0
    pack = {"utterances": N_UTT, "tokens_per_text": N_TOK, "positions": rows, "encoder_rows": int(sum(Tp)), "passes_per_side": passes,
            "batch_mt_features": _side(t["features"]), "batch_mt_score": _side(t["score"]),
            "gemm_ms_features_call": round(g_feat, 4), "gemm_launches_features_call": n_feat,
            "gemm_ms_score_call": round(g_score, 4), "gemm_launches_score_call": n_score,
            "projection_ms": round(g_score - g_feat, 4), "projection_launches": n_score - n_feat,
            "score_kernel_ms_on_the_same_rows": round(_events_ms(k_pack, 20), 4)}
    pack["ratio_score_over_features"] = round(pack["batch_mt_score"]["ms_median"] / pack["batch_mt_features"]["ms_median"], 4)
    print(json.dumps(pack), flush=True)

    # ---- kernel ----
    x = torch.randn(KERNEL_ROWS, KERNEL_V, device=m.device)
    tgt = torch.randint(0, KERNEL_V, (KERNEL_ROWS,), dtype=torch.int32, device=m.device)
    stat = torch.empty(KERNEL_ROWS, 2, device=m.device)
    idx = torch.empty(KERNEL_ROWS, 2, dtype=torch.int32, device=m.device)
    out = torch.empty_like(x)
    k_score = lambda: lib.ss_op_mt_token_scores(st, P(x), KERNEL_V, KERNEL_ROWS, KERNEL_V, P(tgt), P(stat), P(idx))   # noqa: E731
    k_lsm = lambda: lib.ss_log_softmax(st, P(x), KERNEL_ROWS, KERNEL_V, -1, -1, 0, P(out))                            # noqa: E731
    assert k_score() == 0 and k_lsm() == 0
    for _ in range(5):
        k_score(), k_lsm()
    torch.cuda.synchronize()
    k = {"score": [], "log_softmax": []}
    for _ in range(passes):
        k["log_softmax"].append(_events_ms(k_lsm, 50))
        k["score"].append(_events_ms(k_score, 50))
    read_bytes = KERNEL_ROWS * KERNEL_V * 4
    kern = {"rows": KERNEL_ROWS, "V": KERNEL_V, "launches_per_pass": 50, "passes_per_side": passes,
            "mt_token_scores": _side(k["score"]), "log_softmax": _side(k["log_softmax"]),
            "logits_bytes": read_bytes,
            "mt_token_scores_read_GB_per_s": round(read_bytes / (statistics.median(k["score"]) * 1e-3) / 1e9, 1)}
    kern["ratio_score_over_log_softmax"] = round(kern["mt_token_scores"]["ms_median"] / kern["log_softmax"]["ms_median"], 4)
    print(json.dumps(kern), flush=True)
    res = {"tool": "tools/mt_score_bench.py", "device": torch.cuda.get_device_name(0), "order": "alternating passes: a, b, a, b, ...",
           "yardstick": "batch_mt_features of the same build on the same rows: without a score output its launches are the parent's",
           "pack": pack, "kernel": kern}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    measure(ap.parse_args().out)
