"""What an n-gram model costs inside the CTC prefix beam search, and that the plain search costs what it did.  One 128-utterance pack
of the bench workload goes through the encoder once; then, on one text head and the same packed encoder output, per setting beam /
cand = 4/8, 8/16, 32/32 in ALTERNATING passes (plain, lm3, lm5, parent, plain, ...) so that clock and thermal drift fall on all sides:
  plain   batch_ctc_beam(head, enc, Tp, beam, cand)                         this tree
  lm3     batch_ctc_beam(..., lm=order-3 model of about 10^6 entries, lm_weight 0.5)
  lm5     batch_ctc_beam(..., lm=order-5 model of about 10^6 entries, lm_weight 0.5)
  parent  batch_ctc_beam(head, enc, Tp, beam, cand)                         the parent build (--parent-lib), in a child process that
                                                                            stays up for the whole run and measures a pass when told to
Each call is timed on the host, synchronised before and after (head GEMM, table fill, both kernels, the device-to-host copy and the
host unpacking).  Per side: the median call in each pass, the median over passes and the run-to-run spread (highest / lowest pass
median).  Reported: lm3 / plain and lm5 / plain per setting, and plain / parent beside the parent's own spread -- the plain search's
code path is meant to be untouched, so that ratio has to lie inside the spread (`plain_inside_parent_spread`).

The two kernels apart: ss_op_ctc_beam / ss_op_ctc_beam_lm on the head's own logits between two events (fill + both kernels), and the
plain call with every frame row declared an utterance of its own as the candidate kernel's estimate; a search kernel ~ the
difference.  Estimates from differences of medians, not a kernel trace.

The synthetic models are seeded random tables over the head's vocabulary (values in [-7, -0.2], back-off weights in [-2, 0]): the
cost of a lookup depends on the table's size and on how often a context backs off, not on the values.

  python tools/ctc_lm_bench.py --out profiles/ctc_lm.json [--parent-lib PARENT.so]     SS_BENCH_PASSES passes per side (default 7)"""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PACK, CALLS, HEAD = 128, 5, 0
SETTINGS = ((4, 8), (8, 16), (32, 32))
NEW_SYMBOLS = ("ss_ngram_lm_create", "ss_ngram_lm_destroy", "ss_ngram_lm_info", "ss_ngram_score_host", "ss_op_ngram_score",
               "ss_ctc_beam_lm_host", "ss_op_ctc_beam_lm", "ss_batch_ctc_beam_lm")


def synthetic_lm(V, order, per_order, seed):
    """The arrays of a seeded model: a unigram for <s> and for every id the head can emit (</s> among them), and per_order unique
    n-grams of each higher order, every one the extension of an n-gram of the order below."""
    import numpy as np
    rng = np.random.default_rng(seed)
    grams = [np.asarray([0] + [i for i in range(2, V) if i != 3], np.int64).reshape(-1, 1)]
    for k in range(2, order + 1):
        ctx = grams[-1][rng.integers(0, len(grams[-1]), int(per_order * 1.2))]
        ctx = ctx[ctx[:, -1] != 2]                               # nothing follows </s>
        g = np.unique(np.concatenate([ctx, rng.integers(4, V, (len(ctx), 1))], axis=1), axis=0)
        grams.append(g[rng.permutation(len(g))[:per_order]])
    n = sum(len(g) for g in grams)
    return {"order": order, "counts": [len(g) for g in grams], "tokens": np.concatenate([g.reshape(-1) for g in grams]).astype(np.int32),
            "logp": rng.uniform(-7.0, -0.2, n).astype(np.float32),
            "backoff": np.concatenate([rng.uniform(-2.0, 0.0, len(g)) if k < order else np.zeros(len(g)) for k, g in enumerate(grams, 1)])
            .astype(np.float32), "V": V, "bos": 0, "eos": 2, "unk": 3, "oov_logp": -20.0}


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _side(vals):
    return {"call_ms_median": round(statistics.median(vals), 4), "call_ms_pass_min": round(min(vals), 4),
            "call_ms_pass_max": round(max(vals), 4), "spread": round(max(vals) / min(vals), 4), "pass_medians_ms": [round(v, 4) for v in vals]}


def _setup():
    import torch
    from streamspeech_amd import synth, workload
    from streamspeech_amd.config import ModelConfig
    from streamspeech_amd.engine import HipModel
    if not torch.cuda.is_available():
        raise SystemExit("ctc_lm_bench measures on the GPU; a CPU run provides no timing")
    cfg = ModelConfig()
    m = HipModel(synth.make_model_state_dict(0, cfg), cfg)
    utts = workload.make_utterances(PACK)
    pcm = torch.cat([torch.from_numpy(synth.synth_pcm(1234 + u.idx, u.n_samples)) for u in utts]).to(m.device)
    feat, T = m.batch_fbank_cmvn(pcm, [u.n_samples for u in utts])
    enc, Tp = m.batch_encoder_forward(feat, T)
    return m, enc, [int(t) for t in Tp]


def child():
    """The parent build's side: `pass <beam> <cand>` on stdin -> the pass median in ms on stdout; `quit` ends."""
    from streamspeech_amd import lib as L
    for name in NEW_SYMBOLS:                                     # the parent build has none of them
        L.SIGNATURES.pop(name, None)
    m, enc, Tp = _setup()
    print("ready", flush=True)
    for line in sys.stdin:
        f = line.split()
        if not f or f[0] == "quit":
            break
        beam, cand = int(f[1]), int(f[2])
        if f[0] == "warm":
            m.batch_ctc_beam(HEAD, enc, Tp, beam, cand)
            print("ok", flush=True)
        else:
            print(statistics.median(_timed(lambda: m.batch_ctc_beam(HEAD, enc, Tp, beam, cand)) for _ in range(CALLS)), flush=True)


def _kernels_ms(model, logits, T, beam, cand, passes, lm=None):
    """The table fill and the two kernels on `logits` between two events: the median over `passes` launches, in ms."""
    import torch
    from streamspeech_amd.lib import SSCtcLmOpts
    B, V = len(T), logits.shape[1]
    stride = max(T)
    hyp = torch.empty((8 * B * beam,), dtype=torch.int32, device=logits.device)
    tok = torch.empty((B * beam * stride,), dtype=torch.int32, device=logits.device)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    hT = (C.c_int32 * B)(*T)
    opts = SSCtcLmOpts(0.5, 0.0, 1)
    ms = []
    for _ in range(passes + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        a.record()
        if lm is None:
            rc = model.lib.ss_op_ctc_beam(s, P(logits), V, V, model.cfg.pad, model.cfg.unk, B, hT, beam, cand, beam, P(hyp), P(tok), stride,
                                          None, None)
        else:
            rc = model.lib.ss_op_ctc_beam_lm(s, P(logits), V, V, model.cfg.pad, model.cfg.unk, B, hT, beam, cand, beam, P(hyp), P(tok),
                                             stride, None, None, lm.h, C.byref(opts))
        b.record()
        assert rc == 0, rc
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms[1:])                       # the first launch sizes the op's scratch


def measure(out_path, parent_lib):
    import torch
    from streamspeech_amd.ngram import NgramLM
    m, enc, Tp = _setup()
    V = m.cfg.src_vocab if HEAD == 0 else m.cfg.tgt_vocab
    passes = int(os.environ.get("SS_BENCH_PASSES", "7"))
    t0 = time.perf_counter()
    lms = {"lm3": NgramLM(synthetic_lm(V, 3, 500000, 1)), "lm5": NgramLM(synthetic_lm(V, 5, 250000, 2))}
    build_s = time.perf_counter() - t0
    par = None
    if parent_lib:
        par = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                               text=True, env=dict(os.environ, SS_HIP_LIB=os.path.abspath(parent_lib)))
        assert par.stdout.readline().strip() == "ready", "the parent build's process did not come up"

    def ask(cmd):
        par.stdin.write(cmd + "\n")
        par.stdin.flush()
        return par.stdout.readline().strip()
    rows = []
    try:
        for beam, cand in SETTINGS:
            sides = {"plain": lambda: m.batch_ctc_beam(HEAD, enc, Tp, beam, cand)}
            for k, lm in lms.items():
                sides[k] = lambda lm=lm: m.batch_ctc_beam(HEAD, enc, Tp, beam, cand, lm=lm, lm_weight=0.5)
            got = {k: fn() for k, fn in sides.items()}               # warm-up: scratch growth, first launches, the models' upload
            if par:
                assert ask(f"warm {beam} {cand}") == "ok"
            med = {k: [] for k in list(sides) + (["parent"] if par else [])}
            for _ in range(passes):
                for k, fn in sides.items():
                    med[k].append(statistics.median(_timed(fn) for _ in range(CALLS)))
                if par:
                    med["parent"].append(float(ask(f"pass {beam} {cand}")))
            m.batch_ctc_beam(HEAD, enc, Tp, beam, cand)
            logits = m.last_logits()
            kern = {"plain": _kernels_ms(m, logits, Tp, beam, cand, passes)}
            for k, lm in lms.items():
                kern[k] = _kernels_ms(m, logits, Tp, beam, cand, passes, lm)
            frame = _kernels_ms(m, logits, [1] * sum(Tp), beam, cand, passes)
            row = {"head": HEAD, "beam": beam, "cand": cand, "nbest": beam, "utterances": PACK, "frames": sum(Tp), "longest_frames": max(Tp),
                   "passes_per_side": passes, "calls_per_pass": CALLS, **{k: _side(v) for k, v in med.items()}}
            for k in lms:
                row[f"ratio_{k}_over_plain"] = round(row[k]["call_ms_median"] / row["plain"]["call_ms_median"], 4)
                row[f"best_differs_from_plain_in_{k}"] = sum(a[0].tokens != b[0].tokens for a, b in zip(got[k], got["plain"]))
            if par:
                r = row["plain"]["call_ms_median"] / row["parent"]["call_ms_median"]
                row["ratio_plain_over_parent"] = round(r, 4)
                row["plain_inside_parent_spread"] = bool(1.0 / row["parent"]["spread"] <= r <= row["parent"]["spread"])
            row["where_the_time_goes_ms"] = {
                "candidate_kernel_estimate": round(frame, 4),
                **{f"fill_and_both_kernels_{k}": round(v, 4) for k, v in kern.items()},
                **{f"search_kernel_estimate_{k}": round(v - frame, 4) for k, v in kern.items()},
                **{f"search_kernel_{k}_over_plain": round((kern[k] - frame) / (kern["plain"] - frame), 4) for k in lms}}
            rows.append(row)
            print(json.dumps(row), flush=True)
    finally:
        if par:
            par.stdin.write("quit\n")
            par.stdin.flush()
            par.wait(timeout=60)
    res = {"tool": "tools/ctc_lm_bench.py", "device": torch.cuda.get_device_name(0),
           "order": "alternating passes: plain, lm3, lm5, parent, plain, ...", "lm_weight": 0.5, "word_score": 0.0, "eos_term": True,
           "models": {k: {"order": lm.order, "entries": lm.entries, "slots": lm.slots, "device_bytes": lm.device_bytes} for k, lm in lms.items()},
           "models_host_build_s": round(build_s, 2), "parent_lib": bool(parent_lib), "settings": rows}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="libstreamspeech_hip.so of the parent commit: its plain search is timed beside this tree's")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child()
    else:
        measure(a.out, a.parent_lib)
