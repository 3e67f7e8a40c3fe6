"""What lexical constraints cost the first-pass text search.  One 128-utterance pack of the bench workload goes through the encoder
once; then, on the same packed encoder output and with max_len = MAX_LEN for every utterance, at beam 4 and beam 10 in ALTERNATING
passes (plain, empty, glossary, plain, ...) so that clock and thermal drift fall on all three:
  plain     batch_mt_beam(enc, Tp, max_len, beam)                          ss_batch_mt_beam: the plain top-2k and merge kernels
  empty     the same call through ss_batch_mt_beam_cons with no phrase     the constrained kernels on C = 0: the price of the variant
  glossary  ss_batch_mt_beam_cons with 2 phrases (1 + 2 tokens) per utterance, drawn seeded from the ordinary tokens
A pack of 128 x beam rows runs as consecutive sub-calls of at most 256 rows (engine.plan_beam_groups), the same split on all three
sides.  Each call is timed on the host, synchronised before and after.  Per side: the median call in each pass, the median over
passes and the run-to-run spread (lowest and highest pass median); a ratio is only meaningful beside that spread.  The synthetic
model emits no early </s>, so every search runs its MAX_LEN + 1 steps on all three sides.

The kernels apart, between two events on R = 32 x beam rows of random scores at the model's vocabulary: ss_op_beam_topk (the plain
top-2k kernel; the constrained variant has no op entry of its own -- it adds two compares per vocabulary entry and at most two
stores per row to this kernel) and ss_op_beam_cons_select (the rank merge and the selection stage of the constrained merge
kernel).  The plain search launches beam_topk_kernel and beam_merge_kernel as before: the variants are chosen on the host, once
per search, and only ss_batch_mt_beam_cons chooses them.

  python tools/mt_constraints_bench.py --out profiles/mt_constraints.json      SS_BENCH_PASSES passes per side (default 5)"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PACK, CALLS, MAX_LEN = 128, 2, 32
BEAMS = (4, 10)


def _timed(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0)


def _side(vals):
    return {"call_ms_median": round(statistics.median(vals), 4), "call_ms_pass_min": round(min(vals), 4),
            "call_ms_pass_max": round(max(vals), 4), "pass_medians_ms": [round(v, 4) for v in vals]}


def _kernels_ms(model, beam, passes):
    """(plain top-2k kernel, selection kernel) on 32 utterances x beam rows, median of `passes` launches each, in ms."""
    import numpy as np
    import torch
    from streamspeech_amd.lib import MT_CONS_TABLE_LD, SS_OP_BEAM_CAND
    rng = np.random.default_rng(beam)
    B, V, k = 32, model.cfg.tgt_vocab, beam
    R = B * k
    dev = model.device
    logits = torch.from_numpy(rng.standard_normal((R, V)).astype(np.float32)).to(dev)
    zi = torch.zeros(B, dtype=torch.int32, device=dev)
    mxl = torch.full((B,), 100, dtype=torch.int32, device=dev)
    cum = torch.from_numpy((-rng.random(R) * 6).astype(np.float32)).to(dev)
    cand_s = torch.empty((R, SS_OP_BEAM_CAND), dtype=torch.float32, device=dev)
    cand_t = torch.empty((R, SS_OP_BEAM_CAND), dtype=torch.int32, device=dev)
    tab = np.zeros((B, MT_CONS_TABLE_LD), np.int32)
    tab[:, :3] = rng.integers(4, V, (B, 3))
    tab[:, 64:] = [3, 3, 0b101, 0]                                   # phrases of 1 + 2 tokens
    state = torch.from_numpy(rng.integers(-1, 3, R).astype(np.int32)).to(dev)
    nt = np.where(state.cpu().numpy() < 2, tab[np.arange(R) // k, np.clip(state.cpu().numpy() + 1, 0, 2)], -1)
    next_t = torch.from_numpy(np.stack([nt, np.full(R, -1)], 1).astype(np.int32)).to(dev)
    next_s = torch.from_numpy((-rng.random((R, 2)) * 9).astype(np.float32)).to(dev)
    d_tab = torch.from_numpy(tab).to(dev)
    out = [torch.empty((B, SS_OP_BEAM_CAND), dtype=torch.float32, device=dev)] + \
          [torch.empty((B, SS_OP_BEAM_CAND), dtype=torch.int32, device=dev) for _ in range(3)]
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    S = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731

    def topk():
        return model.lib.ss_op_beam_topk(S(), P(logits), R, V, k, 3, 1, P(mxl), P(zi), P(zi), P(cum), model.cfg.pad, model.cfg.unk,
                                         model.cfg.eos, 0.0, P(cand_s), P(cand_t))

    def select():
        return model.lib.ss_op_beam_cons_select(S(), P(cand_s), P(cand_t), P(next_s), P(next_t), P(state), P(d_tab), B, k, 3,
                                                *[P(o) for o in out])
    res = []
    for fn in (topk, select):
        ms = []
        for _ in range(passes + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = fn()
            b.record()
            assert rc == 0, rc
            torch.cuda.synchronize()
            ms.append(a.elapsed_time(b))
        res.append(statistics.median(ms[1:]))
    return res


def measure(out_path):
    import numpy as np
    import torch
    from streamspeech_amd import synth, workload
    from streamspeech_amd.config import ModelConfig
    from streamspeech_amd.engine import HipModel
    if not torch.cuda.is_available():
        raise SystemExit("mt_constraints_bench measures on the GPU; a CPU run provides no timing")
    cfg = ModelConfig()
    m = HipModel(synth.make_model_state_dict(0, cfg), cfg)
    utts = workload.make_utterances(PACK)
    pcm = torch.cat([torch.from_numpy(synth.synth_pcm(1234 + u.idx, u.n_samples)) for u in utts]).to(m.device)
    feat, T = m.batch_fbank_cmvn(pcm, [u.n_samples for u in utts])
    enc, Tp = m.batch_encoder_forward(feat, T)
    Tp = [int(t) for t in Tp]
    mx = [MAX_LEN] * PACK
    passes = int(os.environ.get("SS_BENCH_PASSES", "5"))
    rng = np.random.default_rng(0)
    glossary = [[[int(rng.integers(4, cfg.tgt_vocab))], [int(t) for t in rng.integers(4, cfg.tgt_vocab, 2)]] for _ in range(PACK)]
    rows = []
    for beam in BEAMS:
        def cons(c):
            return m._mt_beam("ss_batch_mt_beam", enc, Tp, None, mx, beam, 1, 1, 0.0, True, (1.0, 1.0, 0), constraints=c)[0]
        sides = (("plain", lambda: m.batch_mt_beam(enc, Tp, mx, beam)), ("empty", lambda: cons([[]] * PACK)),
                 ("glossary", lambda: cons(glossary)))
        plain, empty, got = (fn() for _, fn in sides)             # warm-up of all sides: scratch growth, first launches
        plain = plain[0]
        assert [[h["tokens"] for h in a] for a in plain] == [[h["tokens"] for h in a] for a in empty]
        met = sum(all(t in h["tokens"] for p in g for t in p) for g, a in zip(glossary, got) for h in a[:1])
        med = {name: [] for name, _ in sides}
        for _ in range(passes):
            for name, fn in sides:
                med[name].append(statistics.median(_timed(fn) for _ in range(CALLS)))
        topk_ms, select_ms = _kernels_ms(m, beam, passes)
        row = {"beam": beam, "utterances": PACK, "rows": PACK * beam, "max_len": MAX_LEN, "steps": MAX_LEN + 1, "passes_per_side": passes,
               "calls_per_pass": CALLS, "glossary_hypotheses_0_holding_every_phrase": met,
               **{name: _side(v) for name, v in med.items()}}
        for name in ("empty", "glossary"):
            row[f"ratio_{name}_over_plain"] = round(row[name]["call_ms_median"] / row["plain"]["call_ms_median"], 4)
        for name in med:
            row[f"spread_{name}"] = round(row[name]["call_ms_pass_max"] / row[name]["call_ms_pass_min"], 4)
        row["kernels_on_32_utterances_ms"] = {"plain_top2k_kernel": round(topk_ms, 4), "rank_merge_and_selection_kernel": round(select_ms, 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"tool": "tools/mt_constraints_bench.py", "device": torch.cuda.get_device_name(0),
           "order": "alternating passes: plain, empty, glossary, plain, ...", "settings": rows}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    measure(ap.parse_args().out)
