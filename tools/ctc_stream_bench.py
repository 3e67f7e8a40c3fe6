"""What the resumable CTC prefix beam search costs a streaming ASR session pool.  N = 1, 16 and 64 ASR sessions (TextSessionPool, 320-ms
segments) are fed 10 s of audio step by step; the steps that follow, with 10 s of history behind them, are timed on the host
(pool.step, synchronised before and after: front-end, encoder step, CTC side, the device-to-host copy, the host's text).  Four
configurations in ALTERNATING passes (a, b, c, d, parent, a, ...) so that clock and thermal drift fall on all sides:
  a  greedy     TextSessionPool(model, N, rows)                              the arg-max frame path
  b  beam       TextSessionPool(..., ctc_beam=CtcBeamOptions(8))             the resumable search, no model
  c  beam_lm    ... CtcBeamOptions(8, lm=order-3 model of about 10^6 entries, as tools/ctc_lm_bench.py builds it, lm_weight 0.5)
  d  rerun      the greedy pool, plus batch_ctc_beam(head 0, beam 8) over every session's WHOLE encoder output after each step: what
                the pool would pay without the resumable object
  parent        the greedy pool on the parent build (--parent-lib), in a child process that stays up and measures a pass when told to
Per side: the median timed step in each pass, the median over passes and the run-to-run spread (highest / lowest pass median).
Reported as measured, with no ratio fixed in advance: b / a, c / b, d / b, a / parent beside the spread of a against itself
(`greedy_inside_its_own_spread_of_parent`: the greedy pool's launches are meant to be untouched), and the history length at which d's step
first costs more than b's (every step of the 10-s feed is timed for that, per side the median over passes).

  python tools/ctc_stream_bench.py --out profiles/ctc_stream.json [--parent-lib PARENT.so]     SS_BENCH_PASSES passes (default 5)"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SEG_MS, SR, HISTORY_S, TIMED_STEPS, BEAM, MAX_ROWS = 320, 16000, 10, 5, 8, 320
NEW_SYMBOLS = ("ss_ctc_stream_create", "ss_ctc_stream_destroy", "ss_ctc_stream_reset", "ss_ctc_stream_advance",
               "ss_ctc_stream_advance_host", "ss_debug_ctc_stream_create", "ss_op_ctc_stream_advance")


def _args():
    from streamspeech_amd.agent_text import StreamSpeechASRAgent
    p = argparse.ArgumentParser()
    StreamSpeechASRAgent.add_args(p)
    a = p.parse_args(["--model-path", "synthetic:0", "--data-bin", "/nonexistent", "--sample-rate", str(SR)])
    a.source_segment_size = SEG_MS
    return a


def _model():
    import torch
    from streamspeech_amd import synth
    from streamspeech_amd.config import ModelConfig
    from streamspeech_amd.engine import HipModel
    if not torch.cuda.is_available():
        raise SystemExit("ctc_stream_bench measures on the GPU; a CPU run provides no timing")
    cfg = ModelConfig()
    return HipModel(synth.make_model_state_dict(0, cfg), cfg)


def _segments(N):
    """Per session its segments: HISTORY_S seconds plus TIMED_STEPS more steps; the source never finishes."""
    from streamspeech_amd import synth
    from streamspeech_amd.simuleval_shim import SpeechSegment
    step = SR * SEG_MS // 1000
    n_steps = HISTORY_S * 1000 // SEG_MS + TIMED_STEPS
    out = []
    for i in range(N):
        pcm = synth.synth_pcm(4000 + i, step * n_steps)
        out.append([SpeechSegment(content=pcm[k * step:(k + 1) * step].tolist(), sample_rate=SR, finished=False) for k in range(n_steps)])
    return out


class Side:
    """One configuration at one N: a pool, its sessions, and a pass over the whole feed -> the per-step times in ms."""

    def __init__(self, model, N, segs, ctc_beam=None, rerun=False):
        from streamspeech_amd.text_pool import TextSessionPool
        self.model, self.segs, self.rerun = model, segs, rerun
        self.pool = TextSessionPool(model, N, MAX_ROWS, ctc_beam=ctc_beam) if ctc_beam is not None else TextSessionPool(model, N, MAX_ROWS)
        args = _args()
        self.sids = [self.pool.open("asr", args) for _ in range(N)]

    def run(self):
        import torch
        for sid in self.sids:
            self.pool.reset(sid)
        ms = []
        for k in range(len(self.segs[0])):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            self.pool.step({sid: self.segs[i][k] for i, sid in enumerate(self.sids)})
            if self.rerun:
                _, T2, out = self.pool.pool._last
                self.model.batch_ctc_beam(0, out, T2, BEAM)
            torch.cuda.synchronize()
            ms.append(1e3 * (time.perf_counter() - t0))
        return ms


def _side(vals):
    return {"step_ms_median": round(statistics.median(vals), 4), "step_ms_pass_min": round(min(vals), 4),
            "step_ms_pass_max": round(max(vals), 4), "spread": round(max(vals) / min(vals), 4), "pass_medians_ms": [round(v, 4) for v in vals]}


def child():
    """The parent build's side: `make <N>` / `pass` on stdin -> the pass's median timed step in ms on stdout; `quit` ends."""
    from streamspeech_amd import lib as L
    for name in NEW_SYMBOLS:                                     # the parent build has none of them
        L.SIGNATURES.pop(name, None)
    m = _model()
    side = None
    print("ready", flush=True)
    for line in sys.stdin:
        f = line.split()
        if not f or f[0] == "quit":
            break
        if f[0] == "make":
            side = Side(m, int(f[1]), _segments(int(f[1])))
            side.run()
            print("ok", flush=True)
        else:
            print(statistics.median(side.run()[-TIMED_STEPS:]), flush=True)


def measure(out_path, parent_lib):
    import torch
    from streamspeech_amd.ngram import NgramLM
    from streamspeech_amd.text_policy import CtcBeamOptions
    from tools.ctc_lm_bench import synthetic_lm
    par = None
    if parent_lib:                                               # started first: this process has not touched the device yet
        par = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                               text=True, env=dict(os.environ, SS_HIP_LIB=os.path.abspath(parent_lib)))
        assert par.stdout.readline().strip() == "ready", "the parent build's process did not come up"
    m = _model()
    passes = int(os.environ.get("SS_BENCH_PASSES", "5"))
    Ns = [int(x) for x in os.environ.get("SS_BENCH_N", "1,16,64").split(",")]
    t0 = time.perf_counter()
    lm = NgramLM(synthetic_lm(m.cfg.src_vocab, 3, 500000, 1))
    build_s = time.perf_counter() - t0

    def ask(cmd):
        par.stdin.write(cmd + "\n")
        par.stdin.flush()
        return par.stdout.readline().strip()
    rows = []
    try:
        for N in Ns:
            segs = _segments(N)
            sides = {"greedy": Side(m, N, segs), "beam": Side(m, N, segs, CtcBeamOptions(BEAM)),
                     "beam_lm": Side(m, N, segs, CtcBeamOptions(BEAM, lm=lm, lm_weight=0.5)), "rerun": Side(m, N, segs, rerun=True)}
            for s in sides.values():                             # warm-up: scratch growth, first launches, the model's upload
                s.run()
            if par:
                assert ask(f"make {N}") == "ok"
            med = {k: [] for k in list(sides) + (["parent"] if par else [])}
            steps = {k: [] for k in sides}
            for _ in range(passes):
                for k, s in sides.items():
                    ms = s.run()
                    steps[k].append(ms)
                    med[k].append(statistics.median(ms[-TIMED_STEPS:]))
                if par:
                    med["parent"].append(float(ask("pass")))
            row = {"sessions": N, "segment_ms": SEG_MS, "history_s": HISTORY_S, "timed_steps_per_pass": TIMED_STEPS, "passes_per_side": passes,
                   "beam": BEAM, **{k: _side(v) for k, v in med.items()}}
            a, b = row["greedy"]["step_ms_median"], row["beam"]["step_ms_median"]
            row["ratio_beam_over_greedy"] = round(b / a, 4)
            row["ratio_beam_lm_over_beam"] = round(row["beam_lm"]["step_ms_median"] / b, 4)
            row["ratio_rerun_over_beam"] = round(row["rerun"]["step_ms_median"] / b, 4)
            per = {k: [statistics.median(p[j] for p in v) for j in range(len(v[0]))] for k, v in steps.items()}
            cross = next((j for j in range(len(per["beam"])) if all(per["rerun"][i] > per["beam"][i] for i in range(j, len(per["beam"])))), None)
            row["rerun_costs_more_than_beam_from_history_s"] = None if cross is None else round((cross + 1) * SEG_MS / 1000, 2)
            row["step_ms_by_history"] = {k: [round(v, 3) for v in per[k][::5]] for k in ("beam", "rerun")}   # every fifth step (1.6 s)
            row["last_step_of_beam"] = {k: sides["beam"].pool.last_step[k] for k in ("ctc_stream_calls", "ctc_stream_rows", "encoded")}
            if par:
                r = a / row["parent"]["step_ms_median"]
                row["ratio_greedy_over_parent"] = round(r, 4)
                row["greedy_inside_its_own_spread_of_parent"] = bool(1.0 / row["greedy"]["spread"] <= r <= row["greedy"]["spread"])
            rows.append(row)
            print(json.dumps(row), flush=True)
    finally:
        if par:
            par.stdin.write("quit\n")
            par.stdin.flush()
            par.wait(timeout=60)
    res = {"tool": "tools/ctc_stream_bench.py", "device": torch.cuda.get_device_name(0),
           "order": "alternating passes: greedy, beam, beam_lm, rerun, parent, greedy, ...",
           "model": {"order": lm.order, "entries": lm.entries, "device_bytes": lm.device_bytes, "host_build_s": round(build_s, 2)},
           "parent_lib": bool(parent_lib), "runs": rows}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="libstreamspeech_hip.so of the parent commit: its greedy pool is timed beside this tree's")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        child()
    else:
        measure(a.out, a.parent_lib)
