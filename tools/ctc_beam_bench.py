"""What a CTC prefix beam search costs beside the scored greedy search.  One 128-utterance pack of the bench workload goes through the
encoder once; then, on one text head and the same packed encoder output, per setting beam / cand = 4/8, 8/16, 32/32 in ALTERNATING
passes (greedy, beam, greedy, beam, ...) so that clock and thermal drift fall on both:
  greedy  batch_ctc_greedy(head, enc, Tp, return_scores=True)     head GEMM + arg-max / log-prob kernel + span collapse, one D2H copy
  beam    batch_ctc_beam(head, enc, Tp, beam, cand)               head GEMM + table fill + candidate kernel + search kernel, one D2H copy
Each call is timed on the host, synchronised before and after, so both sides include their device-to-host copy and host unpacking.
Per side: the median call in each pass, the median over passes and the run-to-run spread (lowest and highest pass median); the ratio
beam / greedy is only meaningful beside that spread.

The two kernels apart: ss_op_ctc_beam on the head's own logits between two events (fill + both kernels), and the same call with
every frame row declared an utterance of its own -- the candidate kernel does the same work on the same rows, the search is one
frame per workgroup -- as the candidate kernel's estimate; the search kernel ~ the difference.  Estimates from differences of
medians, not a kernel trace.

The register / LDS figures of the kernels come from hipcc -Rpass-analysis=kernel-resource-usage on csrc/ctc_beam.hip when hipcc is at
hand (no device needed: --resources-only prints them alone).

  python tools/ctc_beam_bench.py --out profiles/ctc_beam.json      SS_BENCH_PASSES passes per side (default 7)"""
import argparse
import ctypes as C
import json
import os
import re
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PACK, CALLS, HEAD = 128, 5, 0
SETTINGS = ((4, 8), (8, 16), (32, 32))


def kernel_resources():
    """{kernel: {vgprs, sgprs, lds_bytes_static, scratch_bytes, occupancy_waves_per_simd}} of csrc/ctc_beam.hip, or None without hipcc."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    src = os.path.join(ROOT, "streamspeech_amd", "csrc", "ctc_beam.hip")
    with tempfile.TemporaryDirectory() as d:
        p = subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", src, "-o", os.path.join(d, "x.o"),
                            "-Rpass-analysis=kernel-resource-usage"], capture_output=True, text=True)
    out, name = {}, None
    keys = {"VGPRs": "vgprs", "TotalSGPRs": "sgprs", "LDS Size [bytes/block]": "lds_bytes_static", "ScratchSize [bytes/lane]": "scratch_bytes",
            "Occupancy [waves/SIMD]": "occupancy_waves_per_simd"}
    for line in p.stderr.splitlines():
        m = re.search(r"remark:\s+(?:Function Name: (\S+)|([A-Za-z][^:]*): (\d+))", line)
        if not m:
            continue
        if m.group(1):
            k = re.search(r"ctc_beam_cand_kernelILi(\d+)E", m.group(1))
            name = f"ctc_beam_cand_kernel<{k.group(1)}>" if k else "ctc_beam_search_kernel" if "ctc_beam_search_kernel" in m.group(1) else None
            if name:
                out[name] = {}
        elif name and m.group(2).strip() in keys:
            out[name][keys[m.group(2).strip()]] = int(m.group(3))
    return out or None


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


def _kernels_ms(model, logits, T, beam, cand, passes):
    """The table fill and the two kernels on `logits` between two events: the median over `passes` launches, in ms."""
    import torch
    B, V = len(T), logits.shape[1]
    stride = max(T)
    hyp = torch.empty((4 * B * beam,), dtype=torch.int32, device=logits.device)
    tok = torch.empty((B * beam * stride,), dtype=torch.int32, device=logits.device)
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    hT = (C.c_int32 * B)(*T)
    ms = []
    for _ in range(passes + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = model.lib.ss_op_ctc_beam(C.c_void_p(torch.cuda.current_stream().cuda_stream), P(logits), V, V, model.cfg.pad, model.cfg.unk, B,
                                      hT, beam, cand, beam, P(hyp), P(tok), stride, None, None)
        b.record()
        assert rc == 0, rc
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms[1:])                       # the first launch sizes the op's scratch


def measure(out_path):
    import torch
    from streamspeech_amd import synth, workload
    from streamspeech_amd.config import ModelConfig
    from streamspeech_amd.engine import HipModel
    if not torch.cuda.is_available():
        raise SystemExit("ctc_beam_bench measures on the GPU; a CPU run provides no timing (--resources-only needs none)")
    cfg = ModelConfig()
    m = HipModel(synth.make_model_state_dict(0, cfg), cfg)
    utts = workload.make_utterances(PACK)
    pcm = torch.cat([torch.from_numpy(synth.synth_pcm(1234 + u.idx, u.n_samples)) for u in utts]).to(m.device)
    feat, T = m.batch_fbank_cmvn(pcm, [u.n_samples for u in utts])
    enc, Tp = m.batch_encoder_forward(feat, T)
    Tp = [int(t) for t in Tp]
    passes = int(os.environ.get("SS_BENCH_PASSES", "7"))
    greedy = [r[0] for r in m.batch_ctc_greedy(HEAD, enc, Tp, return_scores=True)]
    rows = []
    for beam, cand in SETTINGS:
        got = m.batch_ctc_beam(HEAD, enc, Tp, beam, cand)     # warm-up of both sides: scratch growth, first launches
        assert all(len(h) >= 1 for h in got)
        med = {"greedy": [], "beam": []}
        for _ in range(passes):
            for side, fn in (("greedy", lambda: m.batch_ctc_greedy(HEAD, enc, Tp, return_scores=True)),
                             ("beam", lambda: m.batch_ctc_beam(HEAD, enc, Tp, beam, cand))):
                med[side].append(statistics.median(_timed(fn) for _ in range(CALLS)))
        m.batch_ctc_greedy(HEAD, enc, Tp)
        logits = m.last_logits()
        both = _kernels_ms(m, logits, Tp, beam, cand, passes)
        frame = _kernels_ms(m, logits, [1] * sum(Tp), beam, cand, passes)
        row = {"head": HEAD, "beam": beam, "cand": cand, "nbest": beam, "utterances": PACK, "frames": sum(Tp), "longest_frames": max(Tp),
               "passes_per_side": passes, "calls_per_pass": CALLS, "greedy": _side(med["greedy"]), "beam_search": _side(med["beam"]),
               "best_differs_from_greedy_in": sum(h[0].tokens != g for h, g in zip(got, greedy))}
        row["ratio_beam_over_greedy"] = round(row["beam_search"]["call_ms_median"] / row["greedy"]["call_ms_median"], 4)
        row["spread_greedy"] = round(row["greedy"]["call_ms_pass_max"] / row["greedy"]["call_ms_pass_min"], 4)
        row["spread_beam"] = round(row["beam_search"]["call_ms_pass_max"] / row["beam_search"]["call_ms_pass_min"], 4)
        row["where_the_time_goes_ms"] = {
            "fill_and_both_kernels_on_the_same_logits": round(both, 4), "candidate_kernel_estimate": round(frame, 4),
            "search_kernel_estimate": round(both - frame, 4),
            "head_gemm_copy_and_host_estimate": round(row["beam_search"]["call_ms_median"] - both, 4)}
        rows.append(row)
        print(json.dumps(row), flush=True)
    res = {"tool": "tools/ctc_beam_bench.py", "device": torch.cuda.get_device_name(0),
           "order": "alternating passes: greedy, beam, greedy, beam, ...", "settings": rows, "kernel_resources": kernel_resources()}
    if out_path:
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return res


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--resources-only", action="store_true")
    a = ap.parse_args()
    if a.resources_only:
        print(json.dumps(kernel_resources(), indent=1))
    else:
        measure(a.out)
