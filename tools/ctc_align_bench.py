"""What a forced alignment costs beside the scored greedy search.  One 128-utterance pack of the bench workload goes through the
encoder once; then, per text head, on the same packed encoder output and in ALTERNATING passes (greedy, align, greedy, align, ...)
so that clock and thermal drift fall on both:
  greedy  batch_ctc_greedy(head, enc, Tp, return_scores=True)     head GEMM + arg-max / log-prob kernel + span collapse, one D2H copy
  align   batch_ctc_align(head, enc, Tp, labels)                  head GEMM + per-frame kernel + trellis kernel, one D2H copy
with labels = the greedy hypothesis of each utterance.  Each call is timed on the host, synchronised before and after, so both sides
include their device-to-host copy and host unpacking.  Per side: the median call in each pass, the median over passes and the
run-to-run spread (lowest and highest pass median); the ratio align / greedy is only meaningful beside that spread.

Where the time goes: the two alignment kernels alone on the head's own logits (ss_op_ctc_align between two events), the same call
with every label list empty -- the per-frame kernel's cost is the row denominators, which do not depend on the labels, and the
trellis of an empty list is one state wide -- and the differences: trellis ~ kernels - per-frame, GEMM + copy + host ~ call - kernels.
These are estimates from differences of medians, not a kernel trace.

The register / LDS figures of the two kernels come from hipcc -Rpass-analysis=kernel-resource-usage on csrc/ctc_align.hip when hipcc is
at hand (no device needed: --resources-only prints them alone).

  python tools/ctc_align_bench.py --out profiles/ctc_align.json      SS_BENCH_PASSES passes per side (default 7)"""
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

PACK, CALLS = 128, 5


def kernel_resources():
    """{kernel: {vgprs, sgprs, lds_bytes_static, scratch_bytes, occupancy_waves_per_simd}} of csrc/ctc_align.hip, or None without hipcc."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        return None
    src = os.path.join(ROOT, "streamspeech_amd", "csrc", "ctc_align.hip")
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
            name = "ctc_align_lp_kernel" if "ctc_align_lp_kernel" in m.group(1) else \
                   "ctc_align_trellis_kernel" if "ctc_align_trellis_kernel" in m.group(1) else None
            if name:
                out[name] = {}
        elif name and m.group(2).strip() in keys:
            out[name][keys[m.group(2).strip()]] = int(m.group(3))
    if "ctc_align_trellis_kernel" in out:
        out["ctc_align_trellis_kernel"]["lds_bytes_dynamic"] = "16 * (2 L + 1) + 4 * (L + T') over the pack's largest L and T' (60 016 at the limits)"
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


def _kernels_ms(model, logits, Tp, labels, passes):
    """The two kernels on `logits` between two events: the median over `passes` launches, in ms."""
    import torch
    B, V = len(Tp), logits.shape[1]
    flat = [int(v) for y in labels for v in y]
    nl, tot = len(flat), sum(Tp)
    res = torch.empty((6 * B,), dtype=torch.int32, device=logits.device)
    ibuf = torch.empty((tot + 2 * max(nl, 1),), dtype=torch.int32, device=logits.device)
    fbuf = torch.empty((max(nl, 1),), dtype=torch.float32, device=logits.device)
    i32 = lambda v: (C.c_int32 * max(len(v), 1))(*(v or [0]))  # noqa: E731
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    hT, hy, hn = i32(Tp), i32(flat), i32([len(y) for y in labels])
    ms = []
    for _ in range(passes + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        rc = model.lib.ss_op_ctc_align(C.c_void_p(torch.cuda.current_stream().cuda_stream), P(logits), V, V, model.cfg.pad, B, hT, hy, hn,
                                       P(res), P(ibuf), P(ibuf[tot:]), P(ibuf[tot + max(nl, 1):]), P(fbuf), None)
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
        raise SystemExit("ctc_align_bench measures on the GPU; a CPU run provides no timing (--resources-only needs none)")
    cfg = ModelConfig()
    m = HipModel(synth.make_model_state_dict(0, cfg), cfg)
    utts = workload.make_utterances(PACK)
    pcm = torch.cat([torch.from_numpy(synth.synth_pcm(1234 + u.idx, u.n_samples)) for u in utts]).to(m.device)
    feat, T = m.batch_fbank_cmvn(pcm, [u.n_samples for u in utts])
    enc, Tp = m.batch_encoder_forward(feat, T)
    passes = int(os.environ.get("SS_BENCH_PASSES", "7"))
    heads = []
    for hd in (0, 1):
        labels = [r[0] for r in m.batch_ctc_greedy(hd, enc, Tp, return_scores=True)]
        got = m.batch_ctc_align(hd, enc, Tp, labels)          # warm-up of both sides: scratch growth, first launches
        assert all(a.status == 0 for a in got)
        med = {"greedy": [], "align": []}
        for _ in range(passes):
            for side, fn in (("greedy", lambda: m.batch_ctc_greedy(hd, enc, Tp, return_scores=True)),
                             ("align", lambda: m.batch_ctc_align(hd, enc, Tp, labels))):
                med[side].append(statistics.median(_timed(fn) for _ in range(CALLS)))
        m.batch_ctc_greedy(hd, enc, Tp)
        logits = m.last_logits()
        both = _kernels_ms(m, logits, Tp, labels, passes)
        frame = _kernels_ms(m, logits, Tp, [[] for _ in Tp], passes)
        row = {"head": hd, "utterances": PACK, "frames": sum(Tp), "labels": sum(len(y) for y in labels),
               "longest_frames": max(Tp), "longest_labels": max(len(y) for y in labels), "passes_per_side": passes,
               "calls_per_pass": CALLS, "greedy": _side(med["greedy"]), "align": _side(med["align"])}
        row["ratio_align_over_greedy"] = round(row["align"]["call_ms_median"] / row["greedy"]["call_ms_median"], 4)
        row["spread_greedy"] = round(row["greedy"]["call_ms_pass_max"] / row["greedy"]["call_ms_pass_min"], 4)
        row["spread_align"] = round(row["align"]["call_ms_pass_max"] / row["align"]["call_ms_pass_min"], 4)
        row["where_the_time_goes_ms"] = {
            "both_kernels_on_the_same_logits": round(both, 4), "per_frame_kernel_estimate": round(frame, 4),
            "trellis_kernel_estimate": round(both - frame, 4),
            "head_gemm_copy_and_host_estimate": round(row["align"]["call_ms_median"] - both, 4)}
        heads.append(row)
        print(json.dumps(row), flush=True)
    res = {"tool": "tools/ctc_align_bench.py", "device": torch.cuda.get_device_name(0),
           "order": "alternating passes: greedy, align, greedy, align, ...", "labels": "the greedy hypothesis of each utterance",
           "heads": heads, "kernel_resources": kernel_resources()}
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
