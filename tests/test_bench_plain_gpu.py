"""A plain `bench.py` run (no --full) does what its headline needs and nothing else: set-up, warm-up, the timed steps,
--dump-outputs and the line.  Every other leg (latency pass, roofline replay, soak, configs[4], pack-invariance / RCCL checks,
CPU baseline, streaming) is behind --full; the timed region still carries the dominant-class event brackets of the parent
arrangement, whose in-region sums go to the sidecar."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_a_plain_run_times_the_steps_and_runs_no_other_leg(tmp_path):
    side, dump = tmp_path / "detail.json", tmp_path / "dump"
    env = dict(os.environ, SS_BENCH_DETAIL=str(side))
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "SS_FORCE_DIST"):
        env.pop(k, None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "32", "--streams", "2",
           "--dump-outputs", str(dump)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["steps"] == 2 and line["warmup"] == 1
    assert line["unit"] == "x real-time" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["cpu_baseline"] is None and line["roofline"] is None and line["pack_invariance"] is None and line["rccl"] is None
    for k in ("soak", "multilingual", "streaming_320ms", "bf16x3", "roofline_family"):
        assert k not in line, k
    full = json.load(open(side))
    for k in ("latency_ms_single_stream", "batch1_8streams", "dispatch", "event_bracket_perturbation", "roofline_second_kernel"):
        assert full[k] is None, k
    assert full["roofline_in_region"] and all(r["launches"] > 0 and r["concurrent_streams"] == 2 for r in full["roofline_in_region"])
    assert full["dumped_outputs"]["files"] and (dump / "wav.npy").exists() and (dump / "mt_tokens.npy").exists()
