"""Host logic of the streaming session pool (engine.StreamPool / plan_pool_step) that needs no GPU: the packed layout of a step,
which sessions take part in it, the argument checks that refuse a bad step before any device call, and a loud failure without a GPU."""
import types

import pytest
import torch

from streamspeech_amd import lib as L
from streamspeech_amd.engine import StreamPool, plan_pool_step


def _out_len(T):
    t1 = (T + 4 - 5) // 2 + 1
    return (t1 + 4 - 5) // 2 + 1


def test_plan_layout_in_call_order():
    T = [83, 200, 40, 131]
    n = [21, 3, 0, 9]            # rows each session recomputes (session 2: all final)
    p = plan_pool_step(T, n, 256)
    assert p["T2"] == [_out_len(t) for t in T] == [21, 50, 10, 33]
    assert p["off"] == [0, 21, 71, 81] and p["total"] == 114            # packed output: session 0's rows, then 1's, ...
    assert p["q_start"] == [0, 21, 24, 24] and p["M"] == 33              # stacked tail rows of the sessions that compute
    assert p["active"] == [0, 1, 3]                                      # all-final sessions take no part in the layers
    assert p["qtiles"] == [2, 1, 0, 1]


def test_plan_refuses_bad_steps():
    with pytest.raises(ValueError):
        plan_pool_step([400], [0], 96)          # 99 output rows > max_rows
    with pytest.raises(ValueError):
        plan_pool_step([0], [0], 96)            # no frames
    with pytest.raises(ValueError):
        plan_pool_step([83], [22], 96)          # more rows to compute than the session has
    assert plan_pool_step([383], [0], 96)["T2"] == [96]                   # exactly max_rows is fine


def test_step_argument_checks_before_any_device_call():
    fake = types.SimpleNamespace(max_sessions=4, max_rows=64)
    fb = [torch.zeros(100, 80), torch.zeros(120, 80)]
    assert StreamPool.check_step(fake, [0, 3], fb)["T2"] == [_out_len(100), _out_len(120)]
    with pytest.raises(ValueError):
        StreamPool.check_step(fake, [1, 1], fb)                           # duplicate slot
    with pytest.raises(ValueError):
        StreamPool.check_step(fake, [0, 4], fb)                           # slot outside the pool
    with pytest.raises(ValueError):
        StreamPool.check_step(fake, [0], fb)                              # one fbank per slot
    with pytest.raises(ValueError):
        StreamPool.check_step(fake, [0, 1], [fb[0], torch.zeros(300, 80)])   # 74 rows > max_rows 64
    with pytest.raises(ValueError):
        StreamPool.check_step(fake, [0, 1], fb, [8], [8, 8])              # one attention chunk per slot
    with pytest.raises(ValueError):
        StreamPool.check_step(fake, [0, 1], fb, [8, 8], [8, 8, 8])        # one conv chunk per slot


def test_pool_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    fake = types.SimpleNamespace(lib=None, device="cuda:0", h=None)
    with pytest.raises(L.StreamSpeechHipError, match="no CPU fallback"):
        StreamPool(fake, 4, 64)


def test_pool_abi_is_declared_and_bound():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "streamspeech_hip.h")).read()
    for name in ("ss_stream_pool_create", "ss_stream_pool_destroy", "ss_stream_pool_reset", "ss_stream_pool_set_tail",
                 "ss_encoder_stream_forward_batch", "ss_stream_pool_ctc", "ss_stream_pool_stats"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
        assert name in L.SIGNATURES, name
