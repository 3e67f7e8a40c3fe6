"""Host side of the concurrent text sessions (streamspeech_amd/text_policy.py, text_pool.py, engine.plan_mt_continue): the shared
read/write gate and search-length rule against the agents' own arithmetic, the layout of a ragged continuation and the refusals of
ss_batch_mt_continue -- read from the library's own planner (ss_batch_mt_continue_plan, the code the call runs) -- and the pool's
capacity arithmetic.  No GPU (the library loads without one)."""
import os

import pytest

from streamspeech_amd import lib as L
from streamspeech_amd.engine import ContinueRefused, plan_mt_continue
from streamspeech_amd.text_policy import mt_max_len, s2tt_gate


@pytest.fixture(scope="module", autouse=True)
def _library():
    if not os.path.exists(L.LIB_PATH):            # a clean checkout before build(): the planner lives in the library
        import __graft_entry__
        __graft_entry__.build()


def _agent_gate(ns, nt, src, tgt, committed, k1, n, finished):
    """StreamSpeechS2TTAgent.policy's gate as the reference agent writes it (speech_to_text.s2tt.streamspeech.agent.py)."""
    if finished:
        return True, src, tgt, -1
    if ns < src + n or nt < tgt + n:
        return False, src, tgt, None
    src, tgt = max(ns, src), max(nt, tgt)
    sub = ((nt - k1) // n) * n
    new = sub - committed
    return new >= 1, src, tgt, new


@pytest.mark.parametrize("case", [
    (0, 0, 0, 0, 0, 0, 1, False), (3, 2, 0, 0, 0, 0, 1, False), (3, 2, 3, 2, 2, 0, 1, False), (5, 4, 3, 2, 2, 0, 1, False),
    (5, 4, 3, 2, 2, 3, 1, False), (6, 6, 3, 3, 2, 1, 2, False), (7, 7, 3, 3, 2, 1, 2, False), (9, 9, 6, 6, 4, 0, 3, False),
    (4, 1, 4, 1, 1, 0, 1, True), (1, 9, 0, 0, 0, 2, 1, False), (9, 1, 0, 0, 0, 0, 1, False), (10, 10, 0, 0, 9, 0, 1, False),
])
def test_gate_matches_agent_arithmetic(case):
    g = s2tt_gate(*case)
    w, src, tgt, new = _agent_gate(*case)
    assert (g.write, g.src_prefix_len, g.tgt_prefix_len) == (w, src, tgt)
    if new is not None:
        assert g.new_tokens == new


def test_max_len_rule_of_the_text_search():
    # max_new_tokens = -1: min(a * src_len + b, max_positions - 1) (the text agents: a = 1, b = 200)
    assert mt_max_len(0, 100, -1, 1, 200, 1200, 1) == 300
    assert mt_max_len(5, 2000, -1, 1, 200, 1200, 1) == 1199
    assert mt_max_len(4, 100, 3, 1, 200, 1200, 1) == 7
    with pytest.raises(IndexError):
        mt_max_len(9, 100, -3, 1, 200, 1200, 1)
    with pytest.raises(AssertionError):
        mt_max_len(0, 100, 0, 1, 200, 1200, 1)


def test_continue_layout():
    p = plan_mt_continue([7, 3, 5], [2, 0, 4], [4, 6, 4], 1, prefix_ids=[11, 12, 13, 14, 15, 16])
    assert p["S"] == 4 and p["Tn"] == 6 and p["Lcap"] == 11
    assert p["shift"] == [2, 4, 0] and p["r0"] == [0, 3, 4] and p["Np"] == 3 + 1 + 5
    assert p["feat_rows"] == 7 and p["out_stride"] == 7
    assert p["prefix_self"] == [(0, 3, 0, 3), (3, 1, 3, 1), (4, 5, 4, 5)]
    assert p["prefix_cross"] == [(0, 3, 0, 7), (3, 1, 7, 3), (4, 5, 10, 5)]
    # prefix rows land in the cache so that every row's first generated position is cache index S + 1 = 5
    assert p["cache_row"] == [2, 3, 4, 15, 22, 23, 24, 25, 26]
    assert p["feat_row"] == [0, 1, 2, 7, 14, 15, 16, 17, 18]
    assert p["max_len_at"] == [6, 10, 4] and p["min_len_at"] == [3, 5, 1]
    # step 0 feeds positions 3 / 1 / 5: keys 0 .. that position of each row
    assert p["step_self"][0] == [(0, 1, 2, 4), (1, 1, 15, 2), (2, 1, 22, 6)]
    assert p["step_cross"] == [(0, 1, 0, 7), (1, 1, 7, 3), (2, 1, 10, 5)]
    assert p["prefix_tokens"] == [2, 11, 12, 2, 2, 13, 14, 15, 16] and p["prefix_pos"] == [0, 1, 2, 0, 0, 1, 2, 3, 4]
    assert p["last_row"] == [2, 3, 8]
    # an empty prefix gives the segments of ss_batch_mt_greedy: no shift, cache index = position, step t feeds position t + 1
    q = plan_mt_continue([4, 4], [0, 0], [3, 5], 1)
    assert q["shift"] == [0, 0] and q["Lcap"] == 6 and q["step_self"][2] == [(0, 1, 0, 4), (1, 1, 6, 4)]
    assert q["step_cross"] == [(0, 1, 0, 4), (1, 1, 4, 4)] and q["prefix_tokens"] == [2, 2]


@pytest.mark.parametrize("args,code", [
    (dict(Tp=[3], n_prefix=[2], max_len=[1]), L.SS_ERR_ARG),            # start > max_len
    (dict(Tp=[0], n_prefix=[0], max_len=[3]), L.SS_ERR_ARG),            # no encoder rows
    (dict(Tp=[1] * 257, n_prefix=[0] * 257, max_len=[2] * 257), L.SS_ERR_ARG),
    (dict(Tp=[3], n_prefix=[1], max_len=[5], feat_rows=5), L.SS_ERR_CAPACITY),
    (dict(Tp=[3], n_prefix=[1], max_len=[5], out_stride=4), L.SS_ERR_CAPACITY),
    (dict(Tp=[3], n_prefix=[1], max_len=[1024], max_tgt_pos=1026), L.SS_ERR_CAPACITY),
    (dict(Tp=[3], n_prefix=[1], max_len=[4], prefix_ids=[6000], vocab=6000), L.SS_ERR_ARG),
])
def test_continue_refusals(args, code):
    with pytest.raises(ContinueRefused) as e:
        plan_mt_continue(args.pop("Tp"), args.pop("n_prefix"), args.pop("max_len"), 1, **args)
    assert e.value.code == code


def test_pool_capacity_arithmetic():
    from streamspeech_amd.text_pool import _encoder_out_len, fbank_frames_after
    assert fbank_frames_after(16000, 239) == 0 and fbank_frames_after(16000, 400) == 1 and fbank_frames_after(16000, 16000) == 98
    assert _encoder_out_len(98) == 25
    # 48 kHz: frames of the resampled history (one second -> as many rows as one second at 16 kHz, up to the cut-off)
    assert abs(fbank_frames_after(48000, 48000) - 98) <= 1
