"""The host-side decisions of the streaming text agents, in one place: the read/write gate of the simultaneous S2TT agent (reference
agent/speech_to_text.s2tt.streamspeech.agent.py:480-512) and the length rule of the first-pass text search (agent/sequence_generator.py:
229-245, 340).  StreamSpeechS2TTAgent, SequenceGenerator and the concurrent text session pool (text_pool.py) all call these, so a
session decides the same way whichever of them serves it."""
from typing import NamedTuple


class Gate(NamedTuple):
    write: bool                # run the text search this call
    src_prefix_len: int        # the agent's src_ctc_prefix_length after the call
    tgt_prefix_len: int        # ... and tgt_ctc_prefix_length
    new_tokens: int            # max_new_tokens of the search (-1: the source is finished, search to the end)


def s2tt_gate(n_src_ctc: int, n_tgt_ctc: int, src_prefix_len: int, tgt_prefix_len: int, n_committed: int, lagging_k1: int,
              stride_n: int, source_finished: bool) -> Gate:
    """Read/write gate on the CTC token counts of the two heads.  n_committed = target subwords committed so far (0 before the
    first write).  A read keeps the prefix lengths as they were unless both heads grew by stride_n (then they advance, as the agent
    stores them before it checks the lagging rule)."""
    if source_finished:
        return Gate(True, src_prefix_len, tgt_prefix_len, -1)
    if n_src_ctc < src_prefix_len + stride_n or n_tgt_ctc < tgt_prefix_len + stride_n:
        return Gate(False, src_prefix_len, tgt_prefix_len, 0)
    src_prefix_len = max(n_src_ctc, src_prefix_len)
    tgt_prefix_len = max(n_tgt_ctc, tgt_prefix_len)
    subword_tokens = ((n_tgt_ctc - lagging_k1) // stride_n) * stride_n
    new_tokens = subword_tokens - n_committed
    return Gate(new_tokens >= 1, src_prefix_len, tgt_prefix_len, new_tokens)


def mt_max_len(start: int, src_len: int, max_new_tokens: int, max_len_a: float, max_len_b: int, max_len: int,
               min_len: int) -> int:
    """Forced-</s> position of a greedy continuation of a `start`-token prefix: prefix + max_new_tokens, or with max_new_tokens = -1
    min(max_len_a * src_len + max_len_b, max_len - 1) (src_len = fbank frames).  Raises as the reference does when no hypothesis
    can be finalized (AssertionError for min_len > max_len, IndexError for a prefix past max_len)."""
    if max_new_tokens == -1:
        out = min(int(max_len_a * src_len + max_len_b), max_len - 1)
    else:
        out = start + max_new_tokens
    assert min_len <= out, "min_len cannot be larger than max_len, please adjust these!"
    if start > out:
        # the reference's step loop `for step in range(start, max_len + 1)` (agent/sequence_generator.py:340) is empty
        # then, nothing is finalized and the agent's finalized_mt[0][0] raises IndexError: same error here
        raise IndexError(f"prefix of {start} tokens is longer than max_len = {out}: no hypothesis can be finalized")
    return out
