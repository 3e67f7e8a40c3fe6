"""The three controls of the first-pass text search, restated in numpy over explicit token rows (include/streamspeech_hip.h,
ss_mt_search_opts).  Written from the rules, not from the kernels: the tests hold csrc/beam_kernels.hip against this file, and this file
against the reference's NGramRepeatBlock where the reference tree is present (tests/test_search_options_cpu.py).

A hypothesis row at reference step `step` holds tokens[0 .. step]: </s>, the forced prefix, the generated tokens."""
import numpy as np


def banned_tokens(tokens, n):
    """tokens = the row's tokens[0 .. step] -> the set of token ids the no-repeat rule of size n bans at this step.
    step + 2 - n >= 0 windows start at i < step + 2 - n; window i = tokens[i : i + n - 1] against the last n - 1 tokens; a match
    bans tokens[i + n - 1]."""
    tokens = [int(t) for t in tokens]
    step = len(tokens) - 1
    if n < 2:
        raise ValueError("n-gram size below 2")
    last = tokens[len(tokens) - (n - 1):]
    return {tokens[i + n - 1] for i in range(max(step + 2 - n, 0)) if tokens[i:i + n - 1] == last}


def apply_ban(rows, lprobs, n):
    """rows: one token list per hypothesis row (tokens[0 .. step]); lprobs [R, V] float32 -> a copy with the banned entries -inf."""
    out = np.array(lprobs, dtype=np.float32, copy=True)
    for r, toks in enumerate(rows):
        for t in banned_tokens(toks, n):
            out[r, t] = -np.inf
    return out


def prefix_repeats(prefix, n, eos=2):
    """Does [</s>] + prefix hold the same n-gram twice -- would the ban hit one of the prefix' own forced tokens?"""
    toks = [eos] + [int(t) for t in prefix]
    return any(toks[q] in banned_tokens(toks[:q], n) for q in range(1, len(toks)))


def log_softmax_t(logits, temperature):
    """float64 log-softmax of logits / T, the division made in float32 as the search makes it."""
    x = (np.asarray(logits, dtype=np.float32) / np.float32(temperature)).astype(np.float64)
    x = x - x.max(axis=-1, keepdims=True)
    return x - np.log(np.exp(x).sum(axis=-1, keepdims=True))


def final_score(cum, step, len_penalty, normalize=True):
    """Score of a hypothesis finalised at reference step `step` with cumulative score cum, in float64."""
    return float(cum) / float(step + 1) ** float(len_penalty) if normalize else float(cum)
