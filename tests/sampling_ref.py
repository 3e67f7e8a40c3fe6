"""Sampling from the first-pass text decoder, restated in numpy from the rule (include/streamspeech_hip.h, ss_mt_sample_opts).
Written from the rule, not from the kernel: the tests hold csrc/beam_sample.hip against this file, and this file against the reference's
own Sampling._sample_topp / topk where the reference tree is present (tests/test_sampling_ref_cpu.py).

A row's candidate values v[n] are float64 here: the float32 division of the logits by the temperature, a float64 log-softmax, the
masks in the reference's order.  The kept sets and the draw are then exact statements over v."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """Philox4x32-10: counter (4 words), key (2 words) -> 4 words."""
    c = [int(x) & MASK for x in counter]
    k = [int(x) & MASK for x in key]
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> 32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return c


def words(seed, key, step, j):
    """The four Philox words of chain j of the utterance with `key` at reference step `step` under `seed` (64-bit patterns)."""
    seed, key = int(seed) & (2 ** 64 - 1), int(key) & (2 ** 64 - 1)
    return philox4x32_10([step, j, key & MASK, key >> 32], [seed & MASK, seed >> 32])


def uniform(seed, key, step, j, word=0):
    """u = (x >> 8) * 2^-24 of word 0 (another word: the mutant of the tests); exact in float32 and in float64."""
    return (words(seed, key, step, j)[word] >> 8) * 2.0 ** -24


def row_values(logits, temperature=1.0, pad=1, unk=3, eos=2, unk_pen=0.0, step=0, min_len=0, max_len=10 ** 9, banned=()):
    """One row of logits -> v[n], float64.  Masks in the reference's order: NaN, pad, unk penalty, max_len, min_len, the ban."""
    x = (np.asarray(logits, dtype=np.float32) / np.float32(temperature)).astype(np.float64)
    x = x - np.nanmax(x) if not np.isnan(x).all() else x
    with np.errstate(invalid="ignore"):
        v = x - np.log(np.nansum(np.exp(x))) if not np.isnan(x).any() else np.full_like(x, np.nan)
    v = np.where(np.isnan(v), -np.inf, v)
    V = v.shape[0]
    if 0 <= pad < V:
        v[pad] = -np.inf
    if 0 <= unk < V:
        v[unk] -= unk_pen
    if step >= max_len:
        keep = v[eos]
        v[:] = -np.inf
        v[eos] = keep
    if step < min_len:
        v[eos] = -np.inf
    for t in banned:
        v[int(t)] = -np.inf
    return v


def order(v):
    """The ids with v > -inf ordered by v descending, ties to the lower id."""
    ids = [n for n in range(len(v)) if v[n] > -np.inf]
    return sorted(ids, key=lambda n: (-v[n], n))


def kept_set(v, topk=0, topp=0.0):
    """-> (the kept ids as a sorted list, the mass before every position of order(v): the sums the top-p decision compares with P)."""
    o = order(v)
    before = np.concatenate([[0.0], np.cumsum(np.exp(np.asarray([v[n] for n in o], dtype=np.float64)))])[:len(o)]
    if topk > 0:
        o = o[:topk]
    elif topp > 0:
        o = [n for n, m in zip(o, before) if m < topp]
    return sorted(o), before


def topp_decided(before, topp, tau):
    """Is every prefix mass of the row further than tau from P?  Then any arithmetic within tau takes the same kept set."""
    return bool(np.all(np.abs(np.asarray(before) - topp) > tau))


def cdf(v, kept):
    """Cumulative kept mass in ascending id order: (ids, inclusive sums), float64."""
    ids = sorted(kept)
    return ids, np.cumsum(np.exp(np.asarray([v[n] for n in ids], dtype=np.float64)))


def draw(v, kept, u):
    """The first kept id, in ascending id order, whose cumulative kept mass exceeds u * Z; </s>-free: None when nothing is kept."""
    ids, c = cdf(v, kept)
    if not ids:
        return None
    i = int(np.searchsorted(c, u * c[-1], side="right"))
    return ids[min(i, len(ids) - 1)]


def draw_interval(v, kept, token):
    """[cdf(token - 1), cdf(token)] of a kept token, and Z."""
    ids, c = cdf(v, kept)
    i = ids.index(int(token))
    return (float(c[i - 1]) if i else 0.0), float(c[i]), float(c[-1])


def sample_chain(step_values, seed, key, j, eos=2, topk=0, topp=0.0, first_step=0):
    """An ancestral chain over a callable step_values(tokens so far) -> v: draws until </s>.  -> (tokens, positional scores)."""
    toks, pos, step = [], [], first_step
    while True:
        v = step_values(toks)
        kept, _ = kept_set(v, topk, topp)
        t = draw(v, kept, uniform(seed, key, step, j))
        t = eos if t is None else t
        toks.append(t)
        pos.append(float(v[t]))
        if t == eos:
            return toks, pos
        step += 1
