"""Words with time spans from the two searches that can place them in source time.

CTC: words with time spans and confidences from a scored CTC greedy search (HipModel.ctc_greedy(want_scores=True),
batch_ctc_greedy(return_scores=True), StreamPool.ctc_both() of a pool with scores): the collapsed subword tokens, the first and last
encoder frame of each token's run, and the summed log-probability of the run.

MT: the words of the first-pass text decoder's tokens (what the S2TT agent prints and the S2ST path speaks), placed by the arg-max of
the decoder's head-averaged cross-attention (BatchMixin.batch_mt_attention) -- :func:`words_from_attention`.

Host-side glue: no device work here.
"""
import math
from typing import List, NamedTuple, Optional, Sequence

WORD_START = "▁"      # SentencePiece's word-boundary mark
FRAME_MS = 40              # one encoder output row: 4 fbank frames of 10 ms


class Word(NamedTuple):
    text: str               # the word's subwords joined, boundary mark removed
    start_ms: int           # start of its first subword's first frame
    end_ms: int             # end of its last subword's last frame
    confidence: float       # geometric mean of the frame posteriors of its runs, in (0, 1]; NaN if a frame's row held a NaN
    stable: Optional[bool]  # the word cannot change any more (None: the caller does not know which rows are final)


class CtcDetails(NamedTuple):
    source_words: List[Word]    # head 0: the source text (ASR)
    target_words: List[Word]    # head 1: the target text, aligned to SOURCE time


def words_from_ctc(tokens: Sequence[int], index: Sequence[int], last: Sequence[int], tok_lprob: Sequence[float], symbols,
                   frame_ms: int = FRAME_MS, n_final: Optional[int] = None, finished: bool = False, t0_ms: int = 0) -> List[Word]:
    """Group collapsed CTC tokens into words.  `symbols[t]` is token t's subword string.  A word starts at a subword that begins
    with the boundary mark; a leading subword without it starts the first word.  start_ms = t0_ms + index[first] * frame_ms,
    end_ms = t0_ms + (last[last subword] + 1) * frame_ms, confidence = exp(sum tok_lprob / frames in its runs).
    stable: `finished`, or a LATER word starts at a frame below `n_final` -- then every row of this word's runs, and the row that
    ended its last run, is final, and a final row's arg-max is never recomputed.  n_final None and not finished: stable is None."""
    n = len(tokens)
    if not (len(index) == len(last) == len(tok_lprob) == n):
        raise ValueError("tokens, index, last and tok_lprob must have one entry per collapsed token")
    groups: List[List[int]] = []
    for j in range(n):
        if not groups or str(symbols[int(tokens[j])]).startswith(WORD_START):
            groups.append([])
        groups[-1].append(j)
    words = []
    for k, g in enumerate(groups):
        text = "".join(str(symbols[int(tokens[j])]) for j in g).replace(WORD_START, "")
        frames = sum(int(last[j]) - int(index[j]) + 1 for j in g)
        lp = math.fsum(float(tok_lprob[j]) for j in g)
        conf = math.exp(lp / frames) if frames > 0 and lp == lp else float("nan")
        if finished:
            stable = True
        elif n_final is None:
            stable = None
        else:
            stable = k + 1 < len(groups) and int(index[groups[k + 1][0]]) < int(n_final)
        words.append(Word(text, int(t0_ms) + int(index[g[0]]) * int(frame_ms), int(t0_ms) + (int(last[g[-1]]) + 1) * int(frame_ms),
                          conf, stable))
    return words


class AlignedWord(NamedTuple):
    text: str               # the word's subwords joined, boundary mark removed
    start_ms: int           # start of the earliest source frame a subword of the word peaks at
    end_ms: int             # end of the latest one
    focus: float            # mean over its subwords of the attention probability at the peak, in (0, 1]


def words_from_attention(tokens: Sequence[int], peak: Sequence[int], peak_prob: Sequence[float], symbols, frame_ms: int = FRAME_MS,
                         t0_ms: int = 0, eos: Optional[int] = None) -> List[AlignedWord]:
    """Group MT tokens into words placed in source time by the cross-attention.  peak[p] / peak_prob[p]: the arg-max source frame of
    the decoder position that predicted tokens[p], and the head-averaged probability there.  Grouping as :func:`words_from_ctc`;
    ``</s>`` tokens (id `eos`, or the symbol "</s>" when eos is None) are dropped.  start_ms = t0_ms + min(peak) * frame_ms and
    end_ms = t0_ms + (max(peak) + 1) * frame_ms over the word's subwords, focus = the mean of peak_prob over them."""
    n = len(tokens)
    if not (len(peak) == len(peak_prob) == n):
        raise ValueError("tokens, peak and peak_prob must have one entry per token")
    groups: List[List[int]] = []
    for j in range(n):
        t = int(tokens[j])
        if (t == int(eos)) if eos is not None else (str(symbols[t]) == "</s>"):
            continue
        if not groups or str(symbols[t]).startswith(WORD_START):
            groups.append([])
        groups[-1].append(j)
    words = []
    for g in groups:
        text = "".join(str(symbols[int(tokens[j])]) for j in g).replace(WORD_START, "")
        pk = [int(peak[j]) for j in g]
        words.append(AlignedWord(text, int(t0_ms) + min(pk) * int(frame_ms), int(t0_ms) + (max(pk) + 1) * int(frame_ms),
                                 math.fsum(float(peak_prob[j]) for j in g) / len(g)))
    return words


def details_from_hyps(src_hyp: dict, tgt_hyp: dict, src_symbols, tgt_symbols, n_final: Optional[int] = None, finished: bool = False,
                      t0_ms: int = 0) -> CtcDetails:
    """CtcDetails from the two hypotheses of CTCDecoder.generate(..., want_scores=True) (the agents' --word-details)."""
    def one(h, sym):
        return words_from_ctc(h["tokens"].tolist(), h["index"], h["last"], h["token_scores"].tolist(), sym, n_final=n_final,
                              finished=finished, t0_ms=t0_ms)
    return CtcDetails(one(src_hyp, src_symbols), one(tgt_hyp, tgt_symbols))
