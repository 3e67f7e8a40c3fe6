"""Words with time spans from the two searches that can place them in source time.

CTC: words with time spans and confidences from a scored CTC greedy search (HipModel.ctc_greedy(want_scores=True),
batch_ctc_greedy(return_scores=True), StreamPool.ctc_both() of a pool with scores): the collapsed subword tokens, the first and last
encoder frame of each token's run, and the summed log-probability of the run.

MT: the words of the first-pass text decoder's tokens (what the S2TT agent prints and the S2ST path speaks), placed by the arg-max of
the decoder's head-averaged cross-attention (BatchMixin.batch_mt_attention) -- :func:`words_from_attention`.

Spoken: where each word of the text decoder's tokens lies in the OUTPUT speech -- :func:`spoken_from_segments` over the unit spans
of the writes (HipModel.batch_unit_spans: the unit decoder upsamples every decoder state into ctc_upsample CTC positions, the
duration predictor gives every unit whole 20-ms frames, so the times are exact integers).

Scored: the words of a GIVEN text with the log-probabilities the text decoder gives its pieces (HipModel.batch_mt_score) --
:func:`words_from_scores`.

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


class ScoredWord(NamedTuple):
    text: str               # the word's subwords joined, boundary mark removed
    pieces: int             # its subwords
    lprob: float            # the sum of their log-probabilities (natural log)
    confidence: float       # exp(lprob / pieces): the geometric mean of their probabilities
    min_lprob: float        # the least likely subword's log-probability
    not_top: int            # subwords the decoder would not have chosen itself (rank > 0)


def words_from_scores(tokens: Sequence[int], positional: Sequence[float], rank: Sequence[int], symbols,
                      eos: Optional[int] = None) -> List[ScoredWord]:
    """Group the tokens of a SCORED text (HipModel.batch_mt_score: positional[p] the natural-log probability of tokens[p], rank[p]
    its rank among the vocabulary) into words.  Grouping and the ``</s>`` rule as :func:`words_from_attention`."""
    n = len(tokens)
    if not (len(positional) == len(rank) == n):
        raise ValueError("tokens, positional and rank must have one entry per token")
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
        lps = [float(positional[j]) for j in g]
        lp = math.fsum(lps)
        conf = math.exp(lp / len(g)) if lp == lp else float("nan")
        words.append(ScoredWord(text, len(g), lp, conf, min(lps), sum(1 for j in g if int(rank[j]) > 0)))
    return words


UNIT_FRAME_MS = 20        # one vocoder frame: 320 samples at 16 kHz


class SpokenWord(NamedTuple):
    text: str               # the word's subwords joined, boundary mark removed
    start_ms: int           # where its first unit starts on the clock of the emitted speech
    end_ms: int             # where its last unit ends
    n_units: int            # the units its tokens' states were given (0: nothing of the speech belongs to it)


class Spoken(NamedTuple):
    words: List[SpokenWord]
    tail_ms: int            # speech of states that are not a committed token: the </s> state, a trailing <pad> state, a pending state
    total_ms: int           # all speech emitted for the utterance: the words' segments and the tail add up to it


def segments_from_spans(spans, clock_ms: int, n_seen: int = 0, frame_ms: int = UNIT_FRAME_MS):
    """The segments one write adds: spans = the write's int32 [n, 4] unit spans {first_unit, n_units, start_frame, n_frames} (state s
    is the decoder position that predicted token s), clock_ms = the speech emitted before the write.  -> [(state, start_ms, end_ms,
    n_units)] for every state that was given a new unit, plus the zero-length segment of every state from n_seen on (the states no
    earlier write saw), which marks where a token without units lies."""
    out = []
    clock_ms, frame_ms = int(clock_ms), int(frame_ms)
    for s, (_, k, f0, nf) in enumerate(spans.tolist() if hasattr(spans, "tolist") else spans):
        if k > 0 or s >= n_seen:
            t0 = clock_ms + f0 * frame_ms
            out.append((s, t0, t0 + nf * frame_ms, k))
    return out


def spoken_from_segments(tokens: Sequence[int], segments, symbols, eos: Optional[int] = None) -> Spoken:
    """Words of the committed target tokens placed in the output speech.  segments: (token_index, start_ms, end_ms, n_units) in the
    order the writes added them, times on the clock of the emitted speech; token_index s is the decoder state that predicted
    tokens[s].  Grouping as :func:`words_from_attention` (the boundary mark starts a word, ``</s>`` is dropped).  A word's start_ms is
    the earliest start over its segments that hold units, its end_ms their latest end, n_units their sum; a word none of whose
    tokens received a unit is a zero-length word at the clock value of its first token's state (the first segment recorded for it).
    Speech of an index that is not a committed token -- the state that predicts ``</s>`` or a not-yet-committed token, a trailing
    <pad> state -- is no word: its milliseconds add up in tail_ms.  Segments are kept by index, so once such an index is a committed
    token its earlier segments count for that token.  total_ms = the milliseconds of all segments."""
    n = len(tokens)

    def is_eos(t):
        return (t == int(eos)) if eos is not None else (str(symbols[t]) == "</s>")

    by_tok = {}
    tail = total = 0
    for idx, t0, t1, k in segments:
        idx, t0, t1, k = int(idx), int(t0), int(t1), int(k)
        if t1 < t0 or k < 0:
            raise ValueError("a segment ends before it starts")
        total += t1 - t0
        if 0 <= idx < n and not is_eos(int(tokens[idx])):
            by_tok.setdefault(idx, []).append((t0, t1, k))
        else:
            tail += t1 - t0
    groups: List[List[int]] = []
    for j in range(n):
        t = int(tokens[j])
        if is_eos(t):
            continue
        if not groups or str(symbols[t]).startswith(WORD_START):
            groups.append([])
        groups[-1].append(j)
    words, clock = [], 0
    for g in groups:
        text = "".join(str(symbols[int(tokens[j])]) for j in g).replace(WORD_START, "")
        segs = [sg for j in g for sg in by_tok.get(j, ()) if sg[2] > 0]
        if segs:
            start, end = min(sg[0] for sg in segs), max(sg[1] for sg in segs)
        else:
            first = by_tok.get(g[0]) or [sg for j in g for sg in by_tok.get(j, ())]
            start = end = first[0][0] if first else clock
        clock = max(clock, end)
        words.append(SpokenWord(text, start, end, sum(sg[2] for sg in segs)))
    return Spoken(words, tail, total)


def details_from_hyps(src_hyp: dict, tgt_hyp: dict, src_symbols, tgt_symbols, n_final: Optional[int] = None, finished: bool = False,
                      t0_ms: int = 0) -> CtcDetails:
    """CtcDetails from the two hypotheses of CTCDecoder.generate(..., want_scores=True) (the agents' --word-details)."""
    def one(h, sym):
        return words_from_ctc(h["tokens"].tolist(), h["index"], h["last"], h["token_scores"].tolist(), sym, n_final=n_final,
                              finished=finished, t0_ms=t0_ms)
    return CtcDetails(one(src_hyp, src_symbols), one(tgt_hyp, tgt_symbols))
