"""Lexically constrained beam search restated in Python (the rule: include/streamspeech_hip.h at ss_batch_mt_beam_cons).
Written from the rule, not from the kernels: the tests hold csrc/beam_kernels.hip against this file, and this file against the reference's
LexicallyConstrainedBeamSearch through the per-step traces of tests/golden/mt_constraints.json (tests/make_golden_mt_constraints.py).

Plain Python lists and numpy float32 scalars; nothing here is fast."""
import numpy as np

NEG_INF = np.float32(-np.inf)


class Constraints:
    """The phrases of one utterance: seq, end markers, C and U (distinct ids, the reference's num_constraint_tokens)."""

    def __init__(self, phrases):
        self.phrases = [[int(t) for t in p] for p in (phrases or [])]
        assert all(self.phrases), "an empty phrase"
        self.seq = [t for p in self.phrases for t in p]
        self.end = [i == len(p) - 1 for p in self.phrases for i in range(len(p))]
        self.C = len(self.seq)
        self.U = len(set(self.seq))

    def finished(self, state):
        return state + 1 == self.C

    def advance(self, state, tok):
        if self.finished(state):
            return state
        if self.seq[state + 1] == tok:
            return state + 1
        if self.end[state]:            # state == -1 reads end[-1], the last element, always set -- as the reference does
            return state
        if tok == self.seq[0]:
            return 0
        return -1

    def next_tokens(self, state, descending=False):
        toks = set()
        if state > 0:
            toks.add(self.seq[0])
        if not self.finished(state):
            toks.add(self.seq[state + 1])
        return sorted(toks, reverse=descending)


def parse_packed(row):
    """One row of fairseq's packed constraint tensor (pack_constraints: count, then each phrase followed by a 0) -> phrases."""
    row = [int(x) for x in row]
    phrases, off = [], 1
    for _ in range(row[0]):
        where = row.index(0, off)
        phrases.append(row[off:where])
        off = where + 1
    return phrases


def candidates(cons, rows, states, k, step, descending=False):
    """Step 2 of the rule.  rows [k][V] float32: the rows' scores after step 1 and with the cumulative score added.
    -> [(score, tok, beam)] in list order."""
    rows = np.asarray(rows, np.float32)
    nrow = 1 if step == 0 else k
    V = rows.shape[1]
    flat = rows[:nrow].reshape(-1)
    order = sorted(range(flat.size), key=lambda i: (-float(flat[i]), i))      # score, then flattened index
    out = [(np.float32(flat[i]), i % V, i // V) for i in order[:2 * k]]
    if step > 0:
        for j in range(k):
            best = 0
            for n in range(1, V):
                if rows[j, n] > rows[j, best]:
                    best = n
            out.append((np.float32(rows[j, best]), best, j))
    for j in range(nrow):
        for tok in cons.next_tokens(int(states[j]), descending):
            out.append((np.float32(rows[j, tok]), tok, j))
    return out


def select_from(cons, cands, states, k):
    """Steps 3 - 8 on a candidate list [(score, tok, beam)] -> the 2k selected (score, tok, beam, new_state) in order."""
    items = []
    for pos, (s, tok, beam) in enumerate(cands):
        ns = cons.advance(int(states[beam]), int(tok))
        key = np.float32(np.float32((cons.U - (ns + 1)) * -100) + np.float32(s))
        items.append((key, pos, np.float32(s), int(tok), int(beam), ns))
    # key descending, ties by list position (-inf keys compare equal)
    items.sort(key=lambda it: (-float(it[0]), it[1]))
    seen, uniq = set(), []
    for it in items:
        if (it[4], it[3]) not in seen:
            seen.add((it[4], it[3]))
            uniq.append(it)
    in_bank = {}
    striped = []
    for it in uniq:
        r = in_bank.get(it[5], 0)
        in_bank[it[5]] = r + 1
        striped.append((r, -it[5], it))
    striped.sort(key=lambda x: (x[0], x[1]))
    return [(it[2], it[3], it[4], it[5]) for _, _, it in striped[:2 * k]]


def select(cons, lprobs, cum, states, k, step, eos, descending=False):
    """Steps 1 - 8 for one utterance and one step.  lprobs [k][V] float32 masked log-probabilities before step 1 and before the
    cumulative scores cum [k] are added.  -> the 2k selected (score, tok, beam, new_state)."""
    rows = np.array(lprobs, np.float32, copy=True)
    nrow = 1 if step == 0 else k
    if step > 0:
        for j in range(nrow):
            if not cons.finished(int(states[j])):
                rows[j, eos] = NEG_INF
            rows[j] = rows[j] + np.float32(cum[j])
    return select_from(cons, candidates(cons, rows, states, k, step, descending), states, k)


def contains_in_order(tokens, phrases):
    """The position of each phrase in tokens, matched left to right, one after the other; None where one is missing."""
    tokens = [int(t) for t in tokens]
    out, start = [], 0
    for p in phrases:
        p = [int(t) for t in p]
        hit = next((i for i in range(start, len(tokens) - len(p) + 1) if tokens[i:i + len(p)] == p), None)
        out.append(hit)
        if hit is None:
            return out + [None] * (len(phrases) - len(out))
        start = hit + len(p)
    return out
