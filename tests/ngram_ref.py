"""The n-gram scoring rule as a dict-of-tuples float64 scorer, written from the ARPA definition -- p(c | h) is the n-gram (h, c)'s
value when the model holds it, else the back-off weight of h (when the model holds h) plus p(c | h minus its first token), the
longest context first -- and NOT from the library's state machine (csrc/ngram_lm.hpp).  The tests hold ss_ngram_score_host and
ss_op_ngram_score to exactly these float64 values, and the library's states to `state`: the longest suffix of the history, at
most order - 1 tokens long, that the model holds.

The two choices the rule makes beyond ARPA are restated here: a token without a unigram scores as <unk> when the model has that
unigram, and the history is then (<unk>,) alone (the library goes to the state of the unk unigram); without one it scores
oov_logp and the history is empty."""
import numpy as np


class Ref:
    def __init__(self, a):
        """a: the arrays ss_ngram_lm_create takes (tests/arpa_writer.py:arrays, streamspeech_amd.ngram.read_arpa)."""
        self.order, self.bos, self.eos, self.unk, self.oov = a["order"], a["bos"], a["eos"], a["unk"], float(np.float32(a["oov_logp"]))
        self.logp, self.bo, self.entry = {}, {}, {(): 0}
        off = e = 0
        tok = np.asarray(a["tokens"]).tolist()
        for k, n in enumerate(a["counts"], 1):
            for _ in range(n):
                g = tuple(tok[off:off + k])
                self.logp[g] = float(np.float32(a["logp"][e]))
                self.bo[g] = float(np.float32(a["backoff"][e]))
                e += 1
                off += k
                self.entry[g] = e                              # the library numbers its entries in input order, the root 0
        self.gram_of = {v: k for k, v in self.entry.items()}

    def start(self):
        return (self.bos,) if self.bos >= 0 and (self.bos,) in self.logp else ()

    def lp(self, hist, c):
        """-> (float64 log p(c | hist), the history after c)."""
        h = tuple(hist[max(0, len(hist) - (self.order - 1)):]) if self.order > 1 else ()
        acc = 0.0
        while True:
            if h + (c,) in self.logp:
                return acc + self.logp[h + (c,)], tuple(hist) + (c,)
            if not h:
                break
            if h in self.bo:
                acc += self.bo[h]
            h = h[1:]
        if self.unk >= 0 and (self.unk,) in self.logp:
            return acc + self.logp[(self.unk,)], (self.unk,)
        return acc + self.oov, ()

    def state(self, hist):
        """The longest suffix of hist, at most order - 1 tokens, that the model holds (() is the root)."""
        h = tuple(hist[max(0, len(hist) - (self.order - 1)):]) if self.order > 1 else ()
        while h and h not in self.logp:
            h = h[1:]
        return h

    def score(self, seq, eos=True):
        """-> (lp per token [+ eos], state per position) from the start state."""
        hist, out, states = self.start(), [], []
        for c in list(seq) + ([self.eos] if eos else []):
            v, hist = self.lp(hist, c)
            out.append(v)
            states.append(self.state(hist))
        return out, states
