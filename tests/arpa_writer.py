"""A seeded generator of valid ARPA text over a given symbol list, for the n-gram tests (tests/test_ngram_*.py,
tests/test_ctc_beam_lm_*.py): no LM toolkit is needed.  The values are seeded random log10 numbers with four decimals, so the
text holds them exactly as generated; they are not normalised (the library takes values as given).

generate -> grams {order: [(symbols tuple, log10 p, log10 back-off or None)]}, n-grams of every order unique, every n-gram's
context (itself minus its last symbol) an n-gram of the order below, the highest order without back-off fields.  text(grams) is
the ARPA file; arrays(grams, index, ...) the arrays ss_ngram_lm_create takes, with the values read back from the text's own
decimals as streamspeech_amd.ngram.read_arpa converts them."""
import numpy as np

from streamspeech_amd.ngram import to_ln

BOS, EOS, UNK = "<s>", "</s>", "<unk>"


def generate(symbols, order, counts, seed, unk=False, drop_suffix=False, skip_unigrams=(), logp_range=(-3.0, -0.1)):
    """symbols: the ordinary symbols.  counts[k - 1]: the n-grams of order k wanted (order 1: every symbol not in skip_unigrams,
    <s>, </s> and with `unk` <unk>, whatever counts[0] says; higher orders: up to that many).  drop_suffix: afterwards removes
    n-grams that are the proper suffix of another n-gram and the context of none -- the suffix links must then skip them; the
    removed n-grams are returned as the second value.  logp_range: the log10 range the n-grams' values are drawn from."""
    rng = np.random.default_rng(seed)
    val = lambda lo, hi: round(float(rng.uniform(lo, hi)), 4)  # noqa: E731
    last = order == 1
    uni = [BOS] + [s for s in symbols if s not in skip_unigrams] + [EOS] + ([UNK] if unk else [])
    grams = {1: [((s,), -99.0 if s == BOS else val(*logp_range), None if last else val(-1.0, 0.0)) for s in uni]}
    words = [s for s in uni if s != BOS]
    for k in range(2, order + 1):
        ctxs = [g[0] for g in grams[k - 1] if g[0][-1] != EOS]
        seen, out = set(), []
        tries = 0
        while ctxs and len(out) < counts[k - 1] and tries < 50 * counts[k - 1] + 100:
            tries += 1
            g = ctxs[int(rng.integers(len(ctxs)))] + (words[int(rng.integers(len(words)))],)
            if g in seen:
                continue
            seen.add(g)
            out.append((g, val(*logp_range), None if k == order else val(-1.0, 0.0)))
        grams[k] = out
    removed = []
    if drop_suffix:
        every = {g[0] for k in grams for g in grams[k]}
        contexts = {g[0][:-1] for k in grams for g in grams[k]}
        for k in range(order, 1, -1):
            for g in grams[k]:
                suf = g[0][1:]
                if suf in every and suf not in contexts and suf[0] not in (BOS, UNK) and suf != (EOS,) and len(removed) < 8:
                    removed.append(suf)
                    every.discard(suf)
        for k in grams:
            grams[k] = [g for g in grams[k] if g[0] not in removed]
    return (grams, removed) if drop_suffix else grams


def text(grams):
    order = max(grams)
    out = ["", "\\data\\"] + [f"ngram {k}={len(grams[k])}" for k in range(1, order + 1)] + [""]
    for k in range(1, order + 1):
        out.append(f"\\{k}-grams:")
        for sym, p, bo in grams[k]:
            out.append(f"{p:.4f}\t{' '.join(sym)}" + ("" if bo is None else f"\t{bo:.4f}"))
        out.append("")
    return "\n".join(out + ["\\end\\", ""])


def arrays(grams, index, V, bos=0, eos=2, unk=3, oov_logp=-20.0):
    """index: symbol -> id (a dict, or a Dictionary's index).  Values as read_arpa gives them for text(grams)."""
    ix = index.__getitem__ if isinstance(index, dict) else index
    order = max(grams)
    rows = [g for k in range(1, order + 1) for g in grams[k]]
    return {"order": order, "counts": [len(grams[k]) for k in range(1, order + 1)],
            "tokens": np.asarray([ix(s) for g in rows for s in g[0]], np.int32),
            "logp": np.asarray([to_ln(f"{g[1]:.4f}") for g in rows], np.float32),
            "backoff": np.asarray([to_ln(f"{g[2]:.4f}") if g[2] is not None else 0.0 for g in rows], np.float32),
            "V": V, "bos": bos, "eos": eos, "unk": unk, "oov_logp": oov_logp, "dropped": 0}


def int_symbols(V, first=4):
    """Symbols "4" .. str(V - 1) and the index that maps them, and <s> </s> <unk>, onto the ids of a fairseq dictionary."""
    index = {BOS: 0, "<pad>": 1, EOS: 2, UNK: 3}
    syms = [str(i) for i in range(first, V)]
    index.update({s: int(s) for s in syms})
    return syms, index
