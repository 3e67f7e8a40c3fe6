"""Reference of the token score kernel (csrc/mt_score.hip, ss_op_mt_token_scores), written from its definition, and the op cases
the CPU and GPU tests share.

Per float32 logits row x[0:V] and target tk:
  * target value  log_softmax(x)[tk] and best value max_n log_softmax(x)[n], in float64 (`score_ref`);
  * arg-max: the LOWEST index that holds the maximum; rank: #{n: x[n] > x[tk]} + #{n < tk: x[n] == x[tk]} -- exact integer work on
    the float32 logits (`scan_row` states both as explicit loops; `score_ref` is the same rule on whole arrays);
  * tk < 0: the row answers nothing (`skip`);
  * a NaN or +inf column, or a row of -inf only: NaN, NaN, -1, -1 (the values would be NaN: NaN, inf - inf, -inf - -inf);
  * -inf columns are ordinary: they add 0 to the sum; a -inf target answers -inf and its rank by the rule.
`score_f32` is the float32 twin in the kernel's promised summation order: f32 maximum; thread t of 256 adds exp(x - mx) over columns
t, t + 256, ... ascending; a xor-shuffle tree over each wave of 64; (s0 + s1) + (s2 + s3); one log; (x - mx) - lse.

TOL = 2e-5 is the bound the suite holds this arithmetic to at <= 8193 terms (tests/test_ctc_scores_gpu.py).  It needs |value| < 256:
a float32 in [256, 512) is spaced 3.05e-5, so two roundings there could reach 3e-5 whatever the kernel.  The cases keep to that: the
"scaled by 40" logits are 40 x a normal clamped to [-3, 3] (spread <= 240, lse <= log 8193 = 9.1), the shifts move x and the
maximum alike.
"""
import numpy as np

TOL = 2e-5
WIDTHS = (1, 63, 64, 65, 255, 256, 257, 1005, 6000, 8192, 8193)
REG_MAX_V = 8192                       # widest row the kernel holds in registers; wider rows take the strided form
# the utterances of the model-level GPU tests: (synth_fbank seed, frames), encoded with 8-frame chunks; the greedy hypotheses of
# SEARCH_MAX_LEN tokens are the texts of the consistency test (tests/test_mt_score_cpu.py checks them on the CPU oracle)
SEARCH_UTTS = tuple((500 + i, 60 + 23 * i) for i in range(4))
SEARCH_MAX_LEN = 12


def scan_row(x, tk):
    """(arg-max, rank) of one row by explicit scan and count -- the definition, column by column."""
    best, arg, rank = None, -1, 0
    for n in range(len(x)):
        if best is None or x[n] > best:            # strictly greater: the first maximum stays
            best, arg = x[n], n
        if x[n] > x[tk] or (x[n] == x[tk] and n < tk):
            rank += 1
    return arg, rank


def _bad_rows(x):
    return np.isnan(x).any(1) | np.isposinf(x).any(1) | np.isneginf(x).all(1)


def score_ref(x, tgt):
    """float32 logits [rows, V], targets [rows] -> dict of float64 `target`, `best` [rows], int64 `argmax`, `rank` [rows], bool
    `skip` (tk < 0: nothing is answered; its entries here are meaningless) and `bad` (NaN, NaN, -1, -1)."""
    assert x.dtype == np.float32 and x.ndim == 2
    rows, V = x.shape
    tgt = np.asarray(tgt, dtype=np.int64)
    skip = tgt < 0
    tk = np.where(skip, 0, tgt)
    bad = _bad_rows(x)
    x64 = np.where(bad[:, None], 0.0, x.astype(np.float64))
    mx = x64.max(1)
    with np.errstate(divide="ignore"):
        lse = np.log(np.exp(x64 - mx[:, None]).sum(1))
    xt = x64[np.arange(rows), tk]
    target = (xt - mx) - lse
    best = -lse
    cols = np.arange(V)[None, :]
    argmax = np.where(x64 == mx[:, None], cols, V).min(1)
    rank = (x64 > xt[:, None]).sum(1) + ((x64 == xt[:, None]) & (cols < tk[:, None])).sum(1)
    target[bad], best[bad], argmax[bad], rank[bad] = np.nan, np.nan, -1, -1
    return {"target": target, "best": best, "argmax": argmax.astype(np.int64), "rank": rank.astype(np.int64), "skip": skip, "bad": bad}


def score_f32(x, tgt):
    """The float32 twin in the kernel's summation order -> (target, best) float32 [rows] (NaN on bad rows)."""
    assert x.dtype == np.float32
    rows, V = x.shape
    tk = np.where(np.asarray(tgt) < 0, 0, np.asarray(tgt)).astype(np.int64)
    per = -(-V // 256)
    xp = np.full((rows, per * 256), -np.inf, dtype=np.float32)
    xp[:, :V] = x
    with np.errstate(invalid="ignore", divide="ignore"):
        mx = np.fmax.reduce(xp, axis=1).astype(np.float32)                     # fmaxf skips a NaN
        e = np.exp((xp - mx[:, None]).astype(np.float32)).astype(np.float32).reshape(rows, per, 256)
        acc = np.zeros((rows, 256), dtype=np.float32)
        for i in range(per):                                                    # a thread's columns, ascending
            acc = (acc + e[:, i, :]).astype(np.float32)
        w = acc.reshape(rows, 4, 64)
        lanes = np.arange(64)
        for o in (32, 16, 8, 4, 2, 1):                                          # wave_sum: v += shfl_xor(v, o)
            w = (w + w[:, :, lanes ^ o]).astype(np.float32)
        s = w[:, :, 0]
        tot = ((s[:, 0] + s[:, 1]).astype(np.float32) + (s[:, 2] + s[:, 3]).astype(np.float32)).astype(np.float32)
        lse = np.log(tot).astype(np.float32)
        xt = x[np.arange(rows), tk]
        target = ((xt - mx).astype(np.float32) - lse).astype(np.float32)
        best = ((mx - mx).astype(np.float32) - lse).astype(np.float32)
    bad = np.isnan(tot)
    target[bad], best[bad] = np.nan, np.nan
    return target, best


# -------------------------------------------------------------------------------------------------
# the shared op cases
# -------------------------------------------------------------------------------------------------
def op_cases():
    """name -> {V, rows, ld, scale, shift, special}.  Plain rows: row 0 targets column 0, row 1 column V - 1, row 2 the arg-max, the
    others a seeded column.  `special` rows replace rows 3.. (where the row count allows) -- see case_data."""
    c = {}
    for V in WIDTHS:
        c[f"v{V}"] = dict(V=V, rows=5, ld=V, scale=1.0, shift=0.0, special=())
    c["rows1"] = dict(V=1005, rows=1, ld=1005, scale=1.0, shift=0.0, special=())
    c["rows300"] = dict(V=257, rows=300, ld=257, scale=1.0, shift=0.0, special=())
    c["rows70000"] = dict(V=65, rows=70000, ld=65, scale=1.0, shift=0.0, special=())          # past a 16-bit grid extent
    for V in (1005, 6000, 8193):
        c[f"ties{V}"] = dict(V=V, rows=8, ld=V, scale=1.0, shift=0.0, special=("tie_max", "tie_mid"))
        c[f"edge{V}"] = dict(V=V, rows=15, ld=V, scale=1.0, shift=0.0,
                             special=("neginf_cols", "neginf_target", "nan", "skip", "all_neginf", "posinf"))
    c["scale40"] = dict(V=6000, rows=6, ld=6000, scale=40.0, shift=0.0, special=("tie_max",))
    c["shift+80"] = dict(V=6000, rows=6, ld=6000, scale=1.0, shift=80.0, special=("tie_mid",))
    c["shift-80"] = dict(V=1005, rows=6, ld=1005, scale=1.0, shift=-80.0, special=("neginf_cols",))
    c["ld"] = dict(V=1005, rows=7, ld=1013, scale=1.0, shift=0.0, special=("tie_max", "nan", "skip"))
    c["ld8193"] = dict(V=8193, rows=5, ld=8200, scale=1.0, shift=0.0, special=("tie_max",))
    return c


def case_data(c, name=""):
    """-> (logits float32 [rows, ld], targets int32 [rows]).  Columns V .. ld - 1 hold NaN: no kernel may read them.  Special rows
    (from row 3 on, each followed by a plain row while rows last, so a NaN or skipped row stands between good rows):
      tie_max        two equal maxima at columns a < b, target b: rank 1, arg-max a
      tie_mid        the target's value also at a lower and a higher column, none the maximum
      neginf_cols    every third column -inf
      neginf_target  the target column (and two others) -inf
      nan            one NaN column
      skip           target -1
      all_neginf     every column -inf
      posinf         one +inf column
    """
    V, rows, ld = c["V"], c["rows"], c["ld"]
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name or repr(sorted(c.items())))) % (2 ** 31)
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, V))
    if c["scale"] != 1.0:
        x = np.clip(x, -3.0, 3.0)
    x = (x * c["scale"] + c["shift"]).astype(np.float32)
    tgt = rng.integers(0, V, size=rows).astype(np.int32)
    tgt[0] = 0
    if rows > 1:
        tgt[1] = V - 1
    if rows > 2:
        tgt[2] = int(x[2].argmax())
    r = 3
    for kind in c["special"]:
        if r >= rows:
            break
        if kind == "tie_max" and V >= 3:
            a, b = sorted(rng.choice(V, 2, replace=False))
            x[r, a] = x[r, b] = np.float32(x[r].max() + 1.0)
            tgt[r] = b
        elif kind == "tie_mid" and V >= 5:
            a, t, b = sorted(rng.choice(V, 3, replace=False))
            x[r, a] = x[r, b] = x[r, t] = np.float32(x[r].mean())       # a middling value no other column holds
            tgt[r] = t
        elif kind == "neginf_cols":
            x[r, ::3] = -np.inf
            tgt[r] = 1 if V > 1 else 0
        elif kind == "neginf_target":
            t = int(rng.integers(1, V - 1))
            x[r, [0, t, V - 1]] = -np.inf
            tgt[r] = t
        elif kind == "nan":
            x[r, int(rng.integers(0, V))] = np.nan
        elif kind == "skip":
            tgt[r] = -1
        elif kind == "all_neginf":
            x[r, :] = -np.inf
        elif kind == "posinf":
            x[r, int(rng.integers(0, V))] = np.inf
        r += 2
    full = np.full((rows, ld), np.nan, dtype=np.float32)
    full[:, :V] = x
    return full, tgt
