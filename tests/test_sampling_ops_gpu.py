"""The sampling kernels at op level (csrc/beam_sample.hip: sample_uniform_kernel, sample_step_kernel) against the restatement of the rule in
tests/sampling_ref.py (float64).

Uniforms: the three known Philox vectors and 1024 random (seed, key, step, j), word for word.
Step kernel: V in {9, 97, 6000}, 1 to 64 rows of peaked logits (normal x 4); every row is one chain with its own step, chain index
and key.  A case holds rows below min_len, rows at max_len, the pad and unk masks (with a penalty) and, with a ban, rows whose
history repeats.  Per row:
  * u is the reference's, bit for bit;
  * the kept count: exact for top-k and for plain sampling.  For top-p with tau = V * 2^-23 (the worst-case error of a sequential
    float32 sum of V terms with total <= 1, doubled for the exponentials): the count n is one for which the mass before position
    n - 1 is < P + tau and the mass before position n is >= P - tau.  Where every prefix mass of the reference lies outside tau of P
    (the row is DECIDED) that is the reference's count and nothing else; the cases in DECIDED_CASES assert, on the CPU and before the
    device is looked at, that every one of their rows is decided.  (At V = 6000 the masses around P = 0.9 and below P = 1.0, and
    at V = 97 those below P = 1.0, are spaced closer than tau on rows of this shape whatever the seed, so those cases hold every
    row to the band instead.)
  * the drawn token t is kept and u * Z lies in [cdf(t - 1) - tau, cdf(t) + tau] of the reference;
  * the positional score is bit-equal to the row_scores entry of ss_op_beam_topk_opts on the same inputs.
Three mutants of the reference each fail on at least half the rows; two runs give the same bits; a row's result does not depend on
the rows in front of it."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import sampling_ref as SR
from tests import search_ref as BR
from tests.test_sampling_ref_cpu import PHILOX_VECTORS

pytestmark = pytest.mark.gpu

PAD, UNK, EOS = 1, 3, 2
T_STEP, C0, MIN_LEN, PEN = 2, 3, 4, 0.75
SEED = 0x9E3779B97F4A7C15


@pytest.fixture(scope="module")
def lib():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from streamspeech_amd import lib as L
    return L.load()


def S():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(np.asarray(a), dt)).cuda()


def P(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- uniforms -----------------------------------------------------------------------------------------------------------------------
def _uniforms(lib, seeds, keys, steps, js):
    n = len(seeds)
    a = [dev(np.asarray(seeds, np.uint64).view(np.int64), np.int64), dev(np.asarray(keys, np.uint64).view(np.int64), np.int64),
         dev(steps, np.int32), dev(js, np.int32)]
    u = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    w = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    assert lib.ss_op_sample_uniform(S(), n, P(a[0]), P(a[1]), P(a[2]), P(a[3]), P(u), P(w)) == 0
    return host(u), host(w).view(np.uint32)


def test_uniform_known_vectors(lib):
    seeds = [k[0] | k[1] << 32 for _, k, _ in PHILOX_VECTORS]
    keys = [c[2] | c[3] << 32 for c, _, _ in PHILOX_VECTORS]
    steps = [np.uint32(c[0]).astype(np.int32) for c, _, _ in PHILOX_VECTORS]
    js = [np.uint32(c[1]).astype(np.int32) for c, _, _ in PHILOX_VECTORS]
    u, w = _uniforms(lib, seeds, keys, steps, js)
    for i, (_, _, out) in enumerate(PHILOX_VECTORS):
        assert w[i].tolist() == out
        assert u[i] == np.float32((out[0] >> 8) * 2.0 ** -24)


def test_uniform_agrees_with_the_reference_on_random_tuples(lib):
    rng = np.random.default_rng(1)
    n = 1024
    seeds = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    keys = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    steps, js = rng.integers(0, 1024, n), rng.integers(0, 32, n)
    u, w = _uniforms(lib, seeds, keys, steps, js)
    for i in range(n):
        ref = SR.words(int(seeds[i]), int(keys[i]), int(steps[i]), int(js[i]))
        assert w[i].tolist() == ref, i
        assert float(u[i]) == SR.uniform(int(seeds[i]), int(keys[i]), int(steps[i]), int(js[i]))
    assert np.all((u >= 0) & (u < 1))


def test_uniform_refusals(lib):
    assert lib.ss_op_sample_uniform(S(), 0, None, None, None, None, None, None) == 2
    assert lib.ss_op_sample_uniform(S(), 4, None, None, None, None, None, None) == 2


# ---- the step kernel ------------------------------------------------------------------------------------------------------------------
_CASES = {}


def make_case(V, R, data_seed, ngram=0):
    """R single-chain rows at lock-step index T_STEP behind prefixes of 0 .. 3 tokens (reference step 2 .. 5): rows with step <
    MIN_LEN = 4 may not end, rows 3 and 6 of every eight (steps 5 and 4: the search refuses max_len < min_len) stand at their max_len.  Histories draw from three symbols, so with a ban
    bigrams repeat.  The logits of pad and unk are raised on a few rows so that both masks bite."""
    rng = np.random.default_rng(data_seed)
    Lc = C0 + T_STEP + 2
    npre = np.arange(R) % 4
    step = T_STEP + npre
    mxl = np.full(R, 50)
    mxl[3::8] = step[3::8]
    mxl[6::8] = step[6::8]
    row0 = np.concatenate([[0], np.cumsum(npre)])[:-1]
    sym = np.array([4, 5, 6])
    ptok = np.full(max(int(npre.sum()), 1), 4)
    tok = rng.choice(sym, (T_STEP + 1, R))
    hist = []
    for r in range(R):
        pre = [EOS] + list(rng.choice(sym, npre[r] - 1)) if npre[r] else []
        ptok[row0[r]:row0[r] + npre[r]] = pre
        if npre[r] == 0:
            tok[0, r] = EOS
        hist.append([int(x) for x in pre] + [int(tok[u, r]) for u in range(T_STEP + 1)])
        assert len(hist[r]) == step[r] + 1 and hist[r][0] == EOS
    anc = np.tile(np.arange(R)[:, None], (1, Lc))
    logits = (rng.standard_normal((R, V)) * 4).astype(np.float32)
    logits[0::5, PAD] += 6
    logits[1::5, UNK] += 6
    return dict(V=V, R=R, Lc=Lc, npre=npre, step=step, mxl=mxl, row0=row0, ptok=ptok, tok=tok, anc=anc, hist=hist, logits=logits,
                j=rng.integers(0, 32, R), keys=rng.integers(0, 2 ** 63, R, dtype=np.int64), ngram=ngram)


def ref_values(c, temp):
    """The float64 candidate values of every row, once per (case, temperature)."""
    key = ("v", id(c), temp)
    if key not in _CASES:
        _CASES[key] = [SR.row_values(c["logits"][r], temp, PAD, UNK, EOS, PEN, int(c["step"][r]), MIN_LEN, int(c["mxl"][r]),
                                     BR.banned_tokens(c["hist"][r], c["ngram"]) if c["ngram"] else ()) for r in range(c["R"])]
    return _CASES[key]


def case(V, R, ngram=0, data_seed=None):
    key = (V, R, ngram, data_seed)
    if key not in _CASES:
        _CASES[key] = make_case(V, R, 1000 * V + R + ngram if data_seed is None else data_seed, ngram)
    return _CASES[key]


def run_step(lib, c, temp, topk, topp, rows=None, seed=SEED):
    from streamspeech_amd import lib as L
    rows = list(range(c["R"])) if rows is None else rows
    n, V = len(rows), c["V"]
    # the sub-pack keeps the tables whole: a row names its history through anc, which is the identity here
    sub = lambda a: np.asarray(a)[rows]          # noqa: E731
    tok, anc = c["tok"][:, rows], np.tile(np.arange(n)[:, None], (1, c["Lc"]))
    keep = [dev(sub(c["logits"]), np.float32), dev(sub(c["mxl"]), np.int32), dev(sub(c["npre"]), np.int32), dev(tok, np.int32),
            dev(anc, np.int32), dev(c["ptok"], np.int32), dev(sub(c["row0"]), np.int32), dev(sub(c["j"]), np.int32),
            dev(sub(c["keys"]), np.int64)]
    o_tok = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    o_kept = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    o_sc = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    o_u = torch.full((n,), float("nan"), dtype=torch.float32, device="cuda")
    so = L.sample_opts(topk, topp, seed)
    rc = lib.ss_op_sample_step(S(), P(keep[0]), n, V, T_STEP, MIN_LEN, P(keep[1]), P(keep[2]), PAD, UNK, EOS, PEN, temp, c["ngram"],
                               P(keep[3]), P(keep[4]), c["Lc"], C0, P(keep[5]), P(keep[6]), P(keep[7]), P(keep[8]), C.byref(so),
                               P(o_tok), P(o_sc), P(o_u), P(o_kept))
    assert rc == 0, f"return code {rc}"
    # the beam search's own row values on the same inputs: one chain per utterance, cumulative score 0
    cand_s = torch.zeros((n, L.SS_OP_BEAM_CAND), dtype=torch.float32, device="cuda")
    cand_t = torch.zeros((n, L.SS_OP_BEAM_CAND), dtype=torch.int32, device="cuda")
    rs = torch.full((n, V), float("nan"), dtype=torch.float32, device="cuda")
    zeros_i, zeros_f = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.float32, device="cuda")
    rc = lib.ss_op_beam_topk_opts(S(), P(keep[0]), n, V, 1, T_STEP, MIN_LEN, P(keep[1]), P(keep[2]), P(zeros_i), P(zeros_f), PAD, UNK,
                                  EOS, PEN, P(cand_s), P(cand_t), temp, c["ngram"], P(keep[3]), P(keep[4]), c["Lc"], C0, P(keep[5]),
                                  P(keep[6]), P(rs))
    assert rc == 0, f"return code {rc}"
    out = dict(tok=host(o_tok), score=host(o_sc), u=host(o_u), kept=host(o_kept), row_scores=host(rs))
    del keep
    return out


def tau_of(V):
    return V * 2.0 ** -23


def topp_band(before, P_, tau):
    """The counts n a sum within tau may give: before[n - 1] < P + tau and (n == len or before[n] >= P - tau)."""
    n_lo = int(np.sum(np.asarray(before) < P_ - tau))
    n_hi = int(np.sum(np.asarray(before) < P_ + tau))
    return max(n_lo, min(1, len(before))), n_hi


def check_row(c, v, r, got, i, topk, topp, seed=SEED, shift=0, short=0, word=0):
    """Every check of row r (entry i of the outputs) -> list of failures.  shift / short / word: the mutants of the reference."""
    V, tau = c["V"], tau_of(c["V"])
    bad = []
    u = SR.uniform(seed, int(c["keys"][r]), int(c["step"][r]), int(c["j"][r]), word)
    if float(got["u"][i]) != u:
        bad.append("u")
    order = SR.order(v)
    kept, before = SR.kept_set(v, topk, topp)
    n = int(got["kept"][i])
    if topp > 0:
        lo, hi = topp_band(before, topp, tau)
        if SR.topp_decided(before, topp, tau):
            assert lo == hi == len(kept)
        lo, hi = lo - short, hi - short
        if not lo <= n <= hi:
            bad.append(f"kept {n} outside [{lo}, {hi}]")
        kept = sorted(order[:min(max(n, 0), len(order))])
    else:
        if n != len(kept) - short:
            bad.append(f"kept {n} != {len(kept) - short}")
        kept = sorted(order[:len(kept) - short]) if short else kept
    t = int(got["tok"][i])
    if t not in kept:
        return bad + [f"token {t} is not kept"]
    ids = sorted(kept)
    t_ref = t
    if shift and len(ids) > 1:                   # the mutant claims the neighbouring kept id (the one before, at the last id)
        q = ids.index(t)
        t_ref = ids[q + 1] if q + 1 < len(ids) else ids[q - 1]
    lo, hi, Z = SR.draw_interval(v, kept, t_ref)
    if not lo - tau <= float(got["u"][i]) * Z <= hi + tau:
        bad.append(f"u * Z = {float(got['u'][i]) * Z} outside [{lo}, {hi}] of token {t_ref}")
    if bits(got["score"][i:i + 1])[0] != bits(got["row_scores"][i, t:t + 1])[0]:
        bad.append("score bits")
    if abs(float(got["score"][i]) - v[t]) > 1e-5 * max(1.0, abs(v[t])):
        bad.append(f"score {got['score'][i]} vs {v[t]}")
    return bad


SETTINGS = [("topk", 1), ("topk", 5), ("topk", "V"), ("topp", 0.3), ("topp", 0.9), ("topp", 1.0), ("none", 0)]
SHAPES = [(9, 64), (97, 33), (6000, 17)]
STEP_CASES = [(V, R, 1.0, kind, x, 0) for V, R in SHAPES for kind, x in SETTINGS]
STEP_CASES += [(V, R, T, kind, x, 0) for V, R in SHAPES[1:] for T in (0.5, 1.7) for kind, x in (("topp", 0.9), ("none", 0), ("topk", 5))]
STEP_CASES += [(97, 33, 1.0, kind, x, 2) for kind, x in (("none", 0), ("topk", 5), ("topp", 0.9))] + [(6000, 1, 1.0, "topp", 0.3, 0),
                                                                                                   (6000, 1, 1.0, "none", 0, 0)]
# top-p cases every row of which is decided (asserted below before the device is looked at); the data seeds were chosen for it
DECIDED_CASES = {(9, 64, 0.3), (9, 64, 0.9), (9, 64, 1.0), (97, 33, 0.3), (97, 33, 0.9), (6000, 17, 0.3), (6000, 1, 0.3)}
DATA_SEEDS = {}


def _decided_seed(V, R, topp):
    """The first data seed (searched on the CPU, from the case's default) whose rows are all decided at every temperature used."""
    key = (V, R)
    if key in DATA_SEEDS:
        return DATA_SEEDS[key]
    tau = tau_of(V)
    want = sorted(p for (v_, r_, p) in DECIDED_CASES if (v_, r_) == key)
    for s in range(1000 * V + R, 1000 * V + R + 200):
        c = make_case(V, R, s)
        vs = [SR.row_values(c["logits"][r], 1.0, PAD, UNK, EOS, PEN, int(c["step"][r]), MIN_LEN, int(c["mxl"][r])) for r in range(R)]
        if all(SR.topp_decided(SR.kept_set(v, 0, p)[1], p, tau) for v in vs for p in want):
            DATA_SEEDS[key] = s
            return s
    raise AssertionError(f"no data seed decides every row of V={V} R={R}")


@pytest.mark.parametrize("V,R,temp,kind,x,ngram", STEP_CASES)
def test_sample_step_against_the_reference(lib, V, R, temp, kind, x, ngram):
    topk = (V if x == "V" else x) if kind == "topk" else 0
    topp = x if kind == "topp" else 0.0
    seed = _decided_seed(V, R, topp) if any((V, R) == k[:2] for k in DECIDED_CASES) and ngram == 0 else None
    c = case(V, R, ngram, seed)
    vs = ref_values(c, temp)
    n_min = sum(1 for r in range(R) if c["step"][r] < MIN_LEN and c["step"][r] < c["mxl"][r])
    n_max = sum(1 for r in range(R) if c["step"][r] >= c["mxl"][r])
    assert R < 8 or (n_min > 0 and n_max > 0)
    if (V, R, topp) in DECIDED_CASES and temp == 1.0 and ngram == 0:          # of the reference, before the device is looked at
        for r in range(R):
            assert SR.topp_decided(SR.kept_set(vs[r], 0, topp)[1], topp, tau_of(V)), f"row {r} is not decided"
    if ngram:
        assert sum(len(BR.banned_tokens(h, ngram)) for h in c["hist"]) >= R // 4, "the case bans too little"
    got = run_step(lib, c, temp, topk, topp)
    fails = {r: check_row(c, vs[r], r, got, r, topk, topp) for r in range(R)}
    fails = {r: f for r, f in fails.items() if f}
    assert not fails, fails
    for r in range(R):                                                      # the masks, as the draw saw them
        t = int(got["tok"][r])
        assert t != PAD
        if c["step"][r] >= c["mxl"][r]:
            assert t == EOS and got["kept"][r] == 1
        elif c["step"][r] < MIN_LEN:
            assert t != EOS
        if ngram:
            assert t not in BR.banned_tokens(c["hist"][r], ngram)
    print(f"V={V} R={R} T={temp} {kind}={x} ngram={ngram}: kept {got['kept'].min()}..{got['kept'].max()}, "
          f"{len(set(got['tok'].tolist()))} distinct tokens")


@pytest.mark.parametrize("kind,x", [("none", 0), ("topk", 5), ("topp", 0.9)])
def test_mutants_of_the_reference_fail(lib, kind, x):
    V, R = 97, 64
    c = case(V, R)
    vs = ref_values(c, 1.0)
    topk, topp = (x if kind == "topk" else 0), (x if kind == "topp" else 0.0)
    got = run_step(lib, c, 1.0, topk, topp)
    assert not any(check_row(c, vs[r], r, got, r, topk, topp) for r in range(R))
    free = [r for r in range(R) if c["step"][r] < c["mxl"][r]]              # a row at max_len has one token to draw
    for name, mut in (("shifted draw", dict(shift=1)), ("short kept set", dict(short=1)), ("word 1", dict(word=1))):
        rows = range(R) if name == "word 1" else free
        n_fail = sum(1 for r in rows if check_row(c, vs[r], r, got, r, topk, topp, **mut))
        assert 2 * n_fail >= R, f"{name}: only {n_fail} of {R} rows fail"


def test_two_runs_give_the_same_bits_and_rows_do_not_depend_on_the_pack(lib):
    for V, R, topk, topp in ((6000, 17, 0, 0.9), (97, 33, 5, 0.0), (9, 64, 0, 0.0)):
        c = case(V, R, 0, DATA_SEEDS.get((V, R)))
        a, b = run_step(lib, c, 1.7, topk, topp), run_step(lib, c, 1.7, topk, topp)
        for k in ("tok", "kept"):
            assert np.array_equal(a[k], b[k])
        for k in ("score", "u"):
            assert np.array_equal(bits(a[k]), bits(b[k]))
        rows = list(range(5, R))
        s = run_step(lib, c, 1.7, topk, topp, rows=rows)
        assert np.array_equal(s["tok"], a["tok"][rows]) and np.array_equal(s["kept"], a["kept"][rows])
        assert np.array_equal(bits(s["score"]), bits(a["score"][rows])) and np.array_equal(bits(s["u"]), bits(a["u"][rows]))
        other = run_step(lib, c, 1.7, topk, topp, seed=SEED + 1)
        assert not np.array_equal(bits(other["u"]), bits(a["u"]))


def test_sample_step_refusals(lib):
    from streamspeech_amd import lib as L
    c = case(97, 33)
    a = [dev(c["logits"], np.float32), dev(c["mxl"], np.int32), dev(c["npre"], np.int32), dev(c["j"], np.int32), dev(c["keys"], np.int64)]
    o = [torch.zeros(33, dtype=torch.int32, device="cuda"), torch.zeros(33, dtype=torch.float32, device="cuda")]

    def call(so, temp=1.0, n=0, keys=a[4], V=97):
        return lib.ss_op_sample_step(S(), P(a[0]), 33, V, T_STEP, MIN_LEN, P(a[1]), P(a[2]), PAD, UNK, EOS, PEN, temp, n, None, None, 7, C0,
                                     None, None, P(a[3]), P(keys), C.byref(so) if so is not None else None, P(o[0]), P(o[1]), None, None)
    ok = L.sample_opts(5, 0.0, 1)
    assert call(ok) == 0
    for so in (None, L.SSMtSampleOpts(16, 5, 0.0, 0, 1), L.sample_opts(-1, 0.0, 1), L.sample_opts(98, 0.0, 1), L.sample_opts(0, 1.5, 1),
               L.sample_opts(0, float("nan"), 1), L.sample_opts(0, -0.5, 1), L.sample_opts(3, 0.5, 1)):
        assert call(so) == 2
    assert call(ok, keys=None) == 2 and call(ok, temp=0.0) == 2 and call(ok, n=1) == 2 and call(ok, n=2) == 2   # a ban without history
    assert call(ok, V=16385) == 2
    torch.cuda.synchronize()
