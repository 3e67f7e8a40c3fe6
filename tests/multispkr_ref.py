"""Restatements of the multi-speaker conv_pre for the tests (tests/test_multispkr_cpu.py, tests/test_multispkr_gpu.py): the
concatenated form of the reference (agent/tts/codehifigan.py:80-86: [code embedding ; speaker embedding] -> conv_pre) in float64,
the speaker table the weight packer makes of its speaker half, and the add kernel in NumPy float32.  TEST ONLY."""
import numpy as np
import torch
import torch.nn.functional as F

SEG_LENGTHS = (1, 2, 3, 4, 6, 7, 8, 20)            # 1-6: lo and hi both clip; 7 and 8: the first lengths with an interior row


def multispkr_config(num_speakers=5):
    from streamspeech_amd.config import VocoderConfig
    return VocoderConfig(model_in_dim=2 * VocoderConfig().embedding_dim, multispkr=True, num_speakers=num_speakers)


def folded_pre(vsd):
    """conv_pre's weight-norm-folded weight [C0, 2E, 7] (the float32 the packer folds, as float64) and bias."""
    from streamspeech_amd.weights import fold_weight_norm
    return fold_weight_norm(vsd, "conv_pre").double(), torch.from_numpy(np.asarray(vsd["conv_pre.bias"])).double()


def concat_conv_pre(w, b, code_emb, spk_vec):
    """The reference's form in float64: code_emb [L, E] and the speaker vector [E] repeated over the L frames, concatenated along
    the channels, through the 7-tap conv with padding 3.  -> [L, C0]."""
    L = code_emb.shape[0]
    x = torch.cat([code_emb.double().t(), spk_vec.double().view(-1, 1).expand(-1, L)], 0).unsqueeze(0)
    return F.conv1d(x, w, b, padding=3)[0].t()


def tap_vectors(w, spk):
    """G[s][k][co] = sum_c w[co, E + c, k] * spk[s, c] in float64.  -> [S, 7, C0]."""
    E = spk.shape[1]
    return torch.stack([torch.stack([w[:, E:, k] @ spk[s].double() for k in range(7)]) for s in range(spk.shape[0])])


def table64(w, spk):
    """[S, 16, C0] float64: entry 4 * lo + (hi - 3) = G[lo] + ... + G[hi], ascending taps."""
    G = tap_vectors(w, spk)
    out = torch.zeros((spk.shape[0], 16, w.shape[0]), dtype=torch.float64)
    for lo in range(4):
        for hi in range(3, 7):
            acc = torch.zeros_like(G[:, 0])
            for k in range(lo, hi + 1):
                acc = acc + G[:, k]
            out[:, 4 * lo + hi - 3] = acc
    return out


def entry(t, L):
    """Table entry of row t of a segment of L rows."""
    lo, hi = max(0, 3 - t), min(6, L + 2 - t)
    return 4 * lo + hi - 3


def split_conv_pre(w, b, code_emb, table_s):
    """The split form in float64: the code-half conv (Cin = E) plus the table entry of every row.  table_s [16, C0]."""
    E, L = code_emb.shape[1], code_emb.shape[0]
    y = F.conv1d(code_emb.double().t().unsqueeze(0), w[:, :E, :], b, padding=3)[0].t()
    return y + torch.stack([table_s[entry(t, L)] for t in range(L)])


def spkr_pre_add_np(x, C0, table, spkr, segs, act, slope=np.float32(0.1)):
    """The add kernel's documented arithmetic in NumPy float32: for row t of segment (start, L) with speaker sp,
    y[start + t, :C0] = act(x[start + t, :C0] + table[sp][entry(t, L)]) -- ONE float32 add, then the leaky-ReLU select and multiply.
    Rows outside every segment and columns past C0 keep x's values."""
    y = np.array(x, dtype=np.float32, copy=True)
    table = np.asarray(table, np.float32)
    for (start, L), sp in zip(segs, spkr):
        for t in range(L):
            v = (x[start + t, :C0] + table[sp, entry(t, L)]).astype(np.float32)
            if act:
                v = np.where(v > 0, v, (v * np.float32(slope)).astype(np.float32)).astype(np.float32)
            y[start + t, :C0] = v
    return y
