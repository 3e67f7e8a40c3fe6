"""Largest |activation| the FP16 vocoder convs (csrc/conv_f16.hip) stage, per wide stage, on the synthetic checkpoint.

The kernel converts leaky_relu(x) of each ResBlock conv's input to FP16 (saturating at +-65504).  This runs the HiFi-GAN generator
(fairseq/models/text_to_speech/hifigan.py:154-170, ResBlock :95-102) in FP32 torch on the CPU and records, for the 256-, 128- and
64-channel stages, max |leaky_relu(x)| over the inputs of the dilated convs (convs1) and of the plain convs (convs2), and max |w| of
their weights, over unit sequences of the synthetic checkpoint with the bench workload's duration pattern (workload.make_utterances:
1, 1, 2 frames per unit).  Writes one JSON object (--out)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _w(sd, name):
    """Conv weight with weight norm folded (torch.nn.utils.weight_norm, dim 0), or the plain weight."""
    import torch
    if name + ".weight" in sd:
        return torch.as_tensor(sd[name + ".weight"]).float()
    v, g = torch.as_tensor(sd[name + ".weight_v"]).float(), torch.as_tensor(sd[name + ".weight_g"]).float()
    return g * v / v.reshape(v.shape[0], -1).norm(dim=1).view(-1, *([1] * (v.dim() - 1)))


def stage_ranges(vsd, units, vcfg):
    import torch
    import torch.nn.functional as F
    b = lambda name: torch.as_tensor(vsd[name]).float()   # noqa: E731
    code = torch.tensor(units, dtype=torch.long)
    emb = F.embedding(code, b("dict.weight"))
    dur = torch.tensor([(1, 1, 2)[i % 3] for i in range(len(units))], dtype=torch.long)
    x = torch.repeat_interleave(emb, dur, dim=0).t().contiguous()[None]
    x = F.conv1d(x, _w(vsd, "conv_pre"), b("conv_pre.bias"), padding=3)
    nk = len(vcfg.resblock_kernel_sizes)
    out = {}
    for i, (u, ku) in enumerate(zip(vcfg.upsample_rates, vcfg.upsample_kernel_sizes)):
        x = F.conv_transpose1d(F.leaky_relu(x, 0.1), _w(vsd, f"ups.{i}"), b(f"ups.{i}.bias"), stride=u,
                               padding=(ku - u) // 2)
        ch = x.shape[1]
        rec = {"convs1_input": 0.0, "convs2_input": 0.0, "weight": 0.0}
        xs = None
        for j, (kr, dils) in enumerate(zip(vcfg.resblock_kernel_sizes, vcfg.resblock_dilation_sizes)):
            r = x
            for di, dil in enumerate(dils):
                p = f"resblocks.{i * nk + j}"
                w1, w2 = _w(vsd, f"{p}.convs1.{di}"), _w(vsd, f"{p}.convs2.{di}")
                xt = F.leaky_relu(r, 0.1)
                rec["convs1_input"] = max(rec["convs1_input"], float(xt.abs().max()))
                xt = F.conv1d(xt, w1, b(f"{p}.convs1.{di}.bias"), dilation=dil, padding=(kr * dil - dil) // 2)
                xt = F.leaky_relu(xt, 0.1)
                rec["convs2_input"] = max(rec["convs2_input"], float(xt.abs().max()))
                xt = F.conv1d(xt, w2, b(f"{p}.convs2.{di}.bias"), padding=(kr - 1) // 2)
                rec["weight"] = max(rec["weight"], float(w1.abs().max()), float(w2.abs().max()))
                r = xt + r
            xs = r if xs is None else xs + r
        x = xs / nk
        out[ch] = rec
    return out, int(dur.sum())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--utterances", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vocoder_f16_range.json"))
    a = ap.parse_args()
    from streamspeech_amd import synth
    from streamspeech_amd.config import VocoderConfig
    vcfg = VocoderConfig()
    vsd = synth.make_vocoder_state_dict(0, vcfg)
    lens = [60, 170, 95, 130, 150, 77, 110, 165, 40, 200]
    tot, frames = {}, 0
    for k in range(a.utterances):
        units = [int(c) for c in synth.uniform(5, f"f16_range_{k}", (lens[k % len(lens)],), 0, 1000)]
        rec, fr = stage_ranges(vsd, units, vcfg)
        frames += fr
        for ch, r in rec.items():
            t = tot.setdefault(ch, {kk: 0.0 for kk in r})
            for kk, v in r.items():
                t[kk] = max(t[kk], v)
    wide = {f"{ch}_channels": tot[ch] for ch in (256, 128, 64) if ch in tot}
    res = {"checkpoint": "synthetic seed 0 (synth.make_vocoder_state_dict)", "utterances": a.utterances, "frames": frames,
           "fp16_max": 65504.0, "largest_abs_staged": wide,
           "headroom_vs_fp16_max": min(65504.0 / max(r["convs1_input"], r["convs2_input"]) for r in wide.values())}
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
