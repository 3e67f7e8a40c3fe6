"""Writes tests/golden/flac/: run once with the reference tree present (python tests/make_golden_flac.py [reference root]).

Source: fairseq/examples/hubert/tests/6313-76958-0021.flac of the reference tree -- a real libFLAC 1.2.1 stream, 16 kHz mono 16-bit,
block size 4096, 190,800 samples, whose STREAMINFO holds the MD5 of its PCM.  The fixture is the stream's header plus its first
16 frames (65,536 samples), cut at a frame boundary, STREAMINFO left as it is (so it declares more samples than the fixture holds,
which a decoder must accept).  The MD5 of the prefix's PCM is recorded only after the decode of the WHOLE file by the independent
decoder (tests/flac_ref.py) has matched the MD5 in STREAMINFO: the prefix of a verified decode."""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import flac_ref as R  # noqa: E402

REL = "fairseq/examples/hubert/tests/6313-76958-0021.flac"
FRAMES = 16


def s16le(samples) -> bytes:
    return b"".join((v & 0xffff).to_bytes(2, "little") for v in samples)


def main(ref_root="/root/reference"):
    data = open(os.path.join(ref_root, REL), "rb").read()
    facts, chans = R.decode(data)
    full_md5 = hashlib.md5(s16le(chans[0])).hexdigest()
    if full_md5 != facts["md5"]:
        raise SystemExit(f"the full decode does not match STREAMINFO: {full_md5} != {facts['md5']}")
    cut = facts["frame_ends"][FRAMES - 1]
    n = sum(facts["blocks"][:FRAMES])
    out = os.path.join(HERE, "golden", "flac")
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, "libflac_16k_mono.flac"), "wb") as f:
        f.write(data[:cut])
    rec = {"source": REL, "source_bytes": len(data), "source_frames": facts["frames"], "source_samples": facts["samples"],
           "streaminfo_md5": facts["md5"], "sample_rate": facts["sample_rate"], "channels": facts["channels"],
           "bits_per_sample": facts["bits_per_sample"], "block_size": facts["max_block"], "total_samples": facts["total_samples"],
           "file": "libflac_16k_mono.flac", "bytes": cut, "frames": FRAMES, "samples": n,
           "prefix_pcm_md5": hashlib.md5(s16le(chans[0][:n])).hexdigest()}
    with open(os.path.join(out, "fixtures.json"), "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(rec)


if __name__ == "__main__":
    main(*sys.argv[1:2])
