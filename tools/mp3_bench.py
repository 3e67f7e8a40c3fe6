"""MP3 ingest throughput: host unpack (ss_mp3_unpack) per second of audio on 1 thread and on all cores, and device synthesis
(ss_mp3_synthesize) of one pack of 128 clips, about 640 s of 48-kHz audio (the audio of one bench.py step), built by
concatenating the frames of the two example streams (tests/golden/mp3/).  Prints one JSON line and writes it to
profiles/mp3_bench.json.

Kernel stats of the same run:
    rocprofv3 --kernel-trace --stats -d profiles/mp3_rocprof -o mp3 -- python tools/mp3_bench.py
"""
import ctypes as C
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from streamspeech_amd import lib as L, mp3  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "mp3")
FRAME = 192                                          # bytes per frame of the examples (64 kb/s at 48 kHz, no padding)


def pack(n_clips=128, clip_s=5.0):
    a = open(os.path.join(GOLD, "common_voice_fr_17301936.mp3"), "rb").read()
    b = open(os.path.join(GOLD, "common_voice_fr_17767732.mp3"), "rb").read()
    clips = []
    for i in range(n_clips):
        x, y = (a, b) if i % 2 == 0 else (b, a)
        have = (len(x) - 45) // FRAME
        k = int(round(clip_s / 0.024)) - have          # frames of the other stream appended (its first frame starts the reservoir)
        clips.append(x + y[45:45 + k * FRAME])
    return clips


def main():
    clips = pack()
    infos = [mp3.probe(c) for c in clips]
    audio_s = sum(i["samples"] / i["sample_rate"] for i in infos)
    ncpu = os.cpu_count() or 1
    # host stage
    t = time.perf_counter()
    parts = [mp3.unpack(c) for c in clips]
    host1 = time.perf_counter() - t
    t = time.perf_counter()
    with ThreadPoolExecutor(ncpu) as ex:
        list(ex.map(mp3.unpack, clips))
    hostn = time.perf_counter() - t
    # device stage: inputs resident, one ss_mp3_synthesize per iteration
    dev = torch.device("cuda:0")
    lib = L.load()
    files = np.zeros(len(parts), mp3.FILE_DTYPE)
    n_rec = n_out = 0
    for i, (info, _, _, _) in enumerate(parts):
        files[i] = (n_rec, n_out, info["granules"], info["channels"], info["skip"], info["samples"])
        n_rec += info["granule_channels"]
        n_out += info["samples"]
    d_q = torch.from_numpy(np.concatenate([p[1] for p in parts])).to(dev)
    d_rec = torch.from_numpy(np.concatenate([p[2] for p in parts]).view(np.uint8)).to(dev)
    out = torch.empty((n_out,), dtype=torch.float32, device=dev)
    wb = C.c_size_t(0)
    L.check(lib.ss_mp3_synthesize(None, None, None, n_rec, files.ctypes.data, len(files), 1, None, n_out, None, C.byref(wb)))
    work = torch.empty((wb.value,), dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        L.check(lib.ss_mp3_synthesize(stream, d_q.data_ptr(), d_rec.data_ptr(), n_rec, files.ctypes.data, len(files), 1,
                                      out.data_ptr(), n_out, work.data_ptr(), C.byref(wb)), "ss_mp3_synthesize")

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(20):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    assert torch.isfinite(out).all()
    res = {
        "clips": len(clips), "audio_s": round(audio_s, 2), "granule_channels": n_rec,
        "host_unpack_1thread_s": round(host1, 4), "host_unpack_1thread_x_realtime": round(audio_s / host1, 1),
        "host_unpack_threads": ncpu, "host_unpack_allcores_s": round(hostn, 4),
        "host_unpack_allcores_x_realtime": round(audio_s / hostn, 1),
        "device_synth_ms_median": round(float(np.median(times)), 4), "device_synth_ms_min": round(float(np.min(times)), 4),
        "device_synth_x_realtime": round(audio_s / (float(np.median(times)) / 1e3), 0),
        "workspace_mb": round(wb.value / 2 ** 20, 1), "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    print(line)
    print("kernel stats of this command: rocprofv3 --kernel-trace --stats -d profiles/mp3_rocprof -o mp3 -- python tools/mp3_bench.py",
          file=sys.stderr)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "mp3_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
