"""FLAC ingest throughput on one pack of 128 clips, 640 s of 16-kHz mono audio at block size 4096 (2,500 subframes; the audio of one
bench.py step), built from the frames of the libFLAC fixture (tests/golden/flac/): host unpack (ss_flac_unpack) on 1 thread and on
the pool of at most 16; device restore (ss_flac_restore) with inputs resident, median of 30 with spread; the host twin
(ss_flac_restore_host) on the same records at 1 and 16 threads; and the offline ingest wall time of the pack as FLAC files
(frontend.load_audio_batch) against the same samples as 16-bit WAV files through the --pcm16-io staging (offline.stage_wavs_pcm16).
Prints one JSON line and writes it to profiles/flac_bench.json.

Kernel stats of the same run:
    rocprofv3 --kernel-trace --stats -d profiles/flac_rocprof -o flac -- python tools/flac_bench.py
"""
import ctypes as C
import json
import os
import sys
import tempfile
import time
import wave
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import flac_ref  # noqa: E402
from streamspeech_amd import flac, frontend, lib as L, offline  # noqa: E402

GOLD = os.path.join(ROOT, "tests", "golden", "flac")
THREADS = 16


def pack(n_clips=128, total_frames=2500):
    """Clips of 19 or 20 whole frames of the fixture (a rotation of its 16, so the clips differ), 2,500 frames = 640.0 s in all;
    STREAMINFO's total is rewritten to what the clip holds and its MD5 cleared."""
    data = open(os.path.join(GOLD, "libflac_16k_mono.flac"), "rb").read()
    ends = flac_ref.decode(data)[0]["frame_ends"]
    first = _first_frame(data)
    bounds = [first] + ends
    frames = [data[bounds[i]:bounds[i + 1]] for i in range(len(ends))]
    head = bytearray(data[:first])
    clips = []
    for i in range(n_clips):
        k = 20 if i < total_frames - 19 * n_clips else 19
        n = k * 4096
        head[21] = (head[21] & 0xf0) | ((n >> 32) & 0xf)
        head[22:26] = (n & 0xffffffff).to_bytes(4, "big")
        head[26:42] = bytes(16)
        clips.append(bytes(head) + b"".join(frames[(i + j) % len(frames)] for j in range(k)))
    return clips


def _first_frame(data):
    at = 4
    while True:
        last, ln = data[at] >> 7, int.from_bytes(data[at + 1:at + 4], "big")
        at += 4 + ln
        if last:
            return at


def timed(fn, repeats=5):
    ts = []
    for _ in range(repeats):
        t = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t)
    return ts


def spread(ts, scale=1.0, nd=4):
    a = np.asarray(ts) * scale
    return {"median": round(float(np.median(a)), nd), "min": round(float(a.min()), nd), "max": round(float(a.max()), nd),
            "p10": round(float(np.percentile(a, 10)), nd), "p90": round(float(np.percentile(a, 90)), nd), "n": len(ts)}


def main():
    clips = pack()
    infos = [flac.probe(c) for c in clips]
    audio_s = sum(i["samples"] / i["sample_rate"] for i in infos)
    n_sub = sum(i["subframes"] for i in infos)
    # host stage
    host1 = timed(lambda: [flac.unpack(c) for c in clips], 3)
    with ThreadPoolExecutor(THREADS) as ex:
        hostn = timed(lambda: list(ex.map(flac.unpack, clips)), 5)
        parts = [flac.unpack(c) for c in clips]
        # host twin of the device stage, per file
        rest1 = timed(lambda: [flac.restore_host([p], True) for p in parts], 3)
        restn = timed(lambda: list(ex.map(lambda p: flac.restore_host([p], True), parts)), 5)
    host_out = np.concatenate([flac.restore_host([p], True)[0] for p in parts])
    # device stage: inputs resident, one ss_flac_restore per iteration
    dev = torch.device("cuda:0")
    lib = L.load()
    files, r_all, res_all, n_rec, n_res, out_floats = flac._tables(parts, True)
    d_res = torch.from_numpy(res_all).to(dev)
    d_rec = torch.from_numpy(r_all.view(np.uint8)).to(dev)
    out = torch.empty((out_floats,), dtype=torch.float32, device=dev)
    wb = C.c_size_t(0)
    L.check(lib.ss_flac_restore(None, None, None, n_rec, n_res, files.ctypes.data, len(parts), 1, None, out_floats, None, C.byref(wb)))
    work = torch.empty((wb.value,), dtype=torch.uint8, device=dev)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def run():
        L.check(lib.ss_flac_restore(stream, d_res.data_ptr(), d_rec.data_ptr(), n_rec, n_res, files.ctypes.data, len(parts), 1,
                                    out.data_ptr(), out_floats, work.data_ptr(), C.byref(wb)), "ss_flac_restore")

    for _ in range(3):
        run()
    torch.cuda.synchronize()
    times = []
    for _ in range(30):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    assert np.array_equal(out.cpu().numpy(), host_out), "device and host restore differ"
    # restore with its upload (what decode_batch pays per pack after the unpack): device route against host route
    def dev_route():
        flac.restore_device(parts, dev, True)
        torch.cuda.synchronize()

    def host_route():
        with ThreadPoolExecutor(THREADS) as ex:
            fl = list(ex.map(lambda p: flac.restore_host([p], True)[0], parts))
        torch.from_numpy(np.concatenate(fl)).to(dev)
        torch.cuda.synchronize()

    dev_route(); host_route()
    t_dev_route, t_host_route = timed(dev_route, 7), timed(host_route, 7)
    # offline ingest: files on disk -> float32 PCM on the device
    from streamspeech_amd import synth
    from streamspeech_amd.config import ModelConfig
    from streamspeech_amd.engine import HipModel
    cfg = ModelConfig()
    model = HipModel(synth.make_model_state_dict(0, cfg), cfg)
    with tempfile.TemporaryDirectory() as tmp:
        fpaths, wpaths, at = [], [], 0
        for i, (c, p) in enumerate(zip(clips, parts)):
            fpaths.append(os.path.join(tmp, f"{i}.flac"))
            open(fpaths[-1], "wb").write(c)
            n = p[0]["samples"]
            wpaths.append(os.path.join(tmp, f"{i}.wav"))
            with wave.open(wpaths[-1], "wb") as w:
                w.setnchannels(1); w.setsampwidth(2); w.setframerate(16000)
                w.writeframes(np.round(host_out[at:at + n] * 32768.0).astype("<i2").tobytes())
            at += n

        def ingest_flac():
            r = frontend.load_audio_batch(fpaths, dev)
            torch.cuda.synchronize()
            return r

        def ingest_wav():
            r = offline.stage_wavs_pcm16(model, [frontend.read_wav_raw16(p) for p in wpaths], dev)
            torch.cuda.synchronize()
            return r

        a, b = ingest_flac(), ingest_wav()
        assert all(torch.equal(x[0], y[0]) for x, y in zip(a, b)), "FLAC and WAV ingest differ"
        t_flac, t_wav = timed(ingest_flac, 7), timed(ingest_wav, 7)
        flac_bytes, wav_bytes = sum(os.path.getsize(p) for p in fpaths), sum(os.path.getsize(p) for p in wpaths)
    med = float(np.median(times))
    res = {
        "clips": len(clips), "audio_s": round(audio_s, 2), "subframes": n_sub, "samples": int(n_res), "threads": THREADS,
        "host_unpack_1thread_s": spread(host1), "host_unpack_1thread_x_realtime": round(audio_s / float(np.median(host1)), 1),
        "host_unpack_16threads_s": spread(hostn), "host_unpack_16threads_x_realtime": round(audio_s / float(np.median(hostn)), 1),
        "host_restore_1thread_s": spread(rest1), "host_restore_16threads_s": spread(restn),
        "device_restore_ms": spread(times), "device_restore_x_realtime": round(audio_s / (med / 1e3), 0),
        "device_route_with_upload_s": spread(t_dev_route), "host_route_with_upload_s": spread(t_host_route),
        "device_beats_16thread_host_twin": bool(med / 1e3 < float(np.median(restn))),
        "device_route_beats_host_route": bool(np.median(t_dev_route) < np.median(t_host_route)),
        "default_route": flac.DEFAULT_ROUTE,
        "ingest_flac_s": spread(t_flac), "ingest_wav_pcm16_s": spread(t_wav), "flac_mb": round(flac_bytes / 2 ** 20, 2),
        "wav_mb": round(wav_bytes / 2 ** 20, 2), "workspace_mb": round(wb.value / 2 ** 20, 1), "device": torch.cuda.get_device_name(0),
    }
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "flac_bench.json"), "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
