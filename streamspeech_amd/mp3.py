"""MP3 sources: the reference reads `.mp3` paths with soundfile (SimulEval s2t_dataloader.py:62-63,
fairseq audio_utils.py:69-110); here a Layer III decoder of our own does it in two stages through the C ABI.

* ss_mp3_unpack (host, csrc/mp3_host.hip): container, headers, side info, bit reservoir, scalefactors, Huffman -> one 80-byte
  record + int16 q[576] per granule-channel.  Runs on a thread pool: ctypes drops the GIL and the stage has no shared state.
* ss_mp3_synthesize (device, csrc/mp3.hip): requantisation ... polyphase synthesis of a ragged batch of files in one call.

Output: float32 PCM as soundfile.read returns it (not clipped, not rounded to 16 bits); `mono=True` takes the channel mean as
read_wav and fairseq's to_mono do.  No other decoder exists in this image, so the decoder is pinned by the tests of
tests/test_mp3_cpu.py / tests/test_mp3_gpu.py (tables, exact bit accounting on real streams, a float64 restatement of the
synthesis, streams written by tests/mp3_writer.py), not by bit parity with a third-party decoder.
"""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as L

SS_ERR_CAPACITY, SS_ERR_BITSTREAM, SS_ERR_UNSUPPORTED = 4, 6, 7


class Mp3Info(C.Structure):
    _fields_ = [("version", C.c_int32), ("sample_rate", C.c_int32), ("channels", C.c_int32), ("frames", C.c_int32),
                ("granules", C.c_int32), ("granule_channels", C.c_int32), ("samples", C.c_int64), ("delay", C.c_int32),
                ("padding", C.c_int32), ("skip", C.c_int32), ("sr_index", C.c_int32)]


# ss_mp3_granule (include/streamspeech_hip.h), 80 bytes
GRANULE_DTYPE = np.dtype([("global_gain", "<i2"), ("nz", "<i2"), ("scalefac_scale", "u1"), ("preflag", "u1"),
                          ("block_type", "u1"), ("mixed", "u1"), ("ms", "u1"), ("sr_index", "u1"),
                          ("subblock_gain", "u1", (3,)), ("pad0", "u1", (3,)), ("sf_l", "u1", (22,)),
                          ("sf_s", "u1", (13, 3)), ("pad1", "u1", (3,))])
assert GRANULE_DTYPE.itemsize == 80

# ss_mp3_file, 32 bytes
FILE_DTYPE = np.dtype([("rec_offset", "<i8"), ("out_offset", "<i8"), ("granules", "<i4"), ("channels", "<i4"),
                       ("skip", "<i4"), ("n_out", "<i4")])
assert FILE_DTYPE.itemsize == 32


class Mp3Error(L.StreamSpeechHipError):
    """A stream the decoder refuses; `.code` is the SS_ERR_* value."""

    def __init__(self, msg: str, code: int):
        super().__init__(msg)
        self.code = code


def _raise(rc: int, what: str, name: Optional[str]):
    msg = L.load().ss_error_string(rc).decode()
    where = f"{name}: " if name else ""
    raise Mp3Error(f"{where}{what} failed: {msg} (code {rc})", rc)


def probe(data: bytes, name: Optional[str] = None) -> dict:
    """Container + headers only: version (1, 2, 25), sample_rate, channels, frames, granules, granule_channels, samples (per
    channel, after the gapless trim), delay / padding (LAME tag, -1 without one), skip (samples trimmed at the start)."""
    info = Mp3Info()
    rc = L.load().ss_mp3_probe(bytes(data), len(data), C.byref(info))
    if rc:
        _raise(rc, "ss_mp3_probe", name)
    return {k: getattr(info, k) for k, _ in Mp3Info._fields_}


def unpack(data: bytes, name: Optional[str] = None):
    """-> (probe dict, q int16 [granule_channels, 576], records GRANULE_DTYPE [granule_channels], bits int32 [granule_channels])."""
    data = bytes(data)
    info = probe(data, name)
    n = info["granule_channels"]
    q = np.zeros((max(n, 1), 576), np.int16)
    rec = np.zeros(max(n, 1), GRANULE_DTYPE)
    bits = np.zeros(max(n, 1), np.int32)
    rc = L.load().ss_mp3_unpack(data, len(data), n, q.ctypes.data, rec.ctypes.data, bits.ctypes.data)
    if rc:
        _raise(rc, "ss_mp3_unpack", name)
    return info, q[:n], rec[:n], bits[:n]


def decode_batch(blobs: Sequence[bytes], device, mono: bool = True, threads: Optional[int] = None,
                 names: Optional[Sequence[str]] = None, max_seconds: float = 640.0) -> List[Tuple[torch.Tensor, int]]:
    """Decode a batch of MP3 files: every file is probed first, then the files are cut, in order, into groups of at most
    `max_seconds` of audio (a longer file forms a group of its own); each group is unpacked on a thread pool, uploaded once and
    synthesised by one ss_mp3_synthesize call, so the device workspace (4.6 KB per granule-channel, ~234 MB per 640 s of mono
    48-kHz audio) stays bounded however long the list is.
    -> [(float32 tensor on `device` -- [n] with mono, else [channels, n] --, sample rate)], views of one buffer per group.
    A file whose container or headers the decoder refuses raises Mp3Error naming it before anything is launched; a file whose
    main data is corrupt raises before its group is launched."""
    names = list(names) if names is not None else [f"file {i}" for i in range(len(blobs))]
    infos = [probe(b, n) for b, n in zip(blobs, names)]
    groups, cur, cur_s = [], [], 0.0
    for i, info in enumerate(infos):
        sec = info["samples"] / info["sample_rate"]
        if cur and cur_s + sec > max_seconds:
            groups.append(cur)
            cur, cur_s = [], 0.0
        cur.append(i)
        cur_s += sec
    if cur:
        groups.append(cur)
    res = []
    for g in groups:
        res += _decode_group([blobs[i] for i in g], [names[i] for i in g], torch.device(device), mono, threads)
    return res


def _decode_group(blobs, names, dev, mono, threads):
    lib = L.load()
    nthreads = threads or min(len(blobs), os.cpu_count() or 1) or 1
    if nthreads > 1 and len(blobs) > 1:
        with ThreadPoolExecutor(nthreads) as ex:
            parts = list(ex.map(lambda a: unpack(a[0], a[1]), zip(blobs, names)))
    else:
        parts = [unpack(b, n) for b, n in zip(blobs, names)]
    files = np.zeros(len(parts), FILE_DTYPE)
    n_rec = out_floats = 0
    for i, (info, q, rec, _) in enumerate(parts):
        ch = info["channels"]
        files[i] = (n_rec, out_floats, info["granules"], ch, info["skip"], info["samples"])
        n_rec += info["granule_channels"]
        out_floats += info["samples"] * (1 if mono else ch)
    q_all = np.concatenate([p[1] for p in parts]) if n_rec else np.zeros((1, 576), np.int16)
    r_all = np.concatenate([p[2] for p in parts]) if n_rec else np.zeros(1, GRANULE_DTYPE)
    d_q = torch.from_numpy(q_all).to(dev)
    d_rec = torch.from_numpy(r_all.view(np.uint8)).to(dev)
    out = torch.empty((max(out_floats, 1),), dtype=torch.float32, device=dev)
    wb = C.c_size_t(0)
    fptr = files.ctypes.data if len(files) else None
    rc = lib.ss_mp3_synthesize(None, None, None, n_rec, fptr, len(files), int(mono), None, out_floats, None, C.byref(wb))
    if rc:
        _raise(rc, "ss_mp3_synthesize (size query)", None)
    work = torch.empty((max(wb.value, 1),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = lib.ss_mp3_synthesize(C.c_void_p(stream), d_q.data_ptr(), d_rec.data_ptr(), n_rec, fptr, len(files), int(mono),
                                   out.data_ptr(), out_floats, work.data_ptr(), C.byref(wb))
    if rc:
        _raise(rc, "ss_mp3_synthesize", None)
    res = []
    for i, (info, _, _, _) in enumerate(parts):
        o, n, ch = int(files[i]["out_offset"]), int(info["samples"]), info["channels"]
        t = out[o:o + n] if mono else out[o:o + n * ch].view(ch, n)
        res.append((t, info["sample_rate"]))
    # d_q / d_rec / work are freed below while the kernels may still run: torch's caching allocator reuses their memory only for
    # work ordered after them on this stream, which is where they were used
    return res

