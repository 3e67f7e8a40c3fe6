"""FLAC sources: the reference's recipes write 16 kHz FLAC (`sf.write(..., ".flac")`, the members of
src_flac.zip) and read it back with soundfile (fairseq/data/audio/audio_utils.py); here a decoder of our own does it in two stages
through the C ABI, split as the MP3 ingest is (streamspeech_amd/mp3.py).

* ss_flac_unpack (host, csrc/flac_host.hip): container, metadata, frame headers, CRC-8 / CRC-16, Rice and escape residuals -> one
  96-byte record per subframe + one int32 per sample.  Runs on a thread pool: ctypes drops the GIL and the stage has no shared state.
* ss_flac_restore (device, csrc/flac.hip): predictor, wasted bits, stereo decorrelation, float conversion of a ragged batch of files
  in one launch.  ss_flac_restore_host is the same arithmetic on the host (`route="host"`).

FLAC is lossless, so the decoder is pinned bit for bit: the MD5 in a stream's STREAMINFO is that of its PCM (tests/test_flac_cpu.py).
Output: float32 PCM, float(s) * 2^-(bps-1) -- for a 16-bit file frontend.read_wav's bits; `mono=True` takes the channel mean.
"""
import ctypes as C
import os
from concurrent.futures import ThreadPoolExecutor
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import lib as L

SS_ERR_CAPACITY, SS_ERR_BITSTREAM, SS_ERR_UNSUPPORTED = 4, 6, 7
CONSTANT, VERBATIM, FIXED, LPC = 0, 1, 2, 3
INDEPENDENT, LEFT_SIDE, RIGHT_SIDE, MID_SIDE = 0, 1, 2, 3
MAX_THREADS = 16

# Which stage restores the samples when decode_batch is not told: the device stage, which restores the 128-clip, 640-s pack of
# tools/flac_bench.py in 0.42 ms against 13 ms for the 16-thread host twin (profiles/flac_bench.json); same bits.
DEFAULT_ROUTE = "device"


class FlacInfo(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("channels", C.c_int32), ("bits_per_sample", C.c_int32), ("frames", C.c_int32),
                ("subframes", C.c_int64), ("samples", C.c_int64), ("total_samples", C.c_int64), ("min_block", C.c_int32),
                ("max_block", C.c_int32), ("md5", C.c_uint8 * 16)]


assert C.sizeof(FlacInfo) == 64

# ss_flac_subframe (include/streamspeech_hip.h), 96 bytes
SUBFRAME_DTYPE = np.dtype([("res_offset", "<i8"), ("sample_start", "<i8"), ("block_size", "<i4"), ("type", "u1"), ("order", "u1"),
                           ("bps", "u1"), ("wasted", "u1"), ("shift", "u1"), ("assignment", "u1"), ("precision", "u1"),
                           ("channel", "u1"), ("reserved", "<i4"), ("coef", "<i2", (32,))])
assert SUBFRAME_DTYPE.itemsize == 96

# ss_flac_file, 32 bytes
FILE_DTYPE = np.dtype([("rec_offset", "<i8"), ("out_offset", "<i8"), ("frames", "<i4"), ("channels", "<i4"), ("bps", "<i4"),
                       ("n_out", "<i4")])
assert FILE_DTYPE.itemsize == 32


class FlacError(L.StreamSpeechHipError):
    """A stream the decoder refuses; `.code` is the SS_ERR_* value."""

    def __init__(self, msg: str, code: int):
        super().__init__(msg)
        self.code = code


def _raise(rc: int, what: str, name: Optional[str]):
    msg = L.load().ss_error_string(rc).decode()
    where = f"{name}: " if name else ""
    raise FlacError(f"{where}{what} failed: {msg} (code {rc})", rc)


def _info_dict(info: FlacInfo) -> dict:
    d = {k: getattr(info, k) for k, _ in FlacInfo._fields_ if k != "md5"}
    d["md5"] = bytes(info.md5).hex()
    return d


def pool_size(n_items: int, threads: Optional[int] = None) -> int:
    """Workers of the host stage: at most 16 and at most one per file, whatever the machine reports."""
    want = threads if threads else (os.cpu_count() or 1)
    return max(1, min(int(want), MAX_THREADS, max(int(n_items), 1)))


def streaminfo(data: bytes, name: Optional[str] = None) -> dict:
    """STREAMINFO only (no frame is read): sample_rate, channels, bits_per_sample, total_samples (0 = unknown), min_block,
    max_block, md5; frames / subframes / samples are 0."""
    info = FlacInfo()
    rc = L.load().ss_flac_streaminfo(bytes(data), len(data), C.byref(info))
    if rc:
        _raise(rc, "ss_flac_streaminfo", name)
    return _info_dict(info)


def probe(data: bytes, name: Optional[str] = None) -> dict:
    """The whole container, every frame walked and both CRCs checked: sample_rate, channels (1-8), bits_per_sample, frames,
    subframes (records), samples (per channel, counted from the frames), total_samples (STREAMINFO's, 0 = unknown), md5 (hex)."""
    info = FlacInfo()
    rc = L.load().ss_flac_probe(bytes(data), len(data), C.byref(info))
    if rc:
        _raise(rc, "ss_flac_probe", name)
    return _info_dict(info)


def unpack(data: bytes, name: Optional[str] = None):
    """-> (probe dict, res int32 [samples * channels], records SUBFRAME_DTYPE [subframes]).  The buffers are sized from STREAMINFO
    when it declares a total; a stream that holds more than it declares is walked once more to count."""
    data = bytes(data)
    lib = L.load()
    si = streaminfo(data, name)
    cap = res_cap = -1
    if si["total_samples"] > 0 and si["min_block"] >= 16:
        frames = -(-si["total_samples"] // si["min_block"]) + 1
        cap, res_cap = frames * si["channels"], (si["total_samples"] + si["max_block"]) * si["channels"]
        if res_cap > (1 << 28):                  # a header that declares hours: count first
            cap = -1
    info = FlacInfo()
    if cap >= 0:
        res, rec = np.empty(max(res_cap, 1), np.int32), np.empty(max(cap, 1), SUBFRAME_DTYPE)
        rc = lib.ss_flac_unpack(data, len(data), cap, res.ctypes.data, rec.ctypes.data, res_cap, C.byref(info))
        if rc == 0:
            d = _info_dict(info)
            return d, res[:d["samples"] * d["channels"]], rec[:d["subframes"]]
        if rc != SS_ERR_CAPACITY:
            _raise(rc, "ss_flac_unpack", name)
    d = probe(data, name)
    cap, res_cap = d["subframes"], d["samples"] * d["channels"]
    res, rec = np.empty(max(res_cap, 1), np.int32), np.empty(max(cap, 1), SUBFRAME_DTYPE)
    rc = lib.ss_flac_unpack(data, len(data), cap, res.ctypes.data, rec.ctypes.data, res_cap, C.byref(info))
    if rc:
        _raise(rc, "ss_flac_unpack", name)
    return d, res[:res_cap], rec[:cap]


def _tables(parts, mono: bool):
    """The file table of a pack of unpacked streams, and the records with their res_offset moved into the packed residuals."""
    files = np.zeros(max(len(parts), 1), FILE_DTYPE)
    recs, n_rec, n_res, out_floats = [], 0, 0, 0
    for i, (info, res, rec) in enumerate(parts):
        ch = info["channels"]
        files[i] = (n_rec, out_floats, info["frames"], ch, info["bits_per_sample"], info["samples"])
        r = rec.copy()
        r["res_offset"] += n_res
        recs.append(r)
        n_rec += len(rec)
        n_res += len(res)
        out_floats += info["samples"] * (1 if mono else ch)
    r_all = np.concatenate(recs) if n_rec else np.zeros(1, SUBFRAME_DTYPE)
    res_all = np.concatenate([p[1] for p in parts]) if n_res else np.zeros(1, np.int32)
    return files, r_all, res_all, n_rec, n_res, out_floats


def restore_host(parts, mono: bool = True, want_pcm: bool = False):
    """ss_flac_restore_host over unpacked streams [(info, res, rec)] -> [float32 array ([n] with mono, else [channels, n])], and with
    want_pcm also the exact integers, [int32 [channels, n]]."""
    files, r_all, res_all, n_rec, _, out_floats = _tables(parts, mono)
    out = np.zeros(max(out_floats, 1), np.float32)
    n_pcm = sum(p[0]["samples"] * p[0]["channels"] for p in parts)
    pcm = np.zeros(max(n_pcm, 1), np.int32) if want_pcm else None
    rc = L.load().ss_flac_restore_host(res_all.ctypes.data, r_all.ctypes.data, n_rec, files.ctypes.data, len(parts), int(mono),
                                       out.ctypes.data, pcm.ctypes.data if want_pcm else None)
    if rc:
        _raise(rc, "ss_flac_restore_host", None)
    floats, ints, at = [], [], 0
    for i, (info, _, _) in enumerate(parts):
        o, n, ch = int(files[i]["out_offset"]), info["samples"], info["channels"]
        floats.append(out[o:o + n] if mono else out[o:o + n * ch].reshape(ch, n))
        if want_pcm:
            ints.append(pcm[at:at + n * ch].reshape(ch, n))
            at += n * ch
    return (floats, ints) if want_pcm else floats


def pcm_bytes(pcm: np.ndarray, bps: int) -> bytes:
    """int32 [channels, n] -> the interleaved little-endian PCM a FLAC encoder hashes into STREAMINFO (ceil(bps / 8) bytes a sample)."""
    nb = (bps + 7) // 8
    inter = np.ascontiguousarray(pcm.T).astype("<i4")
    return inter.view(np.uint8).reshape(-1, 4)[:, :nb].tobytes()


def restore_device(parts, device, mono: bool = True) -> List[torch.Tensor]:
    """ss_flac_restore over unpacked streams: one upload of the residuals and records, one launch -> views of one device buffer."""
    lib = L.load()
    dev = torch.device(device)
    files, r_all, res_all, n_rec, n_res, out_floats = _tables(parts, mono)
    d_res = torch.from_numpy(res_all).to(dev)
    d_rec = torch.from_numpy(r_all.view(np.uint8)).to(dev)
    out = torch.empty((max(out_floats, 1),), dtype=torch.float32, device=dev)
    wb = C.c_size_t(0)
    fptr = files.ctypes.data
    rc = lib.ss_flac_restore(None, None, None, n_rec, n_res, fptr, len(parts), int(mono), None, out_floats, None, C.byref(wb))
    if rc:
        _raise(rc, "ss_flac_restore (size query)", None)
    work = torch.empty((max(wb.value, 1),), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        stream = torch.cuda.current_stream(dev).cuda_stream
        rc = lib.ss_flac_restore(C.c_void_p(stream), d_res.data_ptr(), d_rec.data_ptr(), n_rec, n_res, fptr, len(parts), int(mono),
                                 out.data_ptr(), out_floats, work.data_ptr(), C.byref(wb))
    if rc:
        _raise(rc, "ss_flac_restore", None)
    views = []
    for i, (info, _, _) in enumerate(parts):
        o, n, ch = int(files[i]["out_offset"]), info["samples"], info["channels"]
        views.append(out[o:o + n] if mono else out[o:o + n * ch].view(ch, n))
    # d_res / d_rec / work are freed while the kernel may still run: torch's caching allocator reuses their memory only for work
    # ordered after it on this stream, which is where they were used
    return views


def decode_batch(blobs: Sequence[bytes], device, mono: bool = True, threads: Optional[int] = None,
                 names: Optional[Sequence[str]] = None, max_seconds: float = 640.0,
                 route: Optional[str] = None) -> List[Tuple[torch.Tensor, int]]:
    """Decode a batch of FLAC files.  STREAMINFO of every file is read first (a file it refuses raises FlacError naming it before
    anything is unpacked), then the files are cut, in order, into groups of at most `max_seconds` of audio (a longer file, or one
    whose header does not declare its length, forms a group of its own); each group is unpacked on a thread pool of at most 16
    workers and restored by one ss_flac_restore launch (route "device") or by ss_flac_restore_host on the same pool and one upload
    (route "host"); both give the same bits.
    -> [(float32 tensor on `device` -- [n] with mono, else [channels, n] --, sample rate)]."""
    route = route or DEFAULT_ROUTE
    if route not in ("device", "host"):
        raise ValueError(f"route is 'device' or 'host', not {route!r}")
    names = list(names) if names is not None else [f"file {i}" for i in range(len(blobs))]
    infos = [streaminfo(b, n) for b, n in zip(blobs, names)]
    groups, cur, cur_s = [], [], 0.0
    for i, info in enumerate(infos):
        sec = info["total_samples"] / info["sample_rate"] if info["total_samples"] else max_seconds
        if cur and cur_s + sec > max_seconds:
            groups.append(cur)
            cur, cur_s = [], 0.0
        cur.append(i)
        cur_s += sec
    if cur:
        groups.append(cur)
    out = []
    dev = torch.device(device)
    for g in groups:
        gb, gn = [blobs[i] for i in g], [names[i] for i in g]
        nthreads = pool_size(len(gb), threads)
        if nthreads > 1:
            with ThreadPoolExecutor(nthreads) as ex:
                parts = list(ex.map(lambda a: unpack(a[0], a[1]), zip(gb, gn)))
                if route == "host":
                    floats = list(ex.map(lambda p: restore_host([p], mono)[0], parts))
        else:
            parts = [unpack(b, n) for b, n in zip(gb, gn)]
            if route == "host":
                floats = [restore_host([p], mono)[0] for p in parts]
        if route == "host":
            sizes = [f.size for f in floats]
            packed = torch.from_numpy(np.concatenate([f.reshape(-1) for f in floats]) if sum(sizes) else np.zeros(0, np.float32)).to(dev)
            views, at = [], 0
            for f, n in zip(floats, sizes):
                views.append(packed[at:at + n].view(f.shape))
                at += n
        else:
            views = restore_device(parts, dev, mono)
        out += [(v, p[0]["sample_rate"]) for v, p in zip(views, parts)]
    return out
