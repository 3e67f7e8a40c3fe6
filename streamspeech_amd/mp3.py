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



# ---- streams: the same decoder, resumable (ss_mp3_stream_*) ------------------------------------------------------
class Mp3StreamInfo(C.Structure):
    _fields_ = [("version", C.c_int32), ("sample_rate", C.c_int32), ("channels", C.c_int32), ("sr_index", C.c_int32),
                ("delay", C.c_int32), ("padding", C.c_int32), ("skip", C.c_int32), ("hold", C.c_int32), ("buffered", C.c_int32),
                ("finished", C.c_int32), ("frames", C.c_int64), ("granules", C.c_int64), ("samples", C.c_int64),
                ("skipped_frames", C.c_int64), ("bytes_in", C.c_int64)]


assert C.sizeof(Mp3StreamInfo) == 80

# ss_mp3_stream_seg, 48 bytes
STREAM_SEG_DTYPE = np.dtype([("rec_offset", "<i8"), ("dst_offset", "<i8"), ("ch_stride", "<i8"), ("granules", "<i4"),
                             ("channels", "<i4"), ("skip", "<i4"), ("history", "<i4"), ("dst", "<i4"), ("pad0", "<i4")])
assert STREAM_SEG_DTYPE.itemsize == 48


def _info_dict(info: Mp3StreamInfo) -> dict:
    return {k: getattr(info, k) for k, _ in Mp3StreamInfo._fields_}


def _chunk_bytes(data) -> bytes:
    if isinstance(data, (bytes, bytearray, memoryview)):
        return bytes(data)
    if isinstance(data, np.ndarray) and data.dtype == np.uint8:
        return data.tobytes()
    raise ValueError(f"an MP3 chunk is bytes, bytearray, memoryview or a uint8 array, not {type(data).__name__}")


class Mp3Chunk:
    """What one push released: the records of the frames it completed and where their samples go.
    q [n_rec, 576] int16, rec [n_rec] GRANULE_DTYPE, bits [n_rec] int32; granules = new granules per channel, history = granules
    decoded before them (saturated at 2), skip = samples of the new granules the gapless trim drops at the front, written = samples
    the device stage writes (576 granules - skip), held = samples written by earlier pushes and not released yet (they lie in front
    of the new ones), released = samples this push hands on: the first `released` of held + written."""
    __slots__ = ("q", "rec", "bits", "channels", "granules", "history", "skip", "written", "held", "released", "n_bytes", "info")

    def __init__(self, q, rec, bits, before: dict, after: dict, n_bytes: int):
        self.q, self.rec, self.bits, self.info, self.n_bytes = q, rec, bits, after, n_bytes
        self.channels = max(after["channels"], 1)
        self.granules = int(after["granules"] - before["granules"])
        self.history = int(min(before["granules"], 2))
        syn0 = max(0, before["granules"] * 576 - after["skip"])            # the trim is known before the first audio frame
        syn1 = max(0, after["granules"] * 576 - after["skip"])
        self.written = int(syn1 - syn0)
        self.skip = self.granules * 576 - self.written
        self.held = int(syn0 - before["samples"])
        self.released = int(after["samples"] - before["samples"])


class Mp3Stream:
    """The host object of one MP3 stream (ss_mp3_stream): push() takes a chunk of any size and returns the records of the frames it
    completes.  A push the library refuses raises Mp3Error and leaves the object as it was.  mark() / rollback() take back pushes
    that SUCCEEDED (a pool that refuses the chunk for capacity after it has seen what it releases)."""

    def __init__(self, join: bool = False, name: Optional[str] = None):
        self.lib = L.load()
        self.name = name
        self._h, self._spare = C.c_void_p(), C.c_void_p()
        for h in (self._h, self._spare):
            rc = self.lib.ss_mp3_stream_create(int(bool(join)), C.byref(h))
            if rc:
                _raise(rc, "ss_mp3_stream_create", name)

    @property
    def info(self) -> dict:
        i = Mp3StreamInfo()
        L.check(self.lib.ss_mp3_stream_query(self._h, C.byref(i)), "ss_mp3_stream_query")
        return _info_dict(i)

    def push(self, data, finished: bool = False, cap: Optional[int] = None) -> Mp3Chunk:
        data = _chunk_bytes(data)
        before = self.info
        if cap is None:
            cap = int(self.lib.ss_mp3_stream_bound(self._h, len(data)))
        q = np.empty((max(cap, 1), 576), np.int16)
        rec = np.empty(max(cap, 1), GRANULE_DTYPE)
        bits = np.empty(max(cap, 1), np.int32)
        n, info = C.c_int64(0), Mp3StreamInfo()
        rc = self.lib.ss_mp3_stream_push(self._h, data, len(data), int(bool(finished)), int(cap), q.ctypes.data, rec.ctypes.data,
                                         bits.ctypes.data, C.byref(n), C.byref(info))
        if rc:
            _raise(rc, "ss_mp3_stream_push", self.name)
        k = n.value
        return Mp3Chunk(q[:k], rec[:k], bits[:k], before, _info_dict(info), len(data))

    def mark(self):
        L.check(self.lib.ss_mp3_stream_copy(self._spare, self._h), "ss_mp3_stream_copy")

    def rollback(self):
        L.check(self.lib.ss_mp3_stream_copy(self._h, self._spare), "ss_mp3_stream_copy")

    def reset(self):
        L.check(self.lib.ss_mp3_stream_reset(self._h), "ss_mp3_stream_reset")

    def close(self):
        for h in (self._h, self._spare):
            if h:
                self.lib.ss_mp3_stream_destroy(h)
                h.value = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def stream_state(channels: int, device) -> torch.Tensor:
    """The device state of one stream: the IMDCT blocks of its last two granules, [2, channels, 1152] float32.  Not zeroed: the
    device stage reads only as many of them as granules were decoded."""
    return torch.empty((2, int(channels), 1152), dtype=torch.float32, device=device)


def stream_synthesize(lib, stream, d_q: int, d_rec: int, n_rec: int, segs, states: Sequence[torch.Tensor],
                      dsts: Sequence[torch.Tensor], mono: bool, device):
    """ss_mp3_stream_synthesize: segs [(rec_offset, dst_offset, ch_stride, granules, channels, skip, history, index into dsts)], one
    per state, over n_rec records at the device addresses d_q / d_rec -> three launches whatever len(segs)."""
    for d in dsts:
        if d.dtype != torch.float32 or not d.is_contiguous():
            raise ValueError("an MP3 destination is a contiguous float32 tensor")
    tab = np.zeros(max(len(segs), 1), STREAM_SEG_DTYPE)
    for i, sg in enumerate(segs):
        tab[i] = tuple(int(v) for v in sg) + (0,)
    n, nd = len(segs), len(dsts)
    sp = (C.c_void_p * max(n, 1))(*[t.data_ptr() for t in states])
    pp = (C.c_void_p * max(nd, 1))(*[d.data_ptr() for d in dsts])
    caps = (C.c_int64 * max(nd, 1))(*[d.numel() for d in dsts])
    wb = C.c_size_t(0)
    rc = lib.ss_mp3_stream_synthesize(None, None, None, n_rec, tab.ctypes.data, n, sp, pp, caps, nd, int(mono), None, C.byref(wb))
    if rc:
        _raise(rc, "ss_mp3_stream_synthesize (size query)", None)
    work = torch.empty((max(wb.value, 1),), dtype=torch.uint8, device=device)
    rc = lib.ss_mp3_stream_synthesize(stream, C.c_void_p(d_q), C.c_void_p(d_rec), n_rec, tab.ctypes.data, n, sp, pp, caps, nd,
                                      int(mono), C.c_void_p(work.data_ptr()), C.byref(wb))
    if rc:
        _raise(rc, "ss_mp3_stream_synthesize", None)
    # `work` is freed while the kernels may still run: the caching allocator reuses it only for work ordered after them on this stream


def decode_stream_batch(arena, items, mono: bool = True, lib=None) -> Tuple[int, int]:
    """The many-session form: items [(Mp3Chunk, state tensor, destination tensor, offset of the chunk's first written sample in it,
    channel stride)] of one step -> (granule-channels decoded, bytes uploaded).  The q rows and records of all items are copied into
    `arena` (a pcm.PcmArena: ONE pinned staging buffer), uploaded ONCE, and decoded by ONE ss_mp3_stream_synthesize call straight
    into the destinations; the states move on.  Items without new granules cost nothing.  The caller owns the arena's step
    (clear() before, synchronized() once it has waited for the device)."""
    lib = lib or L.load()
    items = [it for it in items if it[0].granules > 0]
    if not items:
        return 0, 0
    n_rec = sum(len(it[0].rec) for it in items)
    q_off = None
    for ch, _, _, _, _ in items:                       # q rows are 1152 bytes and records 80: both stay contiguous on the arena's
        off = arena.add(memoryview(np.ascontiguousarray(ch.q)).cast("B"))     # 16-byte grid
        q_off = off if q_off is None else q_off
    r_off = None
    for ch, _, _, _, _ in items:
        off = arena.add(memoryview(np.ascontiguousarray(ch.rec).view(np.uint8)).cast("B"))
        r_off = off if r_off is None else r_off
    stage, n_bytes = arena.upload()
    segs, at = [], 0
    for i, (ch, _, _, dst_off, stride) in enumerate(items):
        segs.append((at, dst_off, stride, ch.granules, ch.channels, ch.skip, ch.history, i))
        at += len(ch.rec)
    dev = stage.device
    if dev.type == "cuda":
        with torch.cuda.device(dev):
            st = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
            stream_synthesize(lib, st, stage.data_ptr() + q_off, stage.data_ptr() + r_off, n_rec, segs, [it[1] for it in items],
                              [it[2] for it in items], mono, dev)
    else:
        raise Mp3Error("the MP3 device stage needs a GPU: there is no host synthesis", L.SS_ERR_ARG)
    return n_rec, n_bytes


class Mp3StreamDecoder:
    """One MP3 stream decoded incrementally on the GPU: push(chunk) -> the newly released float32 samples on `device`, [n] with
    mono (the channel mean) or [channels, n].  Fed in any chunking, the concatenated output is bit for bit decode_batch's of the
    whole stream (for inputs whose end the whole-file scan does not cut: trailing ID3v1 / APEv2 tags are not recognised in a
    stream).  A frame comes out once 4 bytes past its end have arrived, or at finished=True.  join=True: the stream was captured
    mid-way; decoding starts at the first frame whose main data this decoder holds entirely, and the first two granules after that
    (1152 samples per channel) are formed against an empty history.  A refused push raises Mp3Error and changes nothing.
    Until the first frame header is accepted the channel count is unknown: with mono=False the (empty) result then has one row."""

    def __init__(self, device, mono: bool = True, join: bool = False, name: Optional[str] = None):
        from .pcm import PcmArena
        self.device, self.mono = torch.device(device), bool(mono)
        self.host = Mp3Stream(join, name)
        self._arena = PcmArena(self.device)
        self._state = None
        self._held = None                         # samples synthesised and not released yet: [rows, held]

    @property
    def info(self) -> dict:
        return self.host.info

    def _empty(self, rows: int, n: int) -> torch.Tensor:
        return torch.empty((rows, n), dtype=torch.float32, device=self.device)

    def push(self, data, finished: bool = False) -> torch.Tensor:
        ch = self.host.push(data, finished)
        rows = 1 if self.mono else ch.channels
        held = self._held if self._held is not None and self._held.shape[0] == rows else self._empty(rows, 0)
        assert held.shape[1] == ch.held
        out = held
        if ch.granules:
            if self._state is None:
                self._state = stream_state(ch.channels, self.device)
            out = self._empty(rows, ch.held + ch.written)
            out[:, :ch.held] = held
            self._arena.clear()
            decode_stream_batch(self._arena, [(ch, self._state, out, ch.held, out.shape[1])], self.mono, self.host.lib)
        self._held = out[:, ch.released:]
        res = out[:, :ch.released]
        return res[0] if self.mono else res

    def reset(self):
        self.host.reset()
        self._state, self._held = None, None

    def close(self):
        self.host.close()
        self._state, self._held = None, None
