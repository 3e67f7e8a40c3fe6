"""Raw PCM at the edge of the session pools: the formats a service receives off a socket (16-bit PCM, float32, G.711), staged once per
pool step.  :class:`PcmArena` is the step's one pinned host buffer -- every pushed chunk is copied into it on a 16-byte boundary, ONE
asynchronous upload moves it, and ONE ss_pcm_scatter launch (csrc/pcm.hip) decodes all chunks into the sessions' float32 sample
histories.  On the way out ss_pcm_pack_s16 turns the step's synthesised speech into 16-bit PCM for one download.  The conversions are
exact and are the bits of the list route (frontend.read_wav / write_wav); ss_pcm_decode_host / ss_pcm_pack_s16_host run the same
inline functions on the host (tests, and tools that have no device)."""
import ctypes as C
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np
import torch

from . import lib as L

SS_PCM_F32LE, SS_PCM_S16LE, SS_PCM_ULAW, SS_PCM_ALAW = 0, 1, 2, 3
FORMATS = {"f32le": SS_PCM_F32LE, "s16le": SS_PCM_S16LE, "ulaw": SS_PCM_ULAW, "alaw": SS_PCM_ALAW}
_SAMPLE_BYTES = {SS_PCM_F32LE: 4, SS_PCM_S16LE: 2, SS_PCM_ULAW: 1, SS_PCM_ALAW: 1}
_DTYPES = {SS_PCM_F32LE: (np.dtype("<f4"), torch.float32), SS_PCM_S16LE: (np.dtype("<i2"), torch.int16),
           SS_PCM_ULAW: (np.dtype("u1"), torch.uint8), SS_PCM_ALAW: (np.dtype("u1"), torch.uint8)}
ALIGN = 16                                    # ss_pcm_seg.src_offset: every chunk starts on a 16-byte boundary of the staging buffer


class PcmFormat:
    """A sample format ("f32le", "s16le", "ulaw", "alaw") and a channel count (1, or 2 interleaved: decoded to the channel mean)."""

    def __init__(self, fmt: str, channels: int = 1):
        if fmt not in FORMATS:
            raise ValueError(f"PCM format {fmt!r}: one of {tuple(FORMATS)}")
        if channels not in (1, 2):
            raise ValueError(f"{channels} channels: 1 or 2")
        self.fmt, self.channels = fmt, int(channels)
        self.code = FORMATS[fmt]
        self.bytes_per_frame = _SAMPLE_BYTES[self.code] * self.channels

    def __repr__(self):
        return f"PcmFormat({self.fmt!r}, channels={self.channels})"

    def __eq__(self, o):
        return isinstance(o, PcmFormat) and (o.fmt, o.channels) == (self.fmt, self.channels)

    def __hash__(self):
        return hash((self.fmt, self.channels))

    def frames(self, n_bytes: int) -> int:
        """Whole frames in n_bytes; a partial frame is refused (no remainder is carried from chunk to chunk)."""
        if n_bytes % self.bytes_per_frame:
            raise ValueError(f"{n_bytes} bytes are not a whole number of {self.bytes_per_frame}-byte {self.fmt} frames")
        return n_bytes // self.bytes_per_frame


@dataclass
class PcmSegment:
    """A pool's answer to a session opened with pcm_out: `content` is raw mono PCM bytes in `fmt` (beside the shim's segments)."""
    index: int = 0
    content: bytes = b""
    fmt: str = "s16le"
    sample_rate: int = 16000
    finished: bool = False
    is_empty: bool = False
    data_type: str = "pcm"


def as_bytes(data, fmt: PcmFormat) -> memoryview:
    """The chunk as a flat byte view, without a copy: bytes / bytearray / memoryview, or a C-contiguous NumPy or CPU torch array of the
    format's dtype (float32, int16, uint8).  Anything else is refused with ValueError; so is a partial frame."""
    np_dt, t_dt = _DTYPES[fmt.code]
    if isinstance(data, torch.Tensor):
        if data.device.type != "cpu" or data.dtype != t_dt or not data.is_contiguous():
            raise ValueError(f"a {fmt.fmt} chunk as a tensor: C-contiguous {t_dt} on the CPU")
        data = data.numpy()
    if isinstance(data, np.ndarray):
        if data.dtype != np_dt or not data.flags.c_contiguous:
            raise ValueError(f"a {fmt.fmt} chunk as an array: C-contiguous {np_dt}")
        mv = memoryview(data.reshape(-1).view(np.uint8))
    elif isinstance(data, (bytes, bytearray)):
        mv = memoryview(data)
    elif isinstance(data, memoryview):
        if not data.c_contiguous:
            raise ValueError("a PCM chunk as a memoryview: C-contiguous")
        mv = data.cast("B") if data.format != "B" or data.ndim != 1 else data
    else:
        raise ValueError(f"a PCM chunk is bytes, bytearray, memoryview, or a NumPy / CPU torch array, not {type(data).__name__}")
    fmt.frames(mv.nbytes)
    return mv


class PcmArena:
    """One pinned host buffer per pool, and the device staging tensor it is uploaded into.  add() copies a chunk in on a 16-byte
    boundary; the buffer grows by doubling and the chunks already added in this step survive the growth; upload() is the step's ONE
    asynchronous host-to-device copy, into a device tensor that is reused from step to step; clear() starts the next step.

    Single-buffered: the pinned buffer is not rewritten until the copy out of it is known to be complete.  A pool step synchronises
    with the device after its upload and before it returns (the CTC read of every step that encodes; clear() synchronises on the
    upload's own event otherwise), so a later step's add() never overtakes the copy and no second buffer is needed."""

    def __init__(self, device, capacity: int = 1 << 16):
        self.device = torch.device(device)
        self._pinned = self.device.type == "cuda"
        self._host = self._alloc(max(int(capacity), ALIGN))
        self._np = self._host.numpy()
        self._dev = None
        self._event = None
        self.used = 0
        self.uploads = 0                      # upload() calls that moved bytes, since the arena was made

    def _alloc(self, n: int) -> torch.Tensor:
        return torch.empty((n,), dtype=torch.uint8, pin_memory=self._pinned)

    @property
    def capacity(self) -> int:
        return self._host.numel()

    def clear(self):
        """Forget the step's chunks.  Waits for an upload that no other synchronisation of the step has covered."""
        if self._event is not None:
            self._event.synchronize()
            self._event = None
        self.used = 0

    def add(self, data, fmt: PcmFormat = None) -> int:
        """Copy a chunk in -> its byte offset (a multiple of 16).  With `fmt`, array dtypes and whole frames are checked (as_bytes)."""
        mv = as_bytes(data, fmt) if fmt is not None else memoryview(data).cast("B")
        off = (self.used + ALIGN - 1) & ~(ALIGN - 1)
        end = off + mv.nbytes
        if end > self.capacity:
            host = self._alloc(max(2 * self.capacity, 2 * end))
            new = host.numpy()
            new[:self.used] = self._np[:self.used]
            self._host, self._np = host, new
        if mv.nbytes:
            self._np[off:end] = np.frombuffer(mv, dtype=np.uint8)
        self.used = end
        return off

    def view(self, off: int, n: int) -> np.ndarray:
        return self._np[off:off + n]

    def upload(self) -> Tuple[torch.Tensor, int]:
        """-> (device staging tensor, bytes in it): one non-blocking copy of the used part on the current stream."""
        n = self.used
        if self._dev is None or self._dev.numel() < max(n, 1):
            self._dev = torch.empty((max(2 * n, self.capacity),), dtype=torch.uint8, device=self.device)
        if n:
            self._dev[:n].copy_(self._host[:n], non_blocking=True)
            if self._pinned:
                self._event = torch.cuda.Event()
                self._event.record()
            self.uploads += 1
        return self._dev, n

    def synchronized(self):
        """The caller has synchronised with the device since upload(): clear() need not wait."""
        self._event = None


def _seg_table(segs: Sequence[Tuple[int, int, int, int, int, int]]):
    tab = (L.SSPcmSeg * max(len(segs), 1))()
    for i, (src, dst_off, frames, fmt, ch, dst) in enumerate(segs):
        tab[i] = L.SSPcmSeg(int(src), int(dst_off), int(frames), int(fmt), int(ch), int(dst))
    return tab


def scatter(lib, stream, stage: torch.Tensor, stage_bytes: int, segs, dsts: List[torch.Tensor]):
    """ss_pcm_scatter: segs [(src_offset, dst_offset, frames, fmt code, channels, index into dsts)] of the device staging tensor into the
    float32 device tensors `dsts`, one launch."""
    n = len(dsts)
    for d in dsts:
        if d.dtype != torch.float32 or not d.is_contiguous():
            raise ValueError("a PCM destination is a contiguous float32 tensor")
    pp = (C.c_void_p * max(n, 1))(*[d.data_ptr() for d in dsts])
    caps = (C.c_int64 * max(n, 1))(*[d.numel() for d in dsts])
    L.check(lib.ss_pcm_scatter(stream, C.c_void_p(stage.data_ptr()), int(stage_bytes), _seg_table(segs), len(segs), pp, caps, n),
            "ss_pcm_scatter")


def pack_s16(lib, stream, src: torch.Tensor, out: torch.Tensor):
    """ss_pcm_pack_s16: the float32 device tensor `src` -> the int16 device tensor `out` (same length), one launch."""
    if src.dtype != torch.float32 or out.dtype != torch.int16 or not src.is_contiguous() or not out.is_contiguous() \
            or out.numel() < src.numel():
        raise ValueError("pack_s16: contiguous float32 in, contiguous int16 out of at least the same length")
    L.check(lib.ss_pcm_pack_s16(stream, C.c_void_p(src.data_ptr()), src.numel(), C.c_void_p(out.data_ptr())), "ss_pcm_pack_s16")


def decode_host(data, fmt: PcmFormat, lib=None) -> np.ndarray:
    """ss_pcm_decode_host: a chunk -> float32 mono samples, on the host, by the kernels' own conversion functions."""
    lib = lib or L.load()
    mv = as_bytes(data, fmt)
    src = np.frombuffer(mv, dtype=np.uint8)
    n = fmt.frames(mv.nbytes)
    out = np.empty(n, np.float32)
    L.check(lib.ss_pcm_decode_host(C.c_void_p(src.ctypes.data if n else 0), fmt.code, fmt.channels, n,
                                   C.c_void_p(out.ctypes.data if n else 0)), "ss_pcm_decode_host")
    return out


def pack_s16_host(samples, lib=None) -> np.ndarray:
    """ss_pcm_pack_s16_host: float32 samples -> int16, on the host, by the kernel's own conversion function."""
    lib = lib or L.load()
    x = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
    out = np.empty(x.size, np.int16)
    L.check(lib.ss_pcm_pack_s16_host(C.c_void_p(x.ctypes.data if x.size else 0), x.size,
                                     C.c_void_p(out.ctypes.data if x.size else 0)), "ss_pcm_pack_s16_host")
    return out
