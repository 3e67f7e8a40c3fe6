"""Raw PCM at the edge of the session pools: the formats a service receives off a socket (16-bit PCM, float32, G.711), staged once per
pool step.  :class:`PcmArena` is the step's one pinned host buffer -- every pushed chunk is copied into it on a 16-byte boundary, ONE
asynchronous upload moves it, and ONE ss_pcm_scatter launch (csrc/pcm.hip) decodes all chunks into the sessions' float32 sample
histories.  On the way out ss_pcm_pack_s16 turns the step's synthesised speech into 16-bit PCM for one download.  The conversions are
exact and are the bits of the list route (frontend.read_wav / write_wav); ss_pcm_decode_host / ss_pcm_pack_s16_host run the same
inline functions on the host (tests, and tools that have no device).

:class:`PcmOut` is the way out at the caller's own rate and format: the speech of every such session of a step goes through ONE
ss_pcm_emit call -- the streaming output resampler with a short carried history per session, then the encoder -- and ONE download
(:class:`PcmEmitter`; :class:`PcmStreamEncoder` is the same machinery without a pool)."""
import ctypes as C
import math
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

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


OUT_RATES = (8000, 11025, 16000, 22050, 24000, 32000, 44100, 48000)      # the rates the documentation names; others: PcmOut
MAX_TAPS_BYTES = 64 * 1024                   # ss_resample's limit on a tap table (the taps go through LDS)


@dataclass(frozen=True)
class PcmOut:
    """What an S2ST session answers: mono `fmt` ("s16le", "f32le", "ulaw", "alaw") at `sample_rate` Hz.  Any rate whose ratio to
    16000 in lowest terms up / down gives a tap table ss_resample accepts (design_filter(up, down) within 64 KB: max(up, down) <= 819);
    8000, 11025, 16000, 22050, 24000, 32000, 44100 and 48000 all are.  Anything else is ValueError here, at construction."""
    fmt: str
    sample_rate: int = 16000

    def __post_init__(self):
        if self.fmt not in FORMATS:
            raise ValueError(f"PCM format {self.fmt!r}: one of {tuple(FORMATS)}")
        sr = self.sample_rate
        if isinstance(sr, bool) or not isinstance(sr, (int, np.integer)) or sr < 1:
            raise ValueError(f"sample rate {sr!r}: a positive integer")
        object.__setattr__(self, "sample_rate", int(sr))
        up, down, half = self.ratio
        if up != down and (2 * half + 1) * 4 > MAX_TAPS_BYTES:
            raise ValueError(f"sample rate {sr}: {up}/{down} of 16000 Hz needs {2 * half + 1} filter taps, more than the resampler's "
                             f"{MAX_TAPS_BYTES // 4}; rates such as {OUT_RATES} are served")

    @property
    def ratio(self) -> Tuple[int, int, int]:
        """(up, down, half): the ratio to 16000 Hz in lowest terms and design_filter's half length (0 when nothing is resampled)."""
        g = math.gcd(self.sample_rate, 16000)
        up, down = self.sample_rate // g, 16000 // g
        return up, down, (0 if up == down else 10 * max(up, down))

    @property
    def code(self) -> int:
        return FORMATS[self.fmt]

    @property
    def sample_bytes(self) -> int:
        return _SAMPLE_BYTES[self.code]

    @property
    def history(self) -> int:
        """Samples of 16-kHz output a session carries between calls: (2 * half) // up."""
        up, _, half = self.ratio
        return (2 * half) // up


@dataclass
class PcmSegment:
    """A pool's answer to a session opened with pcm_out: `content` is raw mono PCM bytes in `fmt` at `sample_rate` (the session's own:
    "s16le" at 16000 for pcm_out="s16le", the PcmOut's otherwise), beside the shim's segments."""
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


# ---- out at the caller's rate and format --------------------------------------------------------------------------------------------
def emit_count(n: int, up: int, down: int, half: int, finished: bool = False, lib=None) -> int:
    """ss_pcm_emit_count: K, the output samples settled after n samples at 16 kHz (all ceil(n * up / down) once finished)."""
    k = (lib or L.load()).ss_pcm_emit_count(int(n), int(up), int(down), int(half), 1 if finished else 0)
    if k < 0:
        raise ValueError(f"ss_pcm_emit_count({n}, {up}, {down}, {half})")
    return int(k)


class PcmOutState:
    """One session's side of the streaming output resampler: the device carry buffer (allocated here, sized from the ratio), the
    device taps (the engine's table of the ratio) and the host counters -- n samples of 16-kHz output received in this utterance, k
    samples emitted, flushed once the utterance has ended."""

    def __init__(self, out: PcmOut, engine):
        self.out = out
        self.up, self.down, self.half = out.ratio
        self.history = out.history
        dev = torch.device(engine.device)
        self.carry = torch.zeros((self.history,), dtype=torch.float32, device=dev) if self.history else None
        self.taps = engine.pcm_taps(self.up, self.down) if self.up != self.down else None
        self.reset()

    def reset(self):
        self.n, self.k, self.flushed = 0, 0, False


def emit_plan(items, lib=None):
    """[(PcmOutState, tail or None, finished)] -> (segment tuples of ss_pcm_emit, [(byte offset, bytes)], total bytes): every segment's
    output on a 16-byte boundary of one buffer.  A state that has flushed emits nothing (and takes nothing) until it is reset."""
    segs, ranges, cursor = [], [], 0
    for st, tail, finished in items:
        n_new = 0 if (tail is None or st.flushed) else int(tail.numel())
        if n_new and (tail.dtype != torch.float32 or not tail.is_contiguous()):
            raise ValueError("a PcmOut tail is a contiguous float32 tensor")
        k1 = st.k if st.flushed else emit_count(st.n + n_new, st.up, st.down, st.half, finished, lib)
        off = (cursor + ALIGN - 1) & ~(ALIGN - 1)
        nbytes = (k1 - st.k) * st.out.sample_bytes
        cursor = off + nbytes
        segs.append((st.carry.data_ptr() if st.carry is not None else 0, tail.data_ptr() if n_new else 0,
                     st.taps.data_ptr() if st.taps is not None else 0, st.n, st.k, k1, off, min(st.history, st.n), n_new,
                     st.up, st.down, st.half, st.out.code, 1 if finished else 0))
        ranges.append((off, nbytes))
    return segs, ranges, cursor


def _emit_table(segs):
    tab = (L.SSPcmEmitSeg * max(len(segs), 1))()
    for i, sg in enumerate(segs):
        tab[i] = L.SSPcmEmitSeg(*[int(v) for v in sg], 0)
    return tab


def emit(lib, stream, segs, out: torch.Tensor):
    """ss_pcm_emit: the segment tuples of emit_plan into the uint8 device tensor `out`."""
    if out.dtype != torch.uint8 or not out.is_contiguous():
        raise ValueError("emit: a contiguous uint8 output tensor")
    L.check(lib.ss_pcm_emit(stream, _emit_table(segs), len(segs), C.c_void_p(out.data_ptr() if out.numel() else 0), out.numel()),
            "ss_pcm_emit")


def emit_host(segs, out: torch.Tensor, lib=None):
    """ss_pcm_emit_host: the same call on CPU tensors (every pointer of the segments is host memory)."""
    if out.dtype != torch.uint8 or not out.is_contiguous() or out.device.type != "cpu":
        raise ValueError("emit_host: a contiguous uint8 CPU tensor")
    L.check((lib or L.load()).ss_pcm_emit_host(_emit_table(segs), len(segs), C.c_void_p(out.data_ptr() if out.numel() else 0),
                                               out.numel()), "ss_pcm_emit_host")


def encode_host(samples, fmt: str, lib=None) -> bytes:
    """ss_pcm_encode_host: float32 samples -> bytes in `fmt`, on the host, by the kernel's own encoders."""
    lib = lib or L.load()
    x = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
    out = np.empty(x.size * _SAMPLE_BYTES[FORMATS[fmt]], np.uint8)
    L.check(lib.ss_pcm_encode_host(C.c_void_p(x.ctypes.data if x.size else 0), x.size, FORMATS[fmt],
                                   C.c_void_p(out.ctypes.data if x.size else 0)), "ss_pcm_encode_host")
    return out.tobytes()


class PcmEmitter:
    """The out side of a pool step (or of a PcmStreamEncoder): ONE engine.pcm_emit call for every session that answers at its own
    rate and format, ONE device-to-host copy into pinned memory, then a bytes object per session.  The device and pinned buffers are
    reused from call to call and grow by doubling.  Driven by one host thread, like the pools."""

    def __init__(self, engine):
        self.engine = engine
        self.device = torch.device(engine.device)
        self._dev = self._host = None
        self.calls = 0                        # engine.pcm_emit calls since the emitter was made

    def emit(self, items) -> List[bytes]:
        """[(PcmOutState, tail or None, finished)] -> each one's new bytes; the states advance."""
        segs, ranges, total = emit_plan(items, getattr(self.engine, "lib", None))
        if not any(sg[8] or sg[5] > sg[4] for sg in segs):       # nothing new and nothing to flush anywhere: no call
            return [b""] * len(items)
        cuda = self.device.type == "cuda"
        if self._dev is None or self._dev.numel() < total:
            self._dev = torch.empty((max(2 * total, 4096),), dtype=torch.uint8, device=self.device)
            self._host = torch.empty((max(2 * total, 4096),), dtype=torch.uint8, pin_memory=cuda)
        self.engine.pcm_emit(segs, self._dev[:total])
        self.calls += 1
        if total:
            self._host[:total].copy_(self._dev[:total], non_blocking=True)
            if cuda:
                torch.cuda.current_stream(self.device).synchronize()   # the bytes below are read from the pinned buffer
        host = self._host.numpy()
        out = []
        for (st, _, finished), sg, (off, nbytes) in zip(items, segs, ranges):
            out.append(host[off:off + nbytes].tobytes() if nbytes else b"")
            if not st.flushed:
                st.n, st.k, st.flushed = st.n + sg[8], sg[5], bool(finished)
        return out


class PcmStreamEncoder:
    """The streaming output resampler and encoder without a pool, as Mp3StreamDecoder is for input: push() takes the next float32
    samples of a 16-kHz stream (a tensor on the engine's device, or anything torch.as_tensor takes) and returns the bytes they settle
    in `out`'s format at its rate; finished=True flushes the rest, after which reset() starts a new stream.  The concatenated
    returns are encode(resample(whole stream)) byte for byte, however the stream was cut.  `engine`: a HipModel."""

    def __init__(self, engine, out: PcmOut):
        if not isinstance(out, PcmOut):
            raise ValueError(f"a PcmOut, not {out!r}")
        self.out = out
        self._state = PcmOutState(out, engine)
        self._emitter = PcmEmitter(engine)

    def push(self, samples, finished: bool = False) -> bytes:
        if self._state.flushed:
            raise ValueError("the stream is finished: reset() starts a new one")
        x = torch.as_tensor(samples, dtype=torch.float32).reshape(-1).to(self._emitter.device).contiguous()
        return self._emitter.emit([(self._state, x, finished)])[0]

    def reset(self):
        self._state.reset()
