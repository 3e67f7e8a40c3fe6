"""OnlineFeatureExtractor of the agent (reference agent/speech_to_speech.streamspeech.agent.py:43-98)
over the fused fbank+CMVN HIP kernel, plus the waveform front-end.

The reference resamples the whole 48 kHz sample history to 16 kHz with sox ("rate", via
torchaudio.sox_effects, fairseq/data/audio/audio_utils.py:53-62) -- third-party arithmetic outside
the parity contract (BASELINE.json: "on the same fbank input").  Here a zero-phase
polyphase FIR with the published design of scipy.signal.resample_poly runs on the device
(ss_resample, csrc/fbank.hip) when the source is not already 16 kHz.  The streaming extractor does not resample the history it
has already seen: fbank rows whose samples can no longer change are kept, and the others are made from the source-rate history
with the resampler's sum inside the fbank kernel (ss_batch_fbank_frames_sr; OnlineFeatureExtractor.__call__).
"""
import array
import io
import math
import os
import wave
from typing import Optional

import numpy as np
import torch


def filter_half_len(up: int, down: int) -> int:
    """Taps on either side of design_filter's centre tap."""
    return 10 * max(up, down)


def design_filter(up: int, down: int) -> np.ndarray:
    """Low-pass of the polyphase resampler, float64 [2*10*max(up,down)+1]: windowed sinc, cutoff
    1/max(up,down) of Nyquist, Kaiser beta 5, unit DC gain, times `up` (the design
    scipy.signal.resample_poly documents; `up`/`down` in lowest terms)."""
    max_rate = max(up, down)
    half_len = filter_half_len(up, down)
    n = np.arange(2 * half_len + 1, dtype=np.float64) - half_len
    fc = 1.0 / max_rate
    h = fc * np.sinc(fc * n) * np.kaiser(2 * half_len + 1, 5.0)
    return h / h.sum() * up


def unsettled_fbank_frames(sr_in: int, sr_out: int = 16000, shift_samples: int = 160) -> int:
    """How many of the newest fbank frames may still change when more audio arrives: the resampler's output samples whose
    FIR window reaches past the end of the received input (zero-padded there) are recomputed on the next call -- that edge
    is half_len / down output samples of design_filter's low-pass -- and every fbank frame that overlaps it is unsettled.
    0 when nothing is resampled.  (ss_encoder_stream_set_tail: such frames must not be cached as final.)"""
    import math
    g = math.gcd(int(sr_in), int(sr_out))
    up, down = int(sr_out) // g, int(sr_in) // g
    if up == down:
        return 0
    half_len = (len(design_filter(up, down)) - 1) // 2
    edge = math.ceil(half_len / down)                       # output samples that still see zero padding
    return max(1, math.ceil(edge / shift_samples))


def read_wav(path):
    """PCM WAV (8/16/32-bit integer) -> (float32 mono samples in [-1, 1), sample rate): the `list[float]`
    the SimulEval dataloader hands the agent (SimulEval/simuleval/data/dataloader/s2t_dataloader.py).
    `path` is a file name or an open binary file object (a slice of a stored zip, read_audio_cell).
    MP3 (example/wavs/*.mp3) is not read here: read_audio / load_audio_batch decode it (streamspeech_amd/mp3.py)."""
    if isinstance(path, (str, os.PathLike)):
        if str(path).lower().endswith(".mp3"):
            raise IOError("no MP3 decoder is available here; convert %s to PCM WAV" % path)
        path = str(path)
    with wave.open(path, "rb") as w:
        sr, nch, sw, n = w.getframerate(), w.getnchannels(), w.getsampwidth(), w.getnframes()
        raw = w.readframes(n)
    if sw == 2:
        x = np.frombuffer(raw, "<i2").astype(np.float32) / 32768.0
    elif sw == 4:
        x = np.frombuffer(raw, "<i4").astype(np.float32) / 2147483648.0
    elif sw == 1:
        x = (np.frombuffer(raw, "u1").astype(np.float32) - 128.0) / 128.0
    else:
        raise IOError("unsupported WAV sample width %d" % sw)
    if nch > 1:
        x = x.reshape(-1, nch).mean(axis=1)          # convert_waveform(to_mono=True): channel mean
    return x, sr


def is_mp3(path) -> bool:
    return str(path).lower().endswith(".mp3")


def is_flac(path_or_bytes) -> bool:
    """A `.flac` path, or bytes that start with the `fLaC` marker."""
    if isinstance(path_or_bytes, (bytes, bytearray, memoryview)):
        return bytes(path_or_bytes[:4]) == b"fLaC"
    return str(path_or_bytes).lower().endswith(".flac")


def parse_audio_cell(cell: str):
    """A manifest's `audio` / `src_audio` cell, as fairseq's parse_path reads it (fairseq/data/audio/audio_utils.py): `<path>` ->
    (path,), `<zip path>:<byte offset>:<byte length>` -> (path, offset, length).  The member is stored uncompressed, so the slice
    is the file: no zip structure is parsed."""
    cell = str(cell)
    if os.path.splitext(cell)[1].lower() in (".wav", ".flac", ".ogg", ".mp3", ".npy"):
        return (cell,)
    path, *slices = cell.split(":")
    if len(slices) == 0:
        return (cell,)
    if len(slices) != 2 or not all(v.isdigit() for v in slices):
        raise ValueError(f"cannot read the audio cell {cell!r}: expected <path> or <zip>:<offset>:<length>")
    return (path, int(slices[0]), int(slices[1]))


def read_cell_bytes(cell: str) -> bytes:
    """The bytes a cell names: the whole file, or one seek + read of a stored zip's slice."""
    parsed = parse_audio_cell(cell)
    with open(parsed[0], "rb") as f:
        if len(parsed) == 1:
            return f.read()
        f.seek(parsed[1])
        data = f.read(parsed[2])
    if len(data) != parsed[2]:
        raise ValueError(f"the audio cell {cell!r} reaches past the end of {parsed[0]}")
    return data


def sniff(data: bytes, cell: str = "") -> str:
    """What a file or a zip slice holds, by its first bytes as fairseq's loader tells them apart: "npy" (precomputed features),
    "flac", "wav", or "mp3" (no magic of its own: whatever ss_mp3_probe accepts).  Anything else raises ValueError naming the cell."""
    head = bytes(data[:6])
    if head == b"\x93NUMPY":
        return "npy"
    if head[:4] == b"fLaC":
        return "flac"
    if head[:4] == b"RIFF":
        return "wav"
    from . import mp3
    try:
        mp3.probe(data)
        return "mp3"
    except mp3.Mp3Error:
        pass
    raise ValueError(f"the audio cell {cell!r} holds neither npy features nor FLAC, WAV or MP3 audio")


def read_features(data: bytes, cell: str = "") -> np.ndarray:
    """A `.npy` of raw fbank features -> float32 [T, 80] (fairseq get_features_from_npy_or_audio: np.load, no pickles)."""
    x = np.load(io.BytesIO(data), allow_pickle=False)
    if x.ndim != 2 or x.shape[1] != FEATURE_DIM:
        raise ValueError(f"the features of {cell!r} have shape {tuple(x.shape)}, expected [T, {FEATURE_DIM}]")
    return np.ascontiguousarray(x, dtype=np.float32)


def load_cells(cells, device):
    """Manifest cells (paths or stored-zip slices) -> [("pcm", float32 mono tensor on `device`, sample rate) | ("feat", float32
    [T, 80] tensor on `device`, None)], sniffed by content.  The FLAC cells of the call are decoded in one batch and the MP3 cells
    in another (flac.decode_batch / mp3.decode_batch, up to 640 s of audio per launch); WAV is read by read_wav from memory."""
    from . import flac, mp3
    blobs = [read_cell_bytes(c) for c in cells]
    kinds = [sniff(b, c) for b, c in zip(blobs, cells)]
    out = [None] * len(cells)
    for kind, mod in (("flac", flac), ("mp3", mp3)):
        idx = [k for k, v in enumerate(kinds) if v == kind]
        if idx:
            for k, (x, sr) in zip(idx, mod.decode_batch([blobs[k] for k in idx], device, mono=True, names=[str(cells[k]) for k in idx])):
                out[k] = ("pcm", x, sr)
    for k, kind in enumerate(kinds):
        if kind == "wav":
            x, sr = read_wav(io.BytesIO(blobs[k]))
            out[k] = ("pcm", torch.from_numpy(x).to(device), sr)
        elif kind == "npy":
            out[k] = ("feat", torch.from_numpy(read_features(blobs[k], cells[k])).to(device), None)
    return out


def check_eval_transforms(config: dict, split: str = "test"):
    """The feature transforms a data config applies at evaluation (fairseq S2TDataConfig.get_transforms: the split's list, else
    `_eval`, else `*`).  Only global_cmvn is implemented here (the model's CMVN vectors); anything else is refused by name."""
    for key in ("transforms", "feature_transforms"):
        tr = config.get(key) or {}
        if not isinstance(tr, dict):
            continue
        cur = tr.get(split)
        if cur is None:
            cur = tr.get("_eval")
        if cur is None:
            cur = tr.get("*")
        for name in cur or []:
            if name != "global_cmvn":
                raise ValueError(f"the data config lists the evaluation transform {name!r}; only global_cmvn is implemented")


def read_audio(path: str):
    """WAV, FLAC or MP3 -> (float32 numpy samples, sample rate), mono (channel mean) as read_wav returns them.  WAV goes through
    read_wav; FLAC and MP3 through the decoders of streamspeech_amd/flac.py and mp3.py (host bitstream stage, device stage), whose
    output is copied back to the host here -- load_audio_batch keeps it on the device."""
    if not is_mp3(path) and not is_flac(path):
        return read_wav(path)
    (x, sr), = load_audio_batch([path], "cuda")
    return x.cpu().numpy(), sr


def load_audio_batch(paths, device):
    """-> [(float32 mono tensor on `device`, sample rate)] for WAV / FLAC / MP3 paths.  The MP3 files of the call are decoded in
    batches of up to 640 s of audio (one ss_mp3_synthesize launch pair each, mp3.decode_batch), the FLAC files likewise
    (flac.decode_batch, one ss_flac_restore launch each), and stay on the device; WAV files are read by read_wav and uploaded."""
    from . import flac, mp3
    out = [None] * len(paths)
    for pick, mod in ((is_mp3, mp3), (lambda p: is_flac(str(p)), flac)):
        idx = [k for k, p in enumerate(paths) if pick(p)]
        if idx:
            blobs = []
            for k in idx:
                with open(paths[k], "rb") as f:
                    blobs.append(f.read())
            for k, res in zip(idx, mod.decode_batch(blobs, device, mono=True, names=[str(paths[k]) for k in idx])):
                out[k] = res
    for k, p in enumerate(paths):
        if out[k] is None:
            x, sr = read_wav(p)
            out[k] = (torch.from_numpy(x).to(device), sr)
    return out


def write_wav(path: str, samples, sr: int = 16000):
    """float samples in [-1, 1] -> 16-bit PCM WAV (generate_waveform_from_code.py dumps soundfile PCM_16)."""
    x = np.clip(np.asarray(samples, np.float32), -1.0, 1.0)
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(int(sr))
        w.writeframes(np.round(x * 32767.0).astype("<i2").tobytes())



def read_wav_raw16(path: str):
    """A 16-bit PCM WAV as it lies in the file -> (raw interleaved little-endian frames, channels, sample rate, frames), or None for
    any other sample width (the caller then takes read_wav).  The offline driver's --pcm16-io stages these bytes and decodes them on
    the device (ss_pcm_scatter), to read_wav's bits."""
    with wave.open(str(path), "rb") as w:
        if w.getsampwidth() != 2 or w.getnchannels() not in (1, 2):
            return None
        n = w.getnframes()
        return w.readframes(n), w.getnchannels(), w.getframerate(), n


def write_wav_pcm16(path: str, pcm16, sr: int = 16000):
    """write_wav for samples that are 16-bit PCM already (ss_pcm_pack_s16: write_wav's own rounding, done on the device)."""
    with wave.open(str(path), "wb") as w:
        w.setnchannels(1); w.setsampwidth(2); w.setframerate(int(sr))
        w.writeframes(np.ascontiguousarray(pcm16, dtype="<i2").tobytes())

SHIFT_SIZE, WINDOW_SIZE, ORG_SAMPLE_RATE, SAMPLE_RATE, FEATURE_DIM = 10, 25, 48000, 16000, 80


class OnlineFeatureExtractor:
    def __init__(self, args, engine):
        self.shift_size = args.shift_size
        self.window_size = args.window_size
        assert self.window_size >= self.shift_size
        self.sample_rate = args.sample_rate
        self.feature_dim = args.feature_dim
        self.num_samples_per_shift = int(self.shift_size * self.sample_rate / 1000)
        self.num_samples_per_window = int(self.window_size * self.sample_rate / 1000)
        self.len_ms_to_samples = lambda x: x * self.sample_rate / 1000
        self.engine = engine

    def clear_cache(self):
        self._np = np.zeros(0, np.float32)
        self._buf = np.zeros(0, np.float32)      # backing store of _np (grows by doubling: appending a segment does not copy the history)
        self._dev = None
        self._n_dev = 0
        self._fb = None                          # fbank rows of the cached history (HIP engine; see __call__)
        self._n_fb = 0                           # how many of them are final
        self._src_id = None
        self.n_pcm = 0                           # the PCM route's sample counter: samples decoded into _dev so far

    def _samples(self, samples, n):
        """float32 array of samples[:n].  SimulEval hands the WHOLE sample history as a Python list at every policy() call
        (states.source only grows within an utterance); converting 15 s of floats costs ~10 ms per call, so only the new
        tail is converted and the rest comes from the cache.  The cache belongs to ONE source list: it is dropped when
        another list object comes in (AgentStates.reset() starts a new list, SimulEval/simuleval/agents/states.py), when
        the history shrank, or when a spot check of eight cached values (compared as float32, the cache's type) fails.
        The agents also call clear_cache() in reset(); a caller that reuses an extractor for unrelated audio must do the same."""
        c = getattr(self, "_np", None)
        if c is None:
            self.clear_cache()
            c = self._np
        k = len(c)
        ok = k <= n and (k == 0 or getattr(self, "_src_id", None) == id(samples))
        if ok and k:
            for i in {0, k - 1, k // 2, k // 3, k // 5, (2 * k) // 3, (4 * k) // 5, k // 7}:
                if np.float32(samples[i]) != c[i]:
                    ok = False
                    break
        if not ok:
            self.clear_cache()
            c, k = self._np, 0
        self._src_id = id(samples)
        if n > k:
            # Python floats are doubles: array('d') takes the list in one C loop (1.4x faster than np.asarray(list)), the cast to float32
            # rounds exactly as np.asarray(list, float32) does
            new = np.frombuffer(array.array("d", samples[k:n]), dtype=np.float64)
            buf = getattr(self, "_buf", None)
            if buf is None or len(buf) < n or (k and buf.ctypes.data != c.ctypes.data):
                buf = np.empty(max(2 * n, 1 << 15), np.float32)
                buf[:k] = c
                self._buf = buf
            buf[k:n] = new
            c = buf[:n]
            self._np = c
        return c[:n]

    def frames_of(self, n_samples: int):
        """The frame arithmetic of a call, shared by the list route (stage) and the PCM route (stage_pcm): (num_frames, effective
        samples) of a history of `n_samples` samples, or None when no frame exists yet."""
        num_frames = math.floor(
            (n_samples - self.len_ms_to_samples(self.window_size - self.shift_size)) / self.num_samples_per_shift)
        if num_frames <= 0:
            return None
        effective = int(num_frames * self.len_ms_to_samples(self.shift_size)
                        + self.len_ms_to_samples(self.window_size - self.shift_size))
        return int(num_frames), effective

    def stage(self, new_samples):
        """The host part of a call: frames of the history so far, and its new samples copied to the device history.  -> (num_frames,
        effective samples), or None when no frame exists yet.  (The text session pool stages many sessions and computes their new
        fbank rows in one launch: new_rows / commit_rows.)"""
        samples = new_samples
        st = self.frames_of(len(samples))
        if st is None:
            return None
        num_frames, effective = st
        x = self._samples(samples, effective)
        # device copy of the history: only the new samples cross PCIe
        dev = self.engine.device
        if getattr(self, "_dev", None) is None or self._dev.numel() < effective or self._n_dev > effective:
            cap = max(2 * effective, 1 << 16)
            buf = torch.empty((cap,), dtype=torch.float32, device=dev)
            if getattr(self, "_dev", None) is not None and 0 < self._n_dev <= effective:
                buf[: self._n_dev] = self._dev[: self._n_dev]
            else:
                self._n_dev = 0
                self._n_fb = 0
            self._dev = buf
        if effective > self._n_dev:
            self._dev[self._n_dev:effective] = torch.from_numpy(x[self._n_dev:effective]).to(dev)
            self._n_dev = effective
        return int(num_frames), effective

    # ---- the PCM route: raw chunks decoded on the device (streamspeech_amd/pcm.py), a sample COUNTER instead of a sample list ----
    def pcm_reserve(self, frames: int, keep: int = 0):
        """Room for `frames` more samples in the device history (grown by doubling with a device copy, as stage() grows it) -> (the
        history tensor, the offset the new samples go to).  The caller has them written there (one ss_pcm_scatter for all sessions
        of a pool step) and then calls pcm_commit(frames).  keep: samples already written past n_pcm and not committed yet (what a
        gapless MP3 stream holds back); they survive a growth, and the caller writes behind them."""
        if getattr(self, "_np", None) is None:
            self.clear_cache()
        have = self.n_pcm + int(keep)
        n = have + int(frames)
        if self._dev is None or self._dev.numel() < n:
            buf = torch.empty((max(2 * n, 1 << 16),), dtype=torch.float32, device=self.engine.device)
            if self._dev is not None and have:
                buf[:have] = self._dev[:have]
            self._dev = buf
        return self._dev, self.n_pcm

    def pcm_commit(self, frames: int):
        self.n_pcm += int(frames)

    def stage_pcm(self):
        """stage() of the PCM route: (num_frames, effective samples) of the samples counted so far, or None.  The history may hold
        samples past `effective`; rows are computed from the first `effective` ones, exactly as the list route does."""
        return self.frames_of(self.n_pcm)

    def call_pcm(self, data, fmt, sr=None):
        """__call__ for a source that arrives as raw PCM chunks: `data` (bytes-like or a matching array, pcm.as_bytes) holds the NEW
        frames in `fmt` (a pcm.PcmFormat).  -> the fbank rows of everything received so far, bitwise those of __call__ on the list
        of the same samples.  One upload and one ss_pcm_scatter per call; a session pool does the same for all its sessions at once."""
        from . import pcm
        if getattr(self, "_arena", None) is None:
            self._arena = pcm.PcmArena(self.engine.device)
        self._arena.clear()
        frames = fmt.frames(pcm.as_bytes(data, fmt).nbytes)
        off = self._arena.add(data, fmt)
        dst, at = self.pcm_reserve(frames)
        stage, n = self._arena.upload()
        self.engine.pcm_scatter(stage, n, [(off, at, frames, fmt.code, fmt.channels, 0)], [dst])
        self.pcm_commit(frames)
        return self._rows(self.stage_pcm(), sr or self.sample_rate)

    def new_rows(self, nf: int) -> int:
        """The HIP engine: the first of the `nf` fbank rows that is not cached as final yet (the row buffer grows to hold all `nf`).
        The caller computes rows first .. nf - 1 into self._fb and then calls commit_rows(nf)."""
        k = self._n_fb if self._fb is not None else 0
        if k > nf:
            k = 0
        if self._fb is None or self._fb.shape[0] < nf:
            fb = torch.empty((max(2 * nf, 512), self.feature_dim), dtype=torch.float32, device=self.engine.device)
            if k:
                fb[:k] = self._fb[:k]
            self._fb = fb
        return k

    def commit_rows(self, nf: int, final: Optional[int] = None) -> torch.Tensor:
        """The `nf` rows of this call; `final` of them (all, for a 16-kHz source) stay as they are from now on."""
        self._n_fb = nf if final is None else final
        return self._fb[:nf]

    def sr_rows(self, effective: int, sr: int):
        """A source at another rate than 16 kHz on the HIP engine: (fbank rows `effective` samples resample to, how many of them are
        final), as the library counts them (ss_fbank_sr_rows) -- the rows from new_rows() on are then computed from the source-rate
        history in one launch (HipModel.batch_fbank_frames_sr) and committed with the final count.  None: the engine has no such call
        (the CPU oracle engine) or refuses the ratio (taps too large for a workgroup), and the whole history is resampled as before."""
        if not hasattr(self.engine, "batch_fbank_frames_sr"):
            return None
        return self.engine.fbank_sr_rows(effective, int(sr))

    def __call__(self, new_samples, sr=None):
        return self._rows(self.stage(new_samples), sr or self.sample_rate)

    def _rows(self, st, sr):
        """The device part of a call: the fbank rows of the staged history (st: what stage() / stage_pcm() returned)."""
        if st is None:
            return torch.empty((0, self.feature_dim), device=self.engine.device)
        num_frames, effective = st
        pcm = self._dev[:effective]
        if sr != SAMPLE_RATE:
            plan = self.sr_rows(effective, sr)
            if plan is None:
                pcm = self.engine.resample(pcm, int(sr), SAMPLE_RATE)
                return self.engine.fbank_cmvn(pcm, 32768.0)
            # The 16-kHz branch's scheme on the source-rate history: a row whose last sample's FIR window lies inside the audio received
            # so far never changes again (same taps, same order, same 400 samples), so rows final at the previous call come from the
            # cache and the rest -- the new rows and the one that still saw the zero padding -- are computed from self._dev directly.
            rows, final = plan
            if rows == 0:
                return torch.empty((0, self.feature_dim), device=self.engine.device)
            k = self.new_rows(rows)
            if rows > k:
                self.engine.batch_fbank_frames_sr([self._dev], [effective], [int(sr)], [k], [rows - k], [self._fb[k:rows]], 32768.0)
            return self.commit_rows(rows, final)
        if not hasattr(self.engine, "lib"):              # the CPU oracle engine: as the reference, everything every time
            return self.engine.fbank_cmvn(pcm, 32768.0)
        # A fbank row is a function of ITS 400 samples only (one workgroup per 25-ms frame, global CMVN): rows of the cached history stay
        # as they are and only the new frames are computed, into a buffer that grows by doubling.  Same bits as the full call
        # (tests/test_stages_gpu.py); the reference recomputes all frames per policy() call (agent :66-98).
        nf = num_frames
        k = self.new_rows(nf)
        if nf > k:
            self.engine.fbank_cmvn(self._dev[k * self.num_samples_per_shift:effective], 32768.0, out=self._fb[k:nf])
        return self.commit_rows(nf)
