"""Rendered clips as one playable file on the MI355X: what BodyRenderer.render_full_video of the reference's visualize/
render_codes.py does with mediapy and an ffmpeg subprocess (H.264 / AAC in MP4), as a baseline JPEG encoder on the GPU (csrc/
kernels_video.h) and a host-side AVI writer: Motion-JPEG with 16-bit PCM audio, which needs no inter-frame state and no codec
library, and which every desktop player and ffmpeg read.

`coefficients` is the first launch (a2p_jpeg_coefficients: colour transform, chroma subsampling, 8 x 8 DCT, quantisation; fp32, the
arithmetic of include/a2p_hip.h "video frames"), `entropy_segments` the second (a2p_jpeg_entropy: Huffman coding with one restart
interval per MCU row, sized and then written, so nothing is ever truncated).  `encode_jpeg_frames` returns complete JFIF files, one
per frame, in one host array; the uncompressed frames never leave the GPU.  `MJPEGWriter` / `write_video` put them into a RIFF AVI
with the recording's audio, `read_video` takes such a file apart again, and `render_codes_video` renders and writes a clip slice by
slice, so the frames of a long clip never exist at once.  The frames are uint8 tensors that live on the GPU; there is no CPU
encoder.

Differences from the reference, on purpose: MJPEG / PCM in AVI instead of H.264 / AAC in MP4 (about ten times the bytes per second
of video), no ffmpeg, and a file stays below 2 GiB (OpenDML `AVIX` segments are not written)."""
from __future__ import annotations

import os
import struct

import numpy as np
import torch

from . import _lib
from ._lib import A2PError

# ------------------------------------------------------------------------------------------------ the standard's tables (ITU-T T.81)
# Annex K.1, natural order
_Q_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
           103, 99)
_Q_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) \
    + (99,) * 32
# scan position -> natural index
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28, 35, 42, 49,
          56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)


def _rows(*firsts):
    """The regular tails of the AC tables: for every (run, first) the symbols (run, first) .. (run, 10) in order."""
    return tuple(run << 4 | size for run, first in firsts for size in range(first, 11))


# Annex K.3: (BITS: codes per length 1..16, HUFFVAL) of the DC / AC luminance and chrominance tables
_DC_LUMA = ((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0), tuple(range(12)))
_DC_CHROMA = ((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0), tuple(range(12)))
_AC_LUMA = ((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D),
            (0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
             0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18,
             0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A)
            + _rows((3, 4), (4, 3), (5, 3), (6, 3), (7, 3), (8, 3), (9, 2), (10, 2), (11, 2), (12, 2), (13, 2), (14, 1), (15, 1)))
_AC_CHROMA = ((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77),
              (0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
               0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25,
               0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A)
              + _rows((3, 5), (4, 3), (5, 3), (6, 3), (7, 3), (8, 2), (9, 2), (10, 2), (11, 2), (12, 2), (13, 2), (14, 2), (15, 2)))
HUFFMAN_SPECS = {"dc_luma": _DC_LUMA, "dc_chroma": _DC_CHROMA, "ac_luma": _AC_LUMA, "ac_chroma": _AC_CHROMA}
_SUBSAMPLING = {"420": (420, 16, 6), "444": (444, 8, 3)}     # name -> (C ABI value, MCU side, blocks per MCU)
AVI_LIMIT = (1 << 31) - (1 << 20)                            # bytes a file may reach (RIFF sizes of players that read them as int32)


def quant_tables(quality: int) -> np.ndarray:
    """uint16 [2, 64], luminance then chrominance, natural order: the Annex K tables scaled by libjpeg's rule (jpeg_quality_scaling,
    jpeg_add_quant_table with force_baseline): s = 5000 // q below 50, else 200 - 2 q; clip((base s + 50) // 100, 1, 255)."""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError(f"quality={quality} is outside [1, 100]")
    s = 5000 // q if q < 50 else 200 - 2 * q
    base = np.array([_Q_LUMA, _Q_CHROMA], np.int64)
    return np.clip((base * s + 50) // 100, 1, 255).astype(np.uint16)


def huffman_codes(bits, vals) -> dict:
    """{symbol: (code, length)} of a table given as BITS and HUFFVAL (Annex C: codes of one length count up, a longer length
    continues from twice the last code plus two)."""
    if len(bits) != 16 or sum(bits) != len(vals):
        raise ValueError("a Huffman table is 16 counts and as many symbols as they add up to")
    codes, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            codes[vals[k]] = (code, length)
            code, k = code + 1, k + 1
        code <<= 1
    return codes


def huffman_words() -> np.ndarray:
    """uint32 [544]: a2p_jpeg_entropy's `huff` (DC luminance and chrominance by category, 16 slots each; AC luminance and
    chrominance by symbol, 256 each), every entry (length << 16) | code, 0 where the table has no such symbol."""
    out = np.zeros(_lib.JPEG_HUFF_WORDS, np.uint32)
    for base, name in ((0, "dc_luma"), (16, "dc_chroma"), (32, "ac_luma"), (288, "ac_chroma")):
        for sym, (code, length) in huffman_codes(*HUFFMAN_SPECS[name]).items():
            out[base + sym] = (length << 16) | code
    return out


def _segment(marker: int, payload: bytes) -> bytes:
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def frame_header(height: int, width: int, quality: int = 90, subsampling: str = "420") -> bytes:
    """SOI, JFIF APP0, two DQT, SOF0, four DHT, DRI (one MCU row), SOS: everything in front of a frame's entropy-coded segment."""
    _, mcu, _ = _subsampling(subsampling)
    if not (1 <= int(height) <= _lib.JPEG_MAX_SIZE and 1 <= int(width) <= _lib.JPEG_MAX_SIZE):
        raise ValueError(f"a frame of {height} x {width} is outside [1, {_lib.JPEG_MAX_SIZE}]")
    q = quant_tables(quality)
    out = b"\xff\xd8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i in range(2):
        out += _segment(0xDB, bytes([i]) + bytes(int(q[i][n]) for n in ZIGZAG))
    sampling = 0x22 if mcu == 16 else 0x11
    out += _segment(0xC0, struct.pack(">BHHB", 8, int(height), int(width), 3) + bytes([1, sampling, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, name in ((0x00, "dc_luma"), (0x10, "ac_luma"), (0x01, "dc_chroma"), (0x11, "ac_chroma")):
        bits, vals = HUFFMAN_SPECS[name]
        out += _segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    out += _segment(0xDD, struct.pack(">H", (int(width) + mcu - 1) // mcu))
    return out + _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))


EOI = b"\xff\xd9"


def _subsampling(name):
    if str(name) not in _SUBSAMPLING:
        raise ValueError(f"subsampling={name!r}: need '420' or '444'")
    return _SUBSAMPLING[str(name)]


# ------------------------------------------------------------------------------------------------ the launches
_device_tables = {}


def _tables(device, quality=None):
    """(quantisation table for `quality`, Huffman words) on `device`, built once each."""
    key = (str(device), "huff")
    if key not in _device_tables:
        _device_tables[key] = torch.from_numpy(huffman_words().view(np.int32)).to(device)
    qt = None
    if quality is not None:
        qkey = (str(device), int(quality))
        if qkey not in _device_tables:
            _device_tables[qkey] = torch.from_numpy(quant_tables(quality).view(np.int16).copy()).to(device)
        qt = _device_tables[qkey]
    return qt, _device_tables[key]


def _frames_arg(frames):
    """A uint8 GPU tensor [N, H, W, 3] whose pixels are 3 dense bytes; rows and frames may be strided (a panel of a wider image)."""
    if not torch.is_tensor(frames):
        raise A2PError(f"frames must be a torch tensor on the GPU (got {type(frames).__name__})")
    _lib.require_gpu_tensor(frames, "frames")
    if frames.dtype != torch.uint8:
        raise A2PError(f"frames must be uint8 (got {frames.dtype})")
    if frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[1] < 1 or frames.shape[2] < 1:
        raise A2PError(f"frames must be [N, H, W, 3] with H, W >= 1 (got {list(frames.shape)})")
    N, H, W, _ = frames.shape
    if H > _lib.JPEG_MAX_SIZE or W > _lib.JPEG_MAX_SIZE:
        raise A2PError(f"frames of {H} x {W} exceed the format's {_lib.JPEG_MAX_SIZE}")
    sn, sh, sw, sc = frames.stride()
    if N and (sc != 1 or sw != 3 or (H > 1 and sh < 3 * W) or (N > 1 and sn < (H - 1) * sh + 3 * W)):
        frames = frames.contiguous()
    return frames


def mcu_grid(height: int, width: int, subsampling: str = "420"):
    """(mcu_rows, mcu_cols, blocks_per_mcu) of a frame."""
    _, mcu, bpm = _subsampling(subsampling)
    return (int(height) + mcu - 1) // mcu, (int(width) + mcu - 1) // mcu, bpm


def coefficients(frames, quality: int = 90, subsampling: str = "420"):
    """One launch of a2p_jpeg_coefficients: uint8 frames [N, H, W, 3] on the GPU (rows and frames may be strided) -> int16 [N,
    mcu_rows, mcu_cols, blocks_per_mcu, 64], the quantised coefficients in scan order."""
    code, _, _ = _subsampling(subsampling)
    quant_tables(quality)
    frames = _frames_arg(frames)
    N, H, W, _ = frames.shape
    rows, cols, bpm = mcu_grid(H, W, subsampling)
    dev = frames.device
    out = torch.empty(N, rows, cols, bpm, 64, dtype=torch.int16, device=dev)
    if N == 0:
        return out
    qt, _ = _tables(dev, quality)
    with _lib.on_device_of(frames):
        _lib.check(_lib.load().a2p_jpeg_coefficients(_lib.ptr(frames), N, H, W, frames.stride(0), frames.stride(1) if H > 1 else 3 * W, code,
                                                     _lib.ptr(qt), _lib.ptr(out), _lib.current_stream(dev)), "a2p_jpeg_coefficients")
    return out


def entropy_segments(coef, head: bytes = b"", tail: bytes = b"", gap: int = 0, slack: int = 0, fill: int = 0):
    """The two launches of a2p_jpeg_entropy: int16 coefficients [N, mcu_rows, mcu_cols, 3 or 6, 64] on the GPU -> (stream, offsets):
    a uint8 GPU tensor and an int64 host array [N + 1]; frame n is stream[offsets[n]:offsets[n + 1]] = head + its entropy-coded
    segment + tail.  gap: with an empty head, as many bytes in front of every segment that are left untouched; slack: bytes
    allocated behind the stream; both keep `fill` (for tests that look for stray writes).  Reading offsets back waits for the GPU
    once: the stream is allocated at its exact length."""
    if not torch.is_tensor(coef):
        raise A2PError(f"coef must be a torch tensor on the GPU (got {type(coef).__name__})")
    _lib.require_gpu_tensor(coef, "coef")
    if coef.dtype != torch.int16:
        raise A2PError(f"coef must be int16 (got {coef.dtype})")
    if coef.dim() != 5 or coef.shape[4] != 64 or coef.shape[3] not in (3, 6) or coef.shape[1] < 1 or coef.shape[2] < 1:
        raise A2PError(f"coef must be [N, mcu_rows, mcu_cols, 3 or 6, 64] (got {list(coef.shape)})")
    if head and gap:
        raise ValueError("gap goes with an empty head")
    coef = coef.contiguous()
    N, rows, cols, bpm, _ = coef.shape
    dev = coef.device
    _, huff = _tables(dev)
    lib = _lib.load()
    interval = torch.empty(max(N * rows, 1), dtype=torch.int64, device=dev)
    offsets = torch.empty(N + 1, dtype=torch.int64, device=dev)
    head_t = torch.frombuffer(bytearray(head), dtype=torch.uint8).to(dev) if head else None
    tail_t = torch.frombuffer(bytearray(tail), dtype=torch.uint8).to(dev) if tail else None
    n_head = len(head) if head else int(gap)

    def launch(out, out_bytes):
        _lib.check(lib.a2p_jpeg_entropy(_lib.ptr(coef), N, rows, cols, bpm, _lib.ptr(huff), _lib.ptr(head_t), n_head, _lib.ptr(tail_t),
                                        len(tail), _lib.ptr(interval), _lib.ptr(offsets), _lib.ptr(out), out_bytes,
                                        _lib.current_stream(dev)), "a2p_jpeg_entropy")
    with _lib.on_device_of(coef):
        launch(None, 0)
        host_offsets = offsets.cpu().numpy()
        total = int(host_offsets[N])
        stream = torch.full((total + int(slack),), int(fill), dtype=torch.uint8, device=dev)
        if N and total:
            launch(stream, total)
    return stream, host_offsets


def encode_jpeg_frames(frames, quality: int = 90, subsampling: str = "420", max_bytes: int = 1 << 28):
    """(data, offsets): uint8 and int64 [N + 1] host arrays; data[offsets[n]:offsets[n + 1]] is frame n as a complete baseline JFIF
    file, SOI to EOI.  frames: uint8 [N, H, W, 3] on the GPU; a row stride beyond 3 W is read in place.  The coefficients of at
    most max_bytes (at least one frame) exist at a time; the compressed frames are gathered on the GPU and copied to the host once."""
    frames = _frames_arg(frames)
    N, H, W, _ = frames.shape
    rows, cols, bpm = mcu_grid(H, W, subsampling)
    head = frame_header(H, W, quality, subsampling)
    chunk = max(1, int(max_bytes) // (rows * cols * bpm * 128))
    parts, offsets = [], [np.zeros(1, np.int64)]
    for a in range(0, N, chunk):
        stream, off = entropy_segments(coefficients(frames[a:a + chunk], quality, subsampling), head=head, tail=EOI)
        parts.append(stream)
        offsets.append(off[1:] + offsets[-1][-1])
    if not parts:
        return np.zeros(0, np.uint8), np.zeros(1, np.int64)
    data = (parts[0] if len(parts) == 1 else torch.cat(parts)).cpu().numpy()
    return data, np.concatenate(offsets)


# ------------------------------------------------------------------------------------------------ the container
def pcm16(audio) -> np.ndarray:
    """int16 [samples, channels]: rint(clip(x, -1, 1) 32767) of a float array [samples] or [samples, channels]; an int16 array is
    PCM already and is taken as it is."""
    a = np.asarray(audio.detach().cpu().numpy() if torch.is_tensor(audio) else audio)
    if a.ndim == 1:
        a = a[:, None]
    if a.ndim != 2 or a.shape[1] < 1 or not (np.issubdtype(a.dtype, np.floating) or a.dtype == np.int16):
        raise A2PError(f"audio must be a float (or int16) array [samples] or [samples, channels] (got {a.dtype} {list(a.shape)})")
    if a.dtype == np.int16:
        return a.astype("<i2")
    return np.rint(np.clip(a.astype(np.float64), -1.0, 1.0) * 32767.0).astype("<i2")


def wav_audio(path):
    """(audio, rate) of a PCM WAV file as MJPEGWriter takes it: 16-bit samples as they are stored (int16), other widths as floats in
    [-1, 1) (audio.read_wav returns the stored integers)."""
    import wave
    from .audio import read_wav
    values, rate = read_wav(os.fspath(path))
    with wave.open(os.fspath(path), "rb") as w:
        width = w.getsampwidth()
    if width == 2:
        return values.astype(np.int16), rate
    if width == 1:
        return (values.astype(np.float64) - 128.0) / 128.0, rate
    return values.astype(np.float64) / float(1 << (8 * width - 1)), rate


def _fps_fraction(fps):
    """(rate, scale) of an AVI stream header: fps itself when it is whole, else thousandths."""
    f = float(fps)
    if not (f > 0 and np.isfinite(f)):
        raise ValueError(f"fps={fps} must be positive")
    return (int(f), 1) if f == int(f) else (int(round(f * 1000)), 1000)


def _chunk(fourcc: bytes, payload: bytes) -> bytes:
    return fourcc + struct.pack("<I", len(payload)) + payload + (b"\x00" if len(payload) & 1 else b"")


class MJPEGWriter:
    """A RIFF AVI file with one Motion-JPEG stream and, when `audio` is given, one 16-bit PCM stream: `hdrl` (avih; strh + strf per
    stream), `movi` (`00dc` frames and `01wb` chunks of one video second of audio each, the audio of a second in front of its
    frames), `idx1`.  write(frames) encodes uint8 GPU frames [N, height, width, 3] and appends them, any number of times; close()
    writes the audio that is left (audio is never trimmed or stretched to the frames), the index and every size.  Before a write
    would take the finished file past AVI_LIMIT it raises ValueError and writes nothing: close() then finalises what is there."""

    def __init__(self, path, height: int, width: int, fps=30, quality: int = 90, subsampling: str = "420", audio=None, audio_rate=None):
        _subsampling(subsampling)
        quant_tables(quality)
        frame_header(height, width, quality, subsampling)
        self.path, self.height, self.width = os.fspath(path), int(height), int(width)
        self.quality, self.subsampling = int(quality), str(subsampling)
        self.rate, self.scale = _fps_fraction(fps)
        self.audio = None
        if audio is not None:
            if audio_rate is None or int(audio_rate) != audio_rate or int(audio_rate) < 1:
                raise ValueError(f"audio takes audio_rate, a positive whole number of samples per second (got {audio_rate})")
            self.audio, self.audio_rate = pcm16(audio), int(audio_rate)
            self.channels = self.audio.shape[1]
        self.frames = 0
        self._audio_done = 0                 # samples written
        self._second = 0                     # video seconds whose audio is written
        self._index = []                     # (fourcc, offset from the `movi` fourcc, size)
        self._max_frame = self._max_audio = 0
        self._f = open(self.path, "wb")
        self._f.write(self._headers())
        self._movi = self._f.tell() - 4      # position of the `movi` fourcc
        self._closed = False

    # -- layout
    def _headers(self) -> bytes:
        usec = int(round(1e6 * self.scale / self.rate))
        streams = 1 if self.audio is None else 2
        audio_bps = 0 if self.audio is None else self.audio_rate * self.channels * 2
        per_sec = int(self._max_frame * self.rate / self.scale) + audio_bps
        avih = struct.pack("<14I", usec, per_sec, 0, 0x10 | 0x100, self.frames, 0, streams, self._max_frame, self.width, self.height, 0, 0, 0, 0)
        strh = b"vids" + b"MJPG" + struct.pack("<IHHIIIIIIiI4h", 0, 0, 0, 0, self.scale, self.rate, 0, self.frames, self._max_frame, -1, 0,
                                               0, 0, self.width, self.height)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3, 0, 0, 0, 0)
        hdrl = b"hdrl" + _chunk(b"avih", avih) + _chunk(b"LIST", b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf))
        if self.audio is not None:
            align = 2 * self.channels
            strh = b"auds" + struct.pack("<IIHHIIIIIIiI4h", 0, 0, 0, 0, 0, align, self.audio_rate * align, 0, self.audio.shape[0],
                                         self._max_audio, -1, align, 0, 0, 0, 0)
            strf = struct.pack("<HHIIHHH", 1, self.channels, self.audio_rate, self.audio_rate * align, align, 16, 0)
            hdrl += _chunk(b"LIST", b"strl" + _chunk(b"strh", strh) + _chunk(b"strf", strf))
        movi_size = 4 + sum(8 + size + (size & 1) for _, _, size in self._index)
        head = _chunk(b"LIST", hdrl) + b"LIST" + struct.pack("<I", movi_size) + b"movi"
        riff_size = 4 + len(head) + movi_size - 4 + (8 + 16 * len(self._index))
        return b"RIFF" + struct.pack("<I", riff_size) + b"AVI " + head

    def _put(self, fourcc: bytes, payload) -> None:
        self._index.append((fourcc, self._f.tell() - self._movi, len(payload)))
        self._f.write(fourcc + struct.pack("<I", len(payload)))
        self._f.write(payload)
        if len(payload) & 1:
            self._f.write(b"\x00")

    def _audio_chunks(self, done: int, second: int, until: int):
        """([a, b) sample ranges of the audio chunks of video seconds second .. until - 1 that hold samples beyond `done`, the new
        `done`)."""
        out = []
        for k in range(second, until):
            b = min(self.audio.shape[0], (k + 1) * self.audio_rate)
            if b > done:
                out.append((done, b))
                done = b
        return out, done

    def _audio_rest(self, done: int):
        n = 0 if self.audio is None else self.audio.shape[0]
        return [(a, min(n, a + self.audio_rate)) for a in range(done, n, self.audio_rate)] if n > done else []

    def _second_of(self, frame: int) -> int:
        return frame * self.scale // self.rate

    # -- writing
    def write(self, frames) -> int:
        """Encodes and appends uint8 GPU frames [N, height, width, 3]; returns how many frames the file holds."""
        if self._closed:
            raise ValueError(f"{self.path} is closed")
        frames = _frames_arg(frames)
        if tuple(frames.shape[1:3]) != (self.height, self.width):
            raise A2PError(f"the file holds frames of {self.height} x {self.width} (got {list(frames.shape)})")
        data, off = encode_jpeg_frames(frames, self.quality, self.subsampling)
        N = len(off) - 1
        # the plan of this call: [(fourcc, payload)] in file order, and the audio left for close()
        plan, done, second = [], self._audio_done, self._second
        for i in range(N):
            need = self._second_of(self.frames + i) + 1
            if self.audio is not None and need > second:
                ranges, done = self._audio_chunks(done, second, need)
                plan += [(b"01wb", self.audio[a:b].tobytes()) for a, b in ranges]
                second = need
            plan.append((b"00dc", data[off[i]:off[i + 1]]))
        size = lambda n: 8 + n + (n & 1) + 16                      # a chunk and its index entry
        rest = sum(size((b - a) * 2 * self.channels) for a, b in self._audio_rest(done))
        end = self._f.tell() + sum(size(len(p)) for _, p in plan) + rest + 16 * len(self._index) + 8
        if end > AVI_LIMIT:
            raise ValueError(f"{N} more frames would take {self.path} to {end} bytes, past {AVI_LIMIT}: close this file and start another "
                             "(OpenDML files beyond 2 GiB are not written)")
        for fourcc, payload in plan:
            self._put(fourcc, payload)
            if fourcc == b"00dc":
                self._max_frame = max(self._max_frame, len(payload))
            else:
                self._max_audio = max(self._max_audio, len(payload))
        self._second, self._audio_done = second, done
        self.frames += N
        return self.frames

    def close(self) -> None:
        if self._closed:
            return
        for a, b in self._audio_rest(self._audio_done):
            payload = self.audio[a:b].tobytes()
            self._put(b"01wb", payload)
            self._max_audio = max(self._max_audio, len(payload))
            self._audio_done = b
        self._f.write(b"idx1" + struct.pack("<I", 16 * len(self._index)))
        for fourcc, offset, size in self._index:
            self._f.write(fourcc + struct.pack("<III", 0x10, offset, size))
        self._f.seek(0)
        self._f.write(self._headers())
        self._f.close()
        self._closed = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def write_video(path, frames, fps=30, quality: int = 90, subsampling: str = "420", audio=None, audio_rate=None, slice_frames: int = 64) -> int:
    """Writes uint8 GPU frames [N, H, W, 3] (and float audio [samples] or [samples, channels] at audio_rate) to the AVI file
    `path`, slice_frames frames at a time; returns the number of frames."""
    frames = _frames_arg(frames)
    with MJPEGWriter(path, frames.shape[1], frames.shape[2], fps, quality, subsampling, audio, audio_rate) as w:
        for a in range(0, frames.shape[0], max(1, int(slice_frames))):
            w.write(frames[a:a + max(1, int(slice_frames))])
    return int(frames.shape[0])


def read_video(path) -> dict:
    """Takes an AVI file of MJPEGWriter apart: {"frames": [bytes] (one JFIF file each), "fps": float, "size": (height, width),
    "audio": int16 [samples] or [samples, channels] or None, "audio_rate": int or None}.  Reads the `movi` list chunk by chunk."""
    blob = open(os.fspath(path), "rb").read()
    if len(blob) < 12 or blob[:4] != b"RIFF" or blob[8:12] != b"AVI ":
        raise ValueError(f"{path} is not a RIFF AVI file")
    out = {"frames": [], "fps": None, "size": None, "audio": None, "audio_rate": None}
    audio, channels, kinds = [], None, []

    def walk(a, b, inside):
        nonlocal channels
        while a + 8 <= b:
            fourcc, size = blob[a:a + 4], struct.unpack_from("<I", blob, a + 4)[0]
            body = a + 8
            if body + size > b:
                raise ValueError(f"{path}: chunk {fourcc!r} at {a} runs past its list")
            if fourcc == b"LIST":
                walk(body + 4, body + size, blob[body:body + 4])
            elif fourcc == b"strh":
                kinds.append(blob[body:body + 4])
                if kinds[-1] == b"vids":
                    scale, rate = struct.unpack_from("<II", blob, body + 20)
                    out["fps"] = rate / scale
            elif fourcc == b"strf" and kinds and kinds[-1] == b"vids":
                w, h = struct.unpack_from("<ii", blob, body + 4)
                out["size"] = (h, w)
            elif fourcc == b"strf" and kinds and kinds[-1] == b"auds":
                tag, channels, rate, _, _, width = struct.unpack_from("<HHIIHH", blob, body)
                if tag != 1 or width != 16:
                    raise ValueError(f"{path}: the audio is format {tag} with {width} bits; 16-bit PCM is read")
                out["audio_rate"] = rate
            elif inside == b"movi" and fourcc[2:] == b"dc":
                out["frames"].append(blob[body:body + size])
            elif inside == b"movi" and fourcc[2:] == b"wb":
                audio.append(blob[body:body + size])
            a = body + size + (size & 1)

    walk(12, min(len(blob), 8 + struct.unpack_from("<I", blob, 4)[0]), b"AVI ")
    if channels is not None:
        pcm = np.frombuffer(b"".join(audio), "<i2").reshape(-1, channels)
        out["audio"] = pcm[:, 0].copy() if channels == 1 else pcm.copy()
    return out


# ------------------------------------------------------------------------------------------------ rendering into a file
def render_codes_video(face_decoder, face_encoder, body_encoder, decoder, texture, skeleton, rasterizer, poses, face_codes, K, Rt, path,
                       audio=None, audio_rate=None, fps=30, quality: int = 90, subsampling: str = "420", slice_frames: int = 32, **kw) -> int:
    """encoder.render_codes_motion over slices of slice_frames frames of the time axis, every slice encoded and appended to the AVI
    file `path` before the next is rendered: BodyRenderer.render_full_video.  poses [T, P] (or [1, T, P]) and face_codes with the
    same leading axes: one sequence per file; **kw goes to render_codes_motion (camera_pos, body_embs, max_bytes).  A frame's bytes
    do not depend on the slicing.  Returns the number of frames."""
    from .encoder import render_codes_motion
    poses, face_codes = torch.as_tensor(poses), torch.as_tensor(face_codes)
    if poses.dim() == 3 and poses.shape[0] == 1 and face_codes.dim() == 3 and face_codes.shape[0] == 1:
        poses, face_codes = poses[0], face_codes[0]
    if poses.dim() != 2 or face_codes.dim() != 2 or poses.shape[0] != face_codes.shape[0]:
        raise A2PError(f"poses and face_codes must be [T, .] (or [1, T, .]) of one sequence with the same T (got {list(poses.shape)} and "
                       f"{list(face_codes.shape)})")
    C = torch.as_tensor(K).shape[0]
    step = max(1, int(slice_frames))
    with MJPEGWriter(path, rasterizer.height, C * rasterizer.width, fps, quality, subsampling, audio, audio_rate) as w:
        for a in range(0, poses.shape[0], step):
            w.write(render_codes_motion(face_decoder, face_encoder, body_encoder, decoder, texture, skeleton, rasterizer, poses[a:a + step],
                                        face_codes[a:a + step], K, Rt, **kw))
    return int(poses.shape[0])


def sequence_path(path: str, index: int, count: int) -> str:
    """`path` itself for a single sequence, else `stem_<index>.ext`."""
    if count == 1:
        return path
    stem, ext = os.path.splitext(path)
    return f"{stem}_{index:02d}{ext}"


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m audio2photoreal_amd.video",
                                 description="uint8 frames (and a wav file) to a Motion-JPEG AVI file, encoded on the MI355X.")
    ap.add_argument("--frames", required=True, help="frames.npy: uint8 [T, H, W, 3] or [R, T, H, W, 3] (what python -m "
                    "audio2photoreal_amd.encoder writes); R > 1 sequences go to <out stem>_<r>.avi")
    ap.add_argument("--audio", default=None, metavar="FILE", help="a wav file; it is written as 16-bit PCM at its own rate, untrimmed")
    ap.add_argument("--out", required=True, help="the AVI file")
    ap.add_argument("--fps", type=float, default=30)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--subsampling", choices=("420", "444"), default="420")
    ap.add_argument("--slice-frames", type=int, default=64, help="frames on the GPU at a time")
    args = ap.parse_args(argv)
    frames = np.load(args.frames, mmap_mode="r")
    if frames.dtype != np.uint8 or frames.ndim not in (4, 5) or frames.shape[-1] != 3:
        raise A2PError(f"{args.frames} must hold uint8 [T, H, W, 3] or [R, T, H, W, 3] (got {frames.dtype} {list(frames.shape)})")
    if not torch.cuda.is_available():
        raise A2PError("the frames are encoded on the MI355X; there is no CPU implementation")
    if frames.ndim == 4:
        frames = frames[None]
    audio, rate = wav_audio(args.audio) if args.audio is not None else (None, None)
    step = max(1, args.slice_frames)
    for r in range(frames.shape[0]):
        path = sequence_path(args.out, r, frames.shape[0])
        with MJPEGWriter(path, frames.shape[2], frames.shape[3], args.fps, args.quality, args.subsampling, audio, rate) as w:
            for a in range(0, frames.shape[1], step):
                w.write(torch.from_numpy(np.array(frames[r, a:a + step])).to("cuda"))
        print(f"{path}: {frames.shape[1]} frames of {frames.shape[2]} x {frames.shape[3]} at {args.fps:g} fps, {os.path.getsize(path)} bytes")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
