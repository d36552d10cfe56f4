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

The way back (csrc/kernels_video_decode.h): `parse_jpeg_header` reads a file's marker segments on the host, `decode_coefficients` is
the integer stage (a2p_jpeg_restarts finds the restart intervals, a2p_jpeg_decode_entropy decodes one interval per lane; exact) and
`pixels` the arithmetic one (a2p_jpeg_pixels: dequantisation, inverse DCT, chroma replication, colour transform; fp32).
`decode_jpeg_frames` turns JFIF files into uint8 GPU frames, `MJPEGReader` / `read_video_frames` do so for an AVI file, indexed
through mmap and decoded slice by slice; only compressed bytes go to the GPU, and there is no CPU decoder.

Differences from the reference, on purpose: MJPEG / PCM in AVI instead of H.264 / AAC in MP4 (about ten times the bytes per second
of video), no ffmpeg, and a file stays below 2 GiB (OpenDML `AVIX` segments are not written)."""
from __future__ import annotations

import os
import struct

import numpy as np
import torch

from . import _lib, avatar
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


# ------------------------------------------------------------------------------------------------ reading: headers on the host
SAMPLINGS = {"444": (3, 1, 1, 3), "422": (3, 2, 1, 4), "420": (3, 2, 2, 6), "gray": (1, 1, 1, 1)}   # name -> (components, luma h, luma v, blocks per MCU)
_SOF_NAMES = {0xC1: "extended sequential DCT (SOF1)", 0xC2: "progressive DCT (SOF2)", 0xC3: "lossless (SOF3)",
              0xC5: "differential sequential DCT (SOF5)", 0xC6: "differential progressive DCT (SOF6)", 0xC7: "differential lossless (SOF7)",
              0xC9: "arithmetic-coded sequential DCT (SOF9)", 0xCA: "arithmetic-coded progressive DCT (SOF10)",
              0xCB: "arithmetic-coded lossless (SOF11)", 0xCD: "arithmetic-coded differential sequential DCT (SOF13)",
              0xCE: "arithmetic-coded differential progressive DCT (SOF14)", 0xCF: "arithmetic-coded differential lossless (SOF15)"}
DEFAULT_DHT = {0x00: _DC_LUMA, 0x10: _AC_LUMA, 0x01: _DC_CHROMA, 0x11: _AC_CHROMA}     # Tc << 4 | Th -> (BITS, HUFFVAL) of Annex K


def parse_jpeg_header(data) -> dict:
    """The marker segments of one baseline JPEG file (bytes or a uint8 array), read on the host: {"size": (H, W), "components": [(id,
    h, v, tq)], "sampling": "444" | "422" | "420" | "gray", "dqt": {id: uint16 [64] in scan order}, "dht": {Tc << 4 | Th: (BITS,
    HUFFVAL)}, "default_dht": True when the file carries no DHT and the Annex K tables stand in (the AVI MJPEG convention), "dri":
    the restart interval in MCUs (0: none), "scan": [(id, td, ta)], "segment": (begin, end) of the entropy-coded segment, "order":
    the marker codes in file order}.  Read: 8-bit baseline (SOF0) with one component, or three with luminance sampled 1 x 1, 2 x 1 or
    2 x 2 over 1 x 1 chrominance, in one scan.  Everything else raises A2PError with the name of what the file asks for."""
    d = data if isinstance(data, bytes) else bytes(data)
    n = len(d)
    if n < 4 or d[0] != 0xFF or d[1] != 0xD8:
        raise A2PError("not a JPEG file: it does not start with SOI")
    out = {"dqt": {}, "dht": {}, "dri": 0, "order": [0xD8], "size": None, "components": None, "default_dht": False}
    at = 2
    while True:
        if at + 4 > n or d[at] != 0xFF:
            raise A2PError(f"no marker at byte {at} (the file ends before SOS, or fill bytes precede a marker)")
        code, length = d[at + 1], d[at + 2] << 8 | d[at + 3]
        if length < 2 or at + 2 + length > n:
            raise A2PError(f"the segment of marker {code:#x} at byte {at} runs past the file")
        body = bytes(d[at + 4:at + 2 + length])
        out["order"].append(code)
        if code == 0xDB:
            while body:
                if body[0] >> 4:
                    raise A2PError("16-bit quantisation tables are not read (8-bit baseline JPEG is)")
                if len(body) < 65:
                    raise A2PError("a DQT segment is cut short")
                out["dqt"][body[0] & 15] = np.frombuffer(body[1:65], np.uint8).astype(np.uint16)
                body = body[65:]
        elif code == 0xC4:
            while body:
                bits = tuple(body[1:17])
                if len(body) < 17 or len(body) < 17 + sum(bits):
                    raise A2PError("a DHT segment is cut short")
                if body[0] >> 4 > 1 or body[0] & 15 > 1:
                    raise A2PError(f"Huffman table {body[0]:#x}: baseline JPEG holds DC and AC tables 0 and 1")
                out["dht"][body[0]] = (bits, tuple(body[17:17 + sum(bits)]))
                body = body[17 + sum(bits):]
        elif code == 0xC0:
            if len(body) < 6 or len(body) < 6 + 3 * body[5]:
                raise A2PError("the SOF0 segment is cut short")
            if body[0] != 8:
                raise A2PError(f"{body[0]}-bit samples are not read (8-bit baseline JPEG is)")
            out["size"] = (body[1] << 8 | body[2], body[3] << 8 | body[4])
            out["components"] = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(body[5])]
        elif code in _SOF_NAMES:
            raise A2PError(f"{_SOF_NAMES[code]} JPEG is not read (baseline sequential Huffman-coded SOF0 is)")
        elif code == 0xDD:
            if len(body) != 2:
                raise A2PError("a DRI segment of the wrong length")
            out["dri"] = body[0] << 8 | body[1]
        elif code == 0xDA:
            if out["components"] is None:
                raise A2PError("SOS comes before SOF0")
            break
        elif not (0xE0 <= code <= 0xEF or code == 0xFE):
            raise A2PError(f"marker {code:#x} is not part of baseline JPEG")
        at += 2 + length
    comps = out["components"]
    if len(comps) not in (1, 3):
        raise A2PError(f"{len(comps)} components are not read (grayscale and three-component YCbCr are)")
    if out["size"][0] < 1 or out["size"][1] < 1:
        raise A2PError(f"a frame of {out['size'][0]} x {out['size'][1]} (a height given by DNL is not read)")
    if len(comps) == 1:
        out["sampling"] = "gray"
    else:
        luma = comps[0][1:3]
        if comps[1][1:3] != (1, 1) or comps[2][1:3] != (1, 1) or luma not in ((1, 1), (2, 1), (2, 2)):
            raise A2PError(f"sampling factors {[c[1:3] for c in comps]} are not read (luminance 1 x 1, 2 x 1 or 2 x 2 over 1 x 1 "
                           "chrominance is: 4:4:4, 4:2:2, 4:2:0)")
        out["sampling"] = {(1, 1): "444", (2, 1): "422", (2, 2): "420"}[luma]
    if len(body) < 1 or body[0] != len(comps) or len(body) != 4 + 2 * len(comps):
        raise A2PError(f"a scan of {body[0] if body else 0} of the {len(comps)} components is not read (one interleaved scan is)")
    out["scan"] = [(body[1 + 2 * i], body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(body[0])]
    if tuple(body[-3:]) != (0, 63, 0):
        raise A2PError("a scan with spectral selection or successive approximation is not read (a sequential scan is)")
    if [s[0] for s in out["scan"]] != [c[0] for c in comps]:
        raise A2PError("the scan lists the components in another order than the frame")
    if not out["dht"]:
        out["dht"], out["default_dht"] = dict(DEFAULT_DHT), True
    for cid, td, ta in out["scan"]:
        if td > 1 or ta > 1 or td not in out["dht"] or (0x10 | ta) not in out["dht"]:
            raise A2PError(f"component {cid} uses Huffman tables DC {td} / AC {ta}, which the file does not define")
    for c in comps:
        if c[3] not in out["dqt"]:
            raise A2PError(f"component {c[0]} uses quantisation table {c[3]}, which the file does not define")
    begin = at + 2 + length
    end = d.rfind(b"\xff\xd9", begin)
    out["segment"] = (begin, end if end >= 0 else n)
    if end >= 0:
        out["order"].append(0xD9)
    return out


def decoder_table(bits, vals) -> np.ndarray:
    """int32 [JPEG_TABLE_WORDS]: a Huffman table as a2p_jpeg_decode_entropy takes it: maxcode[16], offset[16], the symbols as bytes."""
    if len(bits) != 16 or sum(bits) != len(vals) or len(vals) > 256:
        raise A2PError("a Huffman table is 16 counts and as many symbols, at most 256, as they add up to")
    t = np.zeros(_lib.JPEG_TABLE_WORDS, np.int32)
    code = k = 0
    for length in range(1, 17):
        t[length - 1] = -1
        if bits[length - 1]:
            t[16 + length - 1] = k - code
            code, k = code + bits[length - 1], k + bits[length - 1]
            if code > 1 << length:
                raise A2PError(f"a Huffman table with {bits[length - 1]} codes of {length} bits is no prefix code")
            t[length - 1] = code - 1
        code <<= 1
    t[32:].view(np.uint8)[:len(vals)] = np.asarray(vals, np.uint8)
    return t


def _decoder_tables(header) -> np.ndarray:
    t = np.zeros((_lib.JPEG_TABLES, _lib.JPEG_TABLE_WORDS), np.int32)
    t[:, :16] = -1
    for key, (bits, vals) in header["dht"].items():
        t[(key >> 4) * 2 + (key & 15)] = decoder_table(bits, vals)
    return t


def _header_key(h):
    return (h["size"], tuple(h["components"]), h["dri"], tuple(h["scan"]), tuple(sorted((k, v.tobytes()) for k, v in h["dqt"].items())),
            tuple(sorted(h["dht"].items())))


def header_qtabs(header) -> np.ndarray:
    """uint16 [components, 64]: the quantisation table of every component, in scan order, as `pixels` takes them."""
    return np.stack([header["dqt"][c[3]] for c in header["components"]]).astype(np.uint16)


def _jpeg_files(data, offsets):
    """(buffer, int64 [N + 1]): a list of bytes, or one uint8 array with offsets, as one host buffer."""
    if offsets is None:
        if isinstance(data, (bytes, bytearray, memoryview)):
            data = [data]
        files = [bytes(f) for f in data]
        off = np.zeros(len(files) + 1, np.int64)
        np.cumsum([len(f) for f in files], out=off[1:])
        return b"".join(files), off
    off = np.asarray(offsets, np.int64)
    buf = data.detach().cpu().numpy() if torch.is_tensor(data) else np.asarray(data)
    if buf.dtype != np.uint8 or buf.ndim != 1 or off.ndim != 1 or len(off) < 1 or (np.diff(off) < 0).any() or off[0] < 0 or off[-1] > len(buf):
        raise A2PError("data with offsets must be one uint8 array and ascending int64 offsets [N + 1] inside it")
    return buf.tobytes(), off


def _parse_all(buf, off):
    """The header of every file; a file whose bytes up to the segment equal its predecessor's shares that header's tables."""
    view, out, prev = memoryview(buf), [], None
    for n in range(len(off) - 1):
        a, b = int(off[n]), int(off[n + 1])
        if prev is not None and b - a >= prev[1] and view[a:a + prev[1]] == prev[0]:
            h = dict(out[-1])
            end = buf.rfind(b"\xff\xd9", a + prev[1], b)
            h["segment"] = (prev[1], end - a if end >= 0 else b - a)
        else:
            try:
                h = parse_jpeg_header(view[a:b])
            except A2PError as e:
                raise A2PError(f"frame {n}: {e}") from None
            prev = (bytes(view[a:a + h["segment"][0]]), h["segment"][0])
        out.append(h)
    return out


def _device_of(device):
    if not torch.cuda.is_available():
        raise A2PError("the frames are decoded on the MI355X; there is no CPU implementation")
    return torch.device("cuda" if device is None else device)


def _status_text(word):
    return f"interval {int(word) >> 4}: {_lib.JPEG_CAUSES.get(int(word) & 15, 'cause %d' % (int(word) & 15))}"


def decode_grid(header):
    """(mcu_rows, mcu_cols, blocks_per_mcu) of a parsed header."""
    _, hs, vs, bpm = SAMPLINGS[header["sampling"]]
    return -(-header["size"][0] // (8 * vs)), -(-header["size"][1] // (8 * hs)), bpm


# ------------------------------------------------------------------------------------------------ reading: the launches
def _entropy_stage(segments, header, dev):
    """a2p_jpeg_restarts and a2p_jpeg_decode_entropy over the entropy-coded segments (bytes-likes) of frames that share `header`:
    (coef int16 [n, mcu_rows, mcu_cols, blocks_per_mcu, 64], status int32 [2, n]: the scan's and the decoder's) on dev.  The bytes go
    to the GPU in one copy; nothing is read back."""
    rows, cols, bpm = decode_grid(header)
    intervals = -(-rows * cols // header["dri"]) if header["dri"] else 1
    n = len(segments)
    ends = np.cumsum([len(s) for s in segments], dtype=np.int64)
    segs = np.stack([ends - np.array([len(s) for s in segments], np.int64), ends], 1)
    data = torch.frombuffer(bytearray().join(segments) or bytearray(1), dtype=torch.uint8).to(dev)
    key = (str(dev), "decoder", _header_key(header)[5])
    if key not in _device_tables:
        _device_tables[key] = torch.from_numpy(_decoder_tables(header)).to(dev)
    tables = _device_tables[key]
    selectors = sum((td << i) | (ta << (4 + i)) for i, (_, td, ta) in enumerate(header["scan"]))
    seg_t = torch.from_numpy(segs).to(dev)
    ranges = torch.empty(n, intervals + 1, dtype=torch.int64, device=dev)
    status = torch.empty(2, n, dtype=torch.int32, device=dev)
    coef = torch.empty(n, rows, cols, bpm, 64, dtype=torch.int16, device=dev)
    lib = _lib.load()
    with torch.cuda.device(dev):
        stream = _lib.current_stream(dev)
        _lib.check(lib.a2p_jpeg_restarts(_lib.ptr(data), int(ends[-1]), _lib.ptr(seg_t), n, intervals, _lib.ptr(ranges), _lib.ptr(status[0]),
                                         stream), "a2p_jpeg_restarts")
        _lib.check(lib.a2p_jpeg_decode_entropy(_lib.ptr(data), int(ends[-1]), _lib.ptr(ranges), _lib.ptr(status[0]), n, rows, cols, bpm,
                                               header["dri"], _lib.ptr(tables), selectors, _lib.ptr(coef), _lib.ptr(status[1]), stream),
                   "a2p_jpeg_decode_entropy")
    return coef, status


def _bad_frames(status):
    """[(index, status word)] of the frames a status array [2, n] (on the host) marks; the scan's verdict comes first."""
    return [(i, int(status[0, i] or status[1, i])) for i in np.nonzero((status != 0).any(0))[0]]


def decode_coefficients(data, offsets=None, device=None):
    """The integer stage: a list of JFIF files as bytes (or one uint8 array with `offsets` [N + 1], as encode_jpeg_frames returns them)
    that share one header -> (coef, header): int16 [N, mcu_rows, mcu_cols, blocks_per_mcu, 64] on the GPU, the quantised coefficients
    in scan order (what `coefficients` writes and `entropy_segments` reads), and the parsed header of the first file.  Exact: entropy
    coding is lossless.  A frame the decoder rejects raises A2PError naming the frame, the restart interval and the cause."""
    buf, off = _jpeg_files(data, offsets)
    dev = _device_of(device)
    headers = _parse_all(buf, off)
    if not headers:
        raise A2PError("decode_coefficients needs at least one file")
    if any(_header_key(h) != _header_key(headers[0]) for h in headers[1:]):
        raise A2PError("decode_coefficients takes files that share one header (size, sampling, tables); decode_jpeg_frames groups mixed ones")
    view = memoryview(buf)
    segments = [view[int(off[n]) + h["segment"][0]:int(off[n]) + h["segment"][1]] for n, h in enumerate(headers)]
    coef, status = _entropy_stage(segments, headers[0], dev)
    bad = _bad_frames(status.cpu().numpy())
    if bad:
        raise A2PError(f"frame {bad[0][0]} is rejected: {_status_text(bad[0][1])}" + (f" ({len(bad)} frames in all)" if len(bad) > 1 else ""))
    return coef, headers[0]


def _out_arg(out, N, H, W, dev):
    if out is None:
        return torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)
    if not torch.is_tensor(out) or not out.is_cuda or out.dtype != torch.uint8 or tuple(out.shape) != (N, H, W, 3):
        raise A2PError(f"out must be a uint8 GPU tensor [{N}, {H}, {W}, 3] (got {type(out).__name__} "
                       f"{list(out.shape) if torch.is_tensor(out) else ''})")
    sn, sh, sw, sc = out.stride()
    if N and (sc != 1 or sw != 3 or (H > 1 and sh < 3 * W) or (N > 1 and sn < (H - 1) * sh + 3 * W)):
        raise A2PError(f"out must hold pixels of 3 dense bytes, rows at least 3 W bytes apart and frames that do not overlap (strides {out.stride()})")
    return out


def pixels(coef, height: int, width: int, qtabs, sampling: str = "420", out=None):
    """The arithmetic stage, one launch of a2p_jpeg_pixels: int16 coefficients [N, mcu_rows, mcu_cols, blocks_per_mcu, 64] on the GPU
    -> uint8 frames [N, height, width, 3].  qtabs: uint16 [components, 64] in scan order, one table per component (header_qtabs);
    sampling: "444", "422", "420" or "gray".  out: a uint8 GPU tensor [N, height, width, 3] whose rows and frames may be strided (a
    column window of a wider image): only the window is written."""
    if str(sampling) not in SAMPLINGS:
        raise A2PError(f"sampling={sampling!r}: need one of {sorted(SAMPLINGS)}")
    ncomp, hs, vs, bpm = SAMPLINGS[str(sampling)]
    if not torch.is_tensor(coef):
        raise A2PError(f"coef must be a torch tensor on the GPU (got {type(coef).__name__})")
    _lib.require_gpu_tensor(coef, "coef")
    H, W = int(height), int(width)
    if not (1 <= H <= _lib.JPEG_MAX_SIZE and 1 <= W <= _lib.JPEG_MAX_SIZE):
        raise A2PError(f"a frame of {height} x {width} is outside [1, {_lib.JPEG_MAX_SIZE}]")
    want = (-(-H // (8 * vs)), -(-W // (8 * hs)), bpm, 64)
    if coef.dtype != torch.int16 or coef.dim() != 5 or tuple(coef.shape[1:]) != want:
        raise A2PError(f"coef must be int16 [N, {want[0]}, {want[1]}, {bpm}, 64] for {H} x {W} frames sampled {sampling} (got {coef.dtype} "
                       f"{list(coef.shape)})")
    q = qtabs.detach().cpu().numpy() if torch.is_tensor(qtabs) else np.asarray(qtabs)
    if q.shape != (ncomp, 64) or not np.issubdtype(q.dtype, np.integer) or q.min() < 1 or q.max() > 255:
        raise A2PError(f"qtabs must be [{ncomp}, 64] integers in [1, 255], one table per component in scan order (got {list(q.shape)})")
    coef = coef.contiguous()
    N, dev = coef.shape[0], coef.device
    out = _out_arg(out, N, H, W, dev)
    if N == 0:
        return out
    key = (str(dev), "dequant", q.astype(np.uint16).tobytes())
    if key not in _device_tables:
        _device_tables[key] = torch.from_numpy(q.astype(np.int16)).to(dev)
    with _lib.on_device_of(coef):
        _lib.check(_lib.load().a2p_jpeg_pixels(_lib.ptr(coef), N, H, W, ncomp, hs, vs, _lib.ptr(_device_tables[key]), _lib.ptr(out),
                                               out.stride(0) if N > 1 else (H - 1) * out.stride(1) + 3 * W, out.stride(1) if H > 1 else 3 * W,
                                               _lib.current_stream(dev)), "a2p_jpeg_pixels")
    return out


def decode_jpeg_frames(data, offsets=None, out=None, max_bytes: int = 1 << 28, on_error: str = "raise", device=None):
    """Baseline JPEG files -> uint8 frames [N, H, W, 3] on the GPU.  data: a list of bytes, one JFIF file each, or one uint8 array with
    `offsets` [N + 1] as encode_jpeg_frames returns them.  All frames share one size; frames with identical headers go through one
    set of launches (a2p_jpeg_restarts, a2p_jpeg_decode_entropy, a2p_jpeg_pixels), frames with other tables are grouped by header.
    The coefficients of at most max_bytes (at least one frame) exist at a time; per slice the entropy-coded bytes go to the GPU in
    one copy, and the status of every frame comes back in one read at the end.  out: a uint8 GPU tensor [N, H, W, 3], rows and
    frames may be strided.  A frame the decoder rejects raises A2PError naming the frame, the restart interval and the cause;
    on_error="mark" returns (frames, [bad indices]) instead, the bad frames zeroed.  A frame's bytes depend on that frame alone."""
    if on_error not in ("raise", "mark"):
        raise ValueError(f"on_error={on_error!r}: need 'raise' or 'mark'")
    buf, off = _jpeg_files(data, offsets)
    dev = _device_of(device if out is None or not torch.is_tensor(out) else out.device)
    headers = _parse_all(buf, off)
    N = len(headers)
    if N == 0:
        if out is None:
            raise A2PError("decode_jpeg_frames needs at least one file (the frame size comes from the files)")
        return (out, []) if on_error == "mark" else out
    H, W = headers[0]["size"]
    for n, h in enumerate(headers):
        if h["size"] != (H, W):
            raise A2PError(f"frame {n} is {h['size'][0]} x {h['size'][1]}, frame 0 is {H} x {W}: the frames of one call share one size")
    out = _out_arg(out, N, H, W, dev)
    groups = {}
    for n, h in enumerate(headers):
        groups.setdefault(_header_key(h), []).append(n)
    view, statuses, order = memoryview(buf), [], []
    for idx in groups.values():
        h0 = headers[idx[0]]
        rows, cols, bpm = decode_grid(h0)
        step = max(1, int(max_bytes) // (rows * cols * bpm * 128))
        for a in range(0, len(idx), step):
            part = idx[a:a + step]
            segments = [view[int(off[n]) + headers[n]["segment"][0]:int(off[n]) + headers[n]["segment"][1]] for n in part]
            coef, status = _entropy_stage(segments, h0, dev)
            run = part[-1] - part[0] + 1 == len(part)              # a run of neighbours is decoded in place
            got = pixels(coef, H, W, header_qtabs(h0), h0["sampling"], out[part[0]:part[-1] + 1] if run else None)
            if not run:
                out[torch.as_tensor(part, device=dev)] = got
            statuses.append(status)
            order += part
    status = torch.cat(statuses, 1).cpu().numpy()
    bad = sorted((order[i], word) for i, word in _bad_frames(status))
    if bad and on_error == "raise":
        raise A2PError(f"frame {bad[0][0]} is rejected: {_status_text(bad[0][1])}" + (f" ({len(bad)} frames in all)" if len(bad) > 1 else ""))
    if bad:
        out[torch.as_tensor([n for n, _ in bad], device=dev)] = 0
    return (out, [n for n, _ in bad]) if on_error == "mark" else out


# ------------------------------------------------------------------------------------------------ reading: the container
class MJPEGReader:
    """An AVI file of MJPEGWriter (or one laid out like it: `hdrl` with strh / strf per stream, `movi` with `##dc` and `##wb`
    chunks, below 2 GiB) read back as frames on the GPU.  The `movi` chunks are indexed once through mmap; the file is never
    loaded.  len(), fps, size (height, width), audio (int16 [samples] or [samples, channels], or None), audio_rate; frame_bytes(i)
    is frame i as a JFIF file; read(start, count) returns uint8 GPU frames [count, height, width, 3]; iterating yields the clip
    in slices of slice_frames frames, so a long clip never exists at once."""

    def __init__(self, path, slice_frames: int = 64, device=None):
        import mmap
        self.path, self.slice_frames, self.device = os.fspath(path), max(1, int(slice_frames)), device
        self._f = open(self.path, "rb")
        size = os.fstat(self._f.fileno()).st_size
        if size < 12:
            self._f.close()
            raise ValueError(f"{path} is not a RIFF AVI file")
        self._m = mmap.mmap(self._f.fileno(), 0, access=mmap.ACCESS_READ)
        m = self._m
        if m[:4] != b"RIFF" or m[8:12] != b"AVI ":
            self.close()
            raise ValueError(f"{path} is not a RIFF AVI file")
        self.fps = self.size = self.audio_rate = None
        self._video, self._audio, self._channels, kinds = [], [], None, []

        def walk(a, b, inside):
            while a + 8 <= b:
                fourcc, size = m[a:a + 4], struct.unpack_from("<I", m, a + 4)[0]
                body = a + 8
                if body + size > b:
                    raise ValueError(f"{path}: chunk {fourcc!r} at {a} runs past its list")
                if fourcc == b"LIST":
                    walk(body + 4, body + size, m[body:body + 4])
                elif fourcc == b"strh":
                    kinds.append(m[body:body + 4])
                    if kinds[-1] == b"vids":
                        scale, rate = struct.unpack_from("<II", m, body + 20)
                        self.fps = rate / scale
                elif fourcc == b"strf" and kinds and kinds[-1] == b"vids":
                    w, h = struct.unpack_from("<ii", m, body + 4)
                    self.size = (h, w)
                elif fourcc == b"strf" and kinds and kinds[-1] == b"auds":
                    tag, self._channels, rate, _, _, width = struct.unpack_from("<HHIIHH", m, body)
                    if tag != 1 or width != 16:
                        raise ValueError(f"{path}: the audio is format {tag} with {width} bits; 16-bit PCM is read")
                    self.audio_rate = rate
                elif inside == b"movi" and fourcc[2:] == b"dc":
                    self._video.append((body, size))
                elif inside == b"movi" and fourcc[2:] == b"wb":
                    self._audio.append((body, size))
                a = body + size + (size & 1)

        try:
            walk(12, min(len(m), 8 + struct.unpack_from("<I", m, 4)[0]), b"AVI ")
        except Exception:
            self.close()
            raise

    def __len__(self):
        return len(self._video)

    @property
    def chunks(self):
        """[(offset of the payload in the file, size)] of the video chunks."""
        return list(self._video)

    @property
    def audio(self):
        if self._channels is None:
            return None
        pcm = np.frombuffer(b"".join(self._m[a:a + n] for a, n in self._audio), "<i2").reshape(-1, self._channels)
        return pcm[:, 0].copy() if self._channels == 1 else pcm.copy()

    def frame_bytes(self, i: int) -> bytes:
        a, n = self._video[i]
        return self._m[a:a + n]

    def read(self, start: int = 0, count=None, out=None):
        """uint8 GPU frames [count, height, width, 3]: frames start .. start + count - 1 (count=None: to the end)."""
        start = int(start)
        stop = len(self) if count is None else start + int(count)
        if not (0 <= start <= stop <= len(self)):
            raise A2PError(f"frames [{start}, {stop}) are outside the file's {len(self)}")
        if stop == start:
            if self.size is None:
                raise A2PError(f"{self.path} holds no video stream")
            return torch.empty(0, self.size[0], self.size[1], 3, dtype=torch.uint8, device=_device_of(self.device))
        try:
            return decode_jpeg_frames([self.frame_bytes(i) for i in range(start, stop)], out=out, device=self.device)
        except A2PError as e:
            raise A2PError(f"{self.path}, from frame {start}: {e}") from None

    def __iter__(self):
        for a in range(0, len(self), self.slice_frames):
            yield self.read(a, min(self.slice_frames, len(self) - a))

    def close(self):
        for name in ("_m", "_f"):
            obj = getattr(self, name, None)
            if obj is not None:
                obj.close()
                setattr(self, name, None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False


def read_video_frames(path, start: int = 0, count=None, slice_frames: int = 64, device=None) -> dict:
    """{"frames": uint8 GPU tensor [count, height, width, 3], "fps", "audio", "audio_rate"} of an AVI file of MJPEGWriter: frames
    start .. start + count - 1 (count=None: to the end), decoded slice_frames at a time into one tensor.  A frame's bytes do not
    depend on the slicing."""
    with MJPEGReader(path, slice_frames, device) as r:
        start = int(start)
        stop = len(r) if count is None else start + int(count)
        if not (0 <= start <= stop <= len(r)):
            raise A2PError(f"frames [{start}, {stop}) are outside the file's {len(r)}")
        frames = None
        for a in range(start, stop, r.slice_frames):
            b = min(stop, a + r.slice_frames)
            if frames is None:
                first = r.read(a, b - a)
                if b == stop:
                    frames = first
                    break
                frames = torch.empty(stop - start, *first.shape[1:], dtype=torch.uint8, device=first.device)
                frames[:b - a] = first
            else:
                r.read(a, b - a, out=frames[a - start:b - start])
        if frames is None:
            frames = r.read(start, 0)
        return {"frames": frames, "fps": r.fps, "audio": r.audio, "audio_rate": r.audio_rate}


# ------------------------------------------------------------------------------------------------ rendering into a file
def render_codes_video(face_decoder, face_encoder, body_encoder, decoder, texture, skeleton, rasterizer, poses, face_codes, K, Rt, path,
                       audio=None, audio_rate=None, fps=30, quality: int = 90, subsampling: str = "420", slice_frames: int = 32,
                       supersample: int = 1, background=None, **kw) -> int:
    """encoder.render_codes_motion over slices of slice_frames frames of the time axis, every slice encoded and appended to the AVI
    file `path` before the next is rendered: BodyRenderer.render_full_video.  poses [T, P] (or [1, T, P]) and face_codes with the
    same leading axes: one sequence per file; **kw goes to render_codes_motion (camera_pos, body_embs, max_bytes).  A frame's bytes
    do not depend on the slicing.  supersample and background (anti-aliasing; a display-space colour or panel behind the avatar)
    are render_codes_motion's.  Returns the number of frames."""
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
                                        face_codes[a:a + step], K, Rt, supersample=supersample, background=background, **kw))
    return int(poses.shape[0])


def sequence_path(path: str, index: int, count: int) -> str:
    """`path` itself for a single sequence, else `stem_<index>.ext`."""
    if count == 1:
        return path
    stem, ext = os.path.splitext(path)
    return f"{stem}_{index:02d}{ext}"


def extract_parser():
    """--extract clip.avi --out frames.npy [--frames A:B] [--png-dir DIR] [--wav out.wav]: the frames of an AVI file, decoded on the GPU."""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m audio2photoreal_amd.video --extract",
                                 description="The frames (and the audio) of a Motion-JPEG AVI file, decoded on the MI355X.")
    ap.add_argument("--extract", required=True, metavar="AVI", help="the AVI file, as this module writes it")
    ap.add_argument("--out", required=True, help="frames.npy: uint8 [T, H, W, 3]")
    ap.add_argument("--frames", default=None, metavar="A:B", help="the frames A .. B - 1 (default: all)")
    ap.add_argument("--png-dir", default=None, metavar="DIR", help="also write frame_00_<frame>.png per frame")
    ap.add_argument("--wav", default=None, metavar="FILE", help="also write the audio as a 16-bit PCM wav file")
    ap.add_argument("--slice-frames", type=int, default=64, help="frames on the GPU at a time")
    return ap


def _extract_main(argv) -> int:
    args = extract_parser().parse_args(argv)
    avatar.require_gpu("the frames are decoded")
    with MJPEGReader(args.extract, args.slice_frames) as r:
        window = avatar.frame_window(args.frames)
        a, b = window.start or 0, len(r) if window.stop is None else window.stop
        if not (0 <= a <= b <= len(r)) or r.size is None:
            raise A2PError(f"--frames {args.frames}: {args.extract} holds {len(r)} frames")
        frames = np.lib.format.open_memmap(args.out, mode="w+", dtype=np.uint8, shape=(b - a, r.size[0], r.size[1], 3))
        for s in range(a, b, r.slice_frames):
            frames[s - a:min(b, s + r.slice_frames) - a] = r.read(s, min(b, s + r.slice_frames) - s).cpu().numpy()
        frames.flush()
        print(f"{args.out}: frames {a} .. {b - 1} of {len(r)}, {r.size[0]} x {r.size[1]} at {r.fps:g} fps")
        if args.png_dir is not None:
            from .render import write_pngs
            count = sum(write_pngs({"frame": np.ascontiguousarray(frames[t].transpose(2, 0, 1))[None]}, args.png_dir, first=a + t)
                        for t in range(b - a))                            # one frame at a time; the name carries its index in the file
            print(f"{args.png_dir}: {count} png files")
        if args.wav is not None:
            import wave
            audio = r.audio
            if audio is None:
                raise A2PError(f"{args.extract} holds no audio stream")
            with wave.open(args.wav, "wb") as w:
                w.setnchannels(1 if audio.ndim == 1 else audio.shape[1])
                w.setsampwidth(2)
                w.setframerate(r.audio_rate)
                w.writeframes(audio.astype("<i2").tobytes())
            print(f"{args.wav}: {audio.shape[0]} samples at {r.audio_rate} Hz")
    return 0


def parser():
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
    return ap


def main(argv=None) -> int:
    import sys
    argv = sys.argv[1:] if argv is None else list(argv)
    if any(a == "--extract" or a.startswith("--extract=") for a in argv):
        return _extract_main(argv)
    args = parser().parse_args(argv)
    frames = np.load(args.frames, mmap_mode="r")
    if frames.dtype != np.uint8 or frames.ndim not in (4, 5) or frames.shape[-1] != 3:
        raise A2PError(f"{args.frames} must hold uint8 [T, H, W, 3] or [R, T, H, W, 3] (got {frames.dtype} {list(frames.shape)})")
    avatar.require_gpu("the frames are encoded")
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
