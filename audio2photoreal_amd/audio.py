"""Waveform input: `resample` (torchaudio.functional.resample on the MI355X) and `read_wav`.

torchaudio is not part of this stack, and the demo (demo/demo.py:156-167) brings a recording at any rate to 48 kHz with
`torchaudio.functional.resample(y, orig_freq=sr, new_freq=48_000)`.  `resample` keeps that function's semantics (torchaudio 2.0.2,
pinned by demo/requirements.txt; restated from `_get_sinc_resample_kernel` / `_apply_sinc_resample_kernel`, see
`sinc_resample_table`): the filter bank is built on the host, the convolution is csrc/kernels_audio.h (`a2p_resample`).
"""
from __future__ import annotations

import math
import wave
from typing import Optional, Tuple

import numpy as np
import torch

from . import _lib

KAISER_BETA = 14.769656459379492          # torchaudio's default beta of sinc_interp_kaiser
_METHOD_ALIASES = {"sinc_interpolation": "sinc_interp_hann", "kaiser_window": "sinc_interp_kaiser"}   # torchaudio's deprecated names
_TABLES = {}


def _int_rate(v, name: str) -> int:
    if v <= 0:
        raise ValueError(f"{name} must be positive (got {v})")
    if int(v) != v or int(v) >= 2 ** 31:
        raise ValueError(f"{name} must be an integer frequency below 2**31 (got {v})")
    return int(v)


def reduced_rates(orig_freq: int, new_freq: int) -> Tuple[int, int]:
    """(orig, new) divided by their gcd: the resampler's input stride and phase count."""
    g = math.gcd(orig_freq, new_freq)
    return orig_freq // g, new_freq // g


def sinc_filter_width(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99) -> int:
    o, n = reduced_rates(orig_freq, new_freq)
    return math.ceil(lowpass_filter_width * o / (min(o, n) * rolloff))


def resampled_length(length: int, orig_freq: int, new_freq: int) -> int:
    """Samples `resample` returns for `length` input samples: ceil(n * length / o) (the input itself at equal rates)."""
    if orig_freq == new_freq:
        return length
    o, n = reduced_rates(orig_freq, new_freq)
    return -(-n * length // o)


def sinc_resample_table(orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
                        resampling_method: str = "sinc_interp_hann", beta: Optional[float] = None,
                        dtype: torch.dtype = torch.float32) -> Tuple[torch.Tensor, int]:
    """`_get_sinc_resample_kernel` on the host: (table [n, 2 * width + o] in `dtype`, width).

    `dtype` is the dtype the table is computed in; the device kernel reads it cast to float32.  torchaudio's functional form
    computes it in the waveform's dtype (float32 for the demo's call); `transforms.Resample` computes it in float64 and casts.
    Both rules are restated from the torchaudio source without a copy of it to check against: the float64 rule here is float64
    throughout, beta included (INTEGRATION.md "From a recording": unpinned).
    Tables over A2P_RESAMPLE_MAX_TABLE_BYTES (16 MB; co-prime rates such as 44056 -> 48000 Hz) raise A2PError."""
    orig_freq, new_freq = _int_rate(orig_freq, "orig_freq"), _int_rate(new_freq, "new_freq")
    method = _METHOD_ALIASES.get(resampling_method, resampling_method)
    if method not in ("sinc_interp_hann", "sinc_interp_kaiser"):
        raise ValueError(f"Invalid resampling method: {resampling_method}")
    if lowpass_filter_width <= 0:
        raise ValueError("Low pass filter width should be positive.")
    if dtype not in (torch.float32, torch.float64):
        raise ValueError(f"the table is built in float32 or float64 (got {dtype})")
    o, n = reduced_rates(orig_freq, new_freq)
    width = sinc_filter_width(orig_freq, new_freq, lowpass_filter_width, rolloff)
    nbytes = n * (2 * width + o) * 4
    if nbytes > _lib.RESAMPLE_MAX_TABLE_BYTES:
        raise _lib.A2PError(f"resampling {orig_freq} -> {new_freq} Hz needs a filter table of {nbytes / 2 ** 20:.1f} MB "
                            f"([{n}, {2 * width + o}]; the limit is {_lib.RESAMPLE_MAX_TABLE_BYTES >> 20} MB): resample to a rate "
                            "with a larger common divisor with the target first")
    base = min(o, n) * rolloff
    lpw = lowpass_filter_width
    idx = torch.arange(-width, width + o, dtype=dtype)[None] / o
    t = torch.arange(0, -n, -1, dtype=dtype)[:, None] / n + idx
    t *= base
    t = t.clamp_(-lpw, lpw)
    if method == "sinc_interp_hann":
        window = torch.cos(t * math.pi / lpw / 2) ** 2
    else:
        beta_t = torch.tensor(float(KAISER_BETA if beta is None else beta), dtype=dtype)
        window = torch.i0(beta_t * torch.sqrt(1 - (t / lpw) ** 2)) / torch.i0(beta_t)
    t *= math.pi
    kernels = torch.where(t == 0, torch.tensor(1.0).to(t), t.sin() / t)
    kernels *= window * (base / o)
    return kernels.contiguous(), width


def _device_table(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta, dtype, device):
    key = (reduced_rates(orig_freq, new_freq), lowpass_filter_width, float(rolloff), resampling_method, beta, dtype, str(device))
    hit = _TABLES.get(key)
    if hit is None:
        table, width = sinc_resample_table(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta, dtype)
        if len(_TABLES) >= 32:
            _TABLES.clear()
        hit = _TABLES[key] = (table.to(device=device, dtype=torch.float32), width)
    return hit


def _resample_rows(x: torch.Tensor, length: int, channels: int, orig_freq: int, new_freq: int, lowpass_filter_width=6, rolloff=0.99,
                   resampling_method="sinc_interp_hann", beta=None, kernel_dtype=None) -> torch.Tensor:
    """x fp32 on the GPU, contiguous [rows, length, channels] -> [rows, resampled_length(length)] (channels averaged first)."""
    rows = x.numel() // max(1, length * channels)
    out_len = resampled_length(length, orig_freq, new_freq)
    out = torch.empty(rows, out_len, device=x.device, dtype=torch.float32)
    if out.numel() == 0:
        return out
    table, width = None, 0
    n_phase = n_taps = 0
    if orig_freq != new_freq:
        table, width = _device_table(orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta,
                                     kernel_dtype or torch.float32, x.device)
        n_phase, n_taps = table.shape
    with _lib.on_device_of(x):
        _lib.check(_lib.load().a2p_resample(_lib.ptr(x), rows, length, channels, orig_freq, new_freq, _lib.ptr(table), n_phase, n_taps,
                                            width, _lib.ptr(out), _lib.current_stream(x.device)), "a2p_resample")
    return out


def resample(waveform: torch.Tensor, orig_freq: int, new_freq: int, lowpass_filter_width: int = 6, rolloff: float = 0.99,
             resampling_method: str = "sinc_interp_hann", beta: Optional[float] = None,
             kernel_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """torchaudio.functional.resample for a float32 waveform [..., L] on the GPU -> [..., ceil(n L / o)].

    Equal rates return `waveform` itself.  `kernel_dtype`: the dtype the filter table is computed in before its float32 cast;
    None = the functional form's rule (the waveform's dtype, float32), torch.float64 = the rule of torchaudio.transforms.Resample.
    The convolution sums in float32 on the device, in a different order than conv1d: results agree with torchaudio to float32
    rounding, not bit for bit."""
    orig_freq, new_freq = _int_rate(orig_freq, "orig_freq"), _int_rate(new_freq, "new_freq")
    if orig_freq == new_freq:
        return waveform
    _lib.require_gpu_tensor(waveform, "waveform")
    if waveform.dtype != torch.float32:
        raise TypeError(f"resample takes a float32 waveform (got {waveform.dtype})")
    shape = waveform.shape
    L = shape[-1]
    x = waveform.reshape(-1, L).contiguous()
    out = _resample_rows(x, L, 1, orig_freq, new_freq, lowpass_filter_width, rolloff, resampling_method, beta, kernel_dtype)
    return out.reshape(*shape[:-1], out.shape[-1])


def read_wav(path: str) -> Tuple[np.ndarray, int]:
    """(samples, sample_rate) of a PCM WAV file, read with the standard library's `wave`.  samples: float32 [L] (mono) or [L, C],
    holding the stored integer values as the demo's `torch.Tensor(int array)` does (8-bit PCM is unsigned, 0..255, as stored;
    16/24/32-bit are signed)."""
    try:
        with wave.open(path, "rb") as w:
            C, width, sr, L = w.getnchannels(), w.getsampwidth(), w.getframerate(), w.getnframes()
            raw = w.readframes(L)
    except wave.Error as e:
        raise ValueError(f"{path}: not a PCM WAV file that the `wave` module reads ({e}); convert it to 8/16/24/32-bit PCM") from None
    if width == 1:
        v = np.frombuffer(raw, np.uint8)
    elif width == 2:
        v = np.frombuffer(raw, "<i2")
    elif width == 3:
        b = np.frombuffer(raw, np.uint8).reshape(-1, 3).astype(np.int32)
        v = b[:, 0] | (b[:, 1] << 8) | (b[:, 2] << 16)
        v = np.where(v >= 1 << 23, v - (1 << 24), v)
    elif width == 4:
        v = np.frombuffer(raw, "<i4")
    else:
        raise ValueError(f"{path}: {8 * width}-bit samples are not supported (8/16/24/32-bit PCM)")
    v = v.astype(np.float32).reshape(-1, C)
    return (v[:, 0].copy() if C == 1 else v), sr
