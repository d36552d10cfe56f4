"""Independent numpy restatements the recording tests compare against (no torchaudio on this stack):

- `sinc_table`: torchaudio 2.0.2 `_get_sinc_resample_kernel` (the table in float64, or in float32 step by step the way the
  functional form computes it in the waveform's dtype);
- `apply_table`: `_apply_sinc_resample_kernel` in float64 (pad (width, width + o), stride-o correlation, phases interleaved,
  truncation to ceil(n L / o));
- `dual_audio`: demo/demo.py:178-186 from the resampled mono signal (float64 numpy, then torch.Tensor(...).float()).
"""
import math

import numpy as np

BETA = 14.769656459379492


def sinc_table(orig, new, lpw=6, rolloff=0.99, kaiser=False, beta=BETA, dtype=np.float64):
    g = math.gcd(orig, new)
    o, n = orig // g, new // g
    base = min(o, n) * rolloff
    width = math.ceil(lpw * o / base)
    f = np.dtype(dtype).type
    idx = np.arange(-width, width + o).astype(dtype) / f(o)
    t = np.arange(0, -n, -1).astype(dtype)[:, None] / f(n) + idx[None]
    t = np.clip(t * f(base), f(-lpw), f(lpw))
    if kaiser:
        w = (np.i0(np.float64(beta) * np.sqrt(1 - (t.astype(np.float64) / lpw) ** 2)) / np.i0(np.float64(beta))).astype(dtype)
    else:
        w = np.cos(t * f(math.pi) / f(lpw) / f(2)) ** 2
    tt = t * f(math.pi)
    safe = np.where(tt == 0, f(1), tt)
    k = np.where(tt == 0, f(1), np.sin(tt) / safe)
    return (k * (w * f(base / o))).astype(dtype), width, o, n


def apply_table(x, table, width, o, n):
    """x [..., L] -> [..., ceil(n L / o)], float64."""
    x = np.asarray(x, np.float64)
    shape, L = x.shape[:-1], x.shape[-1]
    rows = x.reshape(-1, L)
    taps = table.shape[1]
    K = np.asarray(table, np.float64)
    want = -(-n * L // o)
    out = []
    for r in rows:
        xp = np.pad(r, (width, width + o))
        win = np.lib.stride_tricks.sliding_window_view(xp, taps)[::o]       # [nq, taps]
        out.append((win @ K.T).reshape(-1)[:want])
    return np.stack(out).reshape(*shape, want)


def resample(x, orig, new, kaiser=False, dtype=np.float64):
    if orig == new:
        return np.asarray(x, np.float64)
    table, width, o, n = sinc_table(orig, new, kaiser=kaiser, dtype=dtype)
    return apply_table(x, table.astype(np.float32), width, o, n)


def dual_audio(mono, noise, audio_mean, audio_std_flat, reps):
    """mono float32 [Lc] (resampled, cut), noise float64 [1, Lc, 2] -> (float32 [reps, Lc, 2], float64 normalised [1, Lc, 2])."""
    mono = np.asarray(mono, np.float32)
    dual = noise.copy()
    dual[:, :, 0] = mono / mono.max()                     # float32 division, widened
    dual = (dual - audio_mean) / audio_std_flat
    return np.tile(dual.astype(np.float32), (reps, 1, 1)), dual
