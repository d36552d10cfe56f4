"""Recording -> y["audio"] on the host: the resampler's filter table against an independent restatement of torchaudio's
`_get_sinc_resample_kernel`, output lengths, `read_wav`, and the argument checks that must refuse before any GPU work."""
import math
import os
import wave

import numpy as np
import pytest
import torch

import torchaudio_restatement as TA
from audio2photoreal_amd import _lib
from audio2photoreal_amd.audio import read_wav, resample, resampled_length, sinc_resample_table
from audio2photoreal_amd.sample.recording import prepare_recording

RATES = [(44100, 48000), (22050, 48000), (16000, 48000), (11025, 48000), (8000, 48000), (96000, 48000), (48000, 16000)]
STATS = {"audio_mean": np.array([0.01, -0.02]), "audio_std_flat": np.array([0.3])}


@pytest.mark.parametrize("kaiser", [False, True], ids=["hann", "kaiser"])
@pytest.mark.parametrize("orig,new", RATES)
def test_table_float64_matches_restatement(orig, new, kaiser):
    method = "sinc_interp_kaiser" if kaiser else "sinc_interp_hann"
    got, width = sinc_resample_table(orig, new, resampling_method=method, dtype=torch.float64)
    want, w_want, o, n = TA.sinc_table(orig, new, kaiser=kaiser)
    assert width == w_want == math.ceil(6 * o / (min(o, n) * 0.99))
    assert got.dtype == torch.float64 and tuple(got.shape) == (n, 2 * width + o)
    assert np.abs(got.numpy() - want).max() <= 1e-12


@pytest.mark.parametrize("kaiser", [False, True], ids=["hann", "kaiser"])
@pytest.mark.parametrize("orig,new", RATES)
def test_table_float32_is_the_float32_computation(orig, new, kaiser):
    """The functional form's rule: the table is computed in float32.  It agrees with the same steps in numpy float32 to a few
    float32 ulps of the peak tap (sin / cos / i0 implementations differ in the last bits; the restatement takes i0 in float64), and with the float64 table only to what
    float32 evaluation of t = (-p/n + k/o) * base allows (the sum cancels before the multiplication: ~1e-5 of the peak)."""
    method = "sinc_interp_kaiser" if kaiser else "sinc_interp_hann"
    got, width = sinc_resample_table(orig, new, resampling_method=method, dtype=torch.float32)
    assert got.dtype == torch.float32
    same, _, _, _ = TA.sinc_table(orig, new, kaiser=kaiser, dtype=np.float32)
    exact, _, _, _ = TA.sinc_table(orig, new, kaiser=kaiser)
    peak = np.abs(exact).max()
    assert np.abs(got.numpy() - same).max() <= 16 * np.finfo(np.float32).eps * peak
    assert np.abs(got.numpy().astype(np.float64) - exact).max() <= 3e-5 * peak


@pytest.mark.parametrize("orig,new", RATES)
@pytest.mark.parametrize("L", [1, 5, 13, 100, 4097])
def test_output_length(orig, new, L):
    """ceil(n L / o), the length the restated conv1d + truncation gives, also for inputs shorter than the filter's width."""
    table, width, o, n = TA.sinc_table(orig, new)
    y = TA.apply_table(np.ones(L), table, width, o, n)
    assert resampled_length(L, orig, new) == y.shape[-1] == math.ceil(n * L / o)
    assert resampled_length(L, 48000, 48000) == L


def _write_wav(path, data, width, sr):
    data = np.asarray(data)
    C = 1 if data.ndim == 1 else data.shape[1]
    if width == 1:
        raw = data.astype(np.uint8).tobytes()
    elif width == 2:
        raw = data.astype("<i2").tobytes()
    elif width == 3:
        v = data.astype(np.int64).reshape(-1) & 0xFFFFFF
        raw = np.stack([v & 0xFF, (v >> 8) & 0xFF, v >> 16], axis=1).astype(np.uint8).tobytes()
    else:
        raw = data.astype("<i4").tobytes()
    with wave.open(path, "wb") as w:
        w.setnchannels(C)
        w.setsampwidth(width)
        w.setframerate(sr)
        w.writeframes(raw)


@pytest.mark.parametrize("channels", [1, 2])
@pytest.mark.parametrize("width", [1, 2, 3, 4])
def test_read_wav_round_trip(tmp_path, width, channels):
    rng = np.random.default_rng(width * 10 + channels)
    lo, hi = {1: (0, 256), 2: (-2 ** 15, 2 ** 15), 3: (-2 ** 23, 2 ** 23), 4: (-2 ** 31, 2 ** 31)}[width]
    shape = (1000,) if channels == 1 else (1000, channels)
    data = rng.integers(lo, hi, size=shape, dtype=np.int64)
    data.reshape(-1)[:2] = [lo, hi - 1]                      # the extremes of the format
    path = os.path.join(tmp_path, f"x{width}_{channels}.wav")
    sr = [8000, 44100, 22050, 96000][width - 1]
    _write_wav(path, data, width, sr)
    got, got_sr = read_wav(path)
    assert got_sr == sr and got.dtype == np.float32 and got.shape == shape
    np.testing.assert_array_equal(got, data.astype(np.float32))   # the integer values, as torch.Tensor(int array) holds them


def test_read_wav_refuses_non_pcm(tmp_path):
    path = os.path.join(tmp_path, "float.wav")
    # a WAVE_FORMAT_IEEE_FLOAT header (format tag 3): Python's wave module reads PCM only
    body = np.zeros(8, np.float32).tobytes()
    fmt = (b"fmt " + (16).to_bytes(4, "little") + (3).to_bytes(2, "little") + (1).to_bytes(2, "little") + (48000).to_bytes(4, "little")
           + (192000).to_bytes(4, "little") + (4).to_bytes(2, "little") + (32).to_bytes(2, "little"))
    data = b"data" + len(body).to_bytes(4, "little") + body
    with open(path, "wb") as f:
        f.write(b"RIFF" + (4 + len(fmt) + len(data)).to_bytes(4, "little") + b"WAVE" + fmt + data)
    with pytest.raises(ValueError, match="PCM"):
        read_wav(path)


# ---------------------------------------------------------------------------------------------- refused on the host
# device="cuda" on purpose: every one of these must be refused before anything is moved to (or launched on) a GPU

def test_too_short_recording():
    with pytest.raises(_lib.A2PError, match="at least 4 s"):
        prepare_recording(np.ones(int(44100 * 3.9), np.int16), 44100, STATS, 1, device="cuda")


def test_too_long_recording():
    # 25 s keeps 24 s = 720 frames > the models' 600; 21 s keeps 20 s and would pass this check
    with pytest.raises(_lib.A2PError, match="at most 600 frames"):
        prepare_recording(np.ones((2, 44100 * 25), np.int16), 44100, STATS, 1, device="cuda")


def test_bad_repetitions():
    with pytest.raises(_lib.A2PError, match="num_repetitions"):
        prepare_recording(np.ones(48000 * 5, np.float32), 48000, STATS, 0, device="cuda")


@pytest.mark.parametrize("orig,new", [(0, 48000), (-44100, 48000), (44100, 0)])
def test_bad_rates(orig, new):
    with pytest.raises(ValueError):
        resample(torch.ones(100), orig, new)
    with pytest.raises(ValueError):
        sinc_resample_table(orig, new)
    if new == 48000:
        with pytest.raises(ValueError):
            prepare_recording(np.ones(48000 * 5, np.float32), orig, STATS, 1, device="cuda")


def test_oversized_table():
    # 44056 and 48000 share only the factor 8: a [6000, 11025] table (252 MB)
    with pytest.raises(_lib.A2PError, match="MB"):
        sinc_resample_table(44056, 48000)
    with pytest.raises(_lib.A2PError, match="MB"):
        prepare_recording(np.ones(44056 * 5, np.float32), 44056, STATS, 1, device="cuda")


def test_cpu_tensor_is_refused():
    with pytest.raises(_lib.A2PError, match="MI355X"):
        resample(torch.ones(1000), 44100, 48000)
    x = torch.ones(10)
    assert resample(x, 48000, 48000) is x          # equal rates: the input itself, as torchaudio does
    with pytest.raises(_lib.A2PError, match="MI355X"):
        prepare_recording(np.ones(48000 * 5, np.float32), 48000, STATS, 1, device="cpu")


def test_abi_rejects_null_arguments():
    lib = _lib.load()
    err_arg = -1        # include/a2p_hip.h A2P_ERR_ARG
    assert lib.a2p_resample(None, 1, 100, 1, 44100, 48000, None, 160, 161, 7, None, None) == err_arg
    assert b"null" in lib.a2p_last_error()
    assert lib.a2p_dual_audio(None, 100, None, None, 0.0, 0.0, 1.0, 1, None, None) == err_arg
    assert b"null" in lib.a2p_last_error()
