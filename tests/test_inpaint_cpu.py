"""Sampling with held elements on the host (sample/inpaint.py): every refusal happens before any GPU work, and the window of a
segment re-roll."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from audio2photoreal_amd import _lib
from audio2photoreal_amd.sample.inpaint import inpaint_sample_loop, segment_window
from audio2photoreal_amd.sample.recording import continue_recording, regenerate_segment

STATS = {"audio_mean": np.array([0.01, -0.02]), "audio_std_flat": np.array([0.3]),
         "code_mean": np.zeros(256), "code_std": np.ones(256), "pose_mean": np.zeros(104), "pose_std": np.ones(104)}
B, C, T = 2, 8, 60


class _Model:
    """Enough of a ClassifierFreeSampleModel for the argument checks; any call into it is GPU work and fails the test."""
    def a2p_sample_step_inpaint(self, *args, **kwargs):
        raise AssertionError("reached the GPU step")


def _loop(**kw):
    args = {"diffusion": None, "model": _Model(), "y": {}, "known": torch.zeros(B, C, 1, T), "known_mask": torch.zeros(B, T, dtype=torch.bool),
            "noise": None}
    args.update(kw)
    return inpaint_sample_loop(**args)


@pytest.mark.parametrize("sampler", ["plms", "ddim_reverse", ""])
def test_loop_refuses_samplers(sampler):
    with pytest.raises(_lib.A2PError, match="PLMS"):
        _loop(sampler=sampler)


def test_loop_refuses_a_model_without_the_step():
    with pytest.raises(_lib.A2PError, match="a2p_sample_step_inpaint"):
        _loop(model=object())


@pytest.mark.parametrize("mask", [torch.zeros(B, T), torch.zeros(B, T, dtype=torch.uint8), torch.zeros(B, T, dtype=torch.int64),
                                  np.zeros((B, T), bool)])
def test_loop_refuses_mask_dtypes(mask):
    with pytest.raises(_lib.A2PError, match="bool"):
        _loop(known_mask=mask)


@pytest.mark.parametrize("shape", [(B, T + 1), (B + 1, T), (B, 1, T), (B, C, T), (B, 2, 1, T), (B, C, 1, T - 1), (1, C, 1, T), (B * C * T,)])
def test_loop_refuses_mask_shapes(shape):
    with pytest.raises(_lib.A2PError, match="known_mask must be"):
        _loop(known_mask=torch.zeros(shape, dtype=torch.bool))


@pytest.mark.parametrize("known,match", [(torch.zeros(B, C, T), r"\[B, C, 1, T\]"), (torch.zeros(B, C, 2, T), r"\[B, C, 1, T\]"),
                                         (np.zeros((B, C, 1, T), np.float32), r"\[B, C, 1, T\]"),
                                         (torch.zeros(B, C, 1, T, dtype=torch.float64), "float32"),
                                         (torch.zeros(B, C, 1, T, dtype=torch.float16), "float32")])
def test_loop_refuses_known(known, match):
    with pytest.raises(_lib.A2PError, match=match):
        _loop(known=known)


def test_loop_refuses_noise_shape():
    with pytest.raises(_lib.A2PError, match="noise must be"):
        _loop(noise=torch.zeros(B, C, 1, T + 30))


def test_loop_refuses_host_tensors():
    """Every mask form is accepted by the checks; the host tensor is then refused (the hot path has no CPU implementation)."""
    for mask in (torch.ones(B, T, dtype=torch.bool), torch.ones(B, 1, 1, T, dtype=torch.bool), torch.ones(B, C, 1, T, dtype=torch.bool)):
        with pytest.raises(_lib.A2PError, match="MI355X"):
            _loop(known_mask=mask, noise=torch.zeros(B, C, 1, T))


# ------------------------------------------------------------------------------------------------------------ recording level

def _pair(nfeats, seq_len=600, guide=False):
    m = SimpleNamespace(audio_frontend=object(), seq_len=seq_len, nfeats=nfeats)
    if guide:
        m.transformer, m.tokenizer = object(), object()
    return (SimpleNamespace(model=m), None)


FACE, POSE = _pair(256), _pair(104, guide=True)


def _result(R=2, T=240):
    return {"face": np.zeros((R, T, 256)), "pose": np.zeros((R, T, 104)), "keyframes": np.zeros((R, T // 30, 104)),
            "audio": np.zeros((2, T * 1600)), "T": T, "sr": 48000}


WAV4 = np.ones(48000 * 4 + 10, np.float32)      # 120 frames


def _cont(previous=None, wav=WAV4, sr=48000, face=FACE, pose=POSE, **kw):
    return continue_recording(face, pose, STATS, wav, sr, _result() if previous is None else previous, **kw)


@pytest.mark.parametrize("P", [0, -30, 100, 45, 29, 120.5])
def test_continue_refuses_context_off_the_grid(P):
    with pytest.raises(_lib.A2PError, match="multiple of 30"):
        _cont(context_frames=P)


def test_continue_refuses_context_longer_than_the_clip():
    with pytest.raises(_lib.A2PError, match="previous clip has 120 frames"):
        _cont(previous=_result(T=120), context_frames=150)


def test_continue_refuses_a_window_over_seq_len():
    with pytest.raises(_lib.A2PError, match="seq_len"):
        _cont(wav=np.ones(48000 * 16, np.float32), context_frames=150)            # 480 + 150 > 600
    with pytest.raises(_lib.A2PError, match="seq_len"):
        _cont(face=_pair(256, seq_len=200), context_frames=120)                    # 120 + 120 > 200


def test_continue_refuses_repetition_mismatch():
    with pytest.raises(_lib.A2PError, match="repetitions"):
        _cont(num_repetitions=3)


@pytest.mark.parametrize("key,value", [("face", np.nan), ("pose", np.inf), ("audio", -np.inf)])
def test_continue_refuses_non_finite_previous(key, value):
    prev = _result()
    prev[key][0, 7] = value
    with pytest.raises(_lib.A2PError, match="non-finite"):
        _cont(previous=prev)


def test_continue_refuses_malformed_previous():
    with pytest.raises(_lib.A2PError, match="result dict"):
        _cont(previous={"face": np.zeros((2, 240, 256))})
    bad = _result()
    bad["audio"] = np.zeros((2, 1000))
    with pytest.raises(_lib.A2PError, match="audio samples"):
        _cont(previous=bad)


def test_continue_refuses_short_chunks_and_models_without_guide():
    with pytest.raises(_lib.A2PError, match="4 s"):
        _cont(wav=np.ones(48000 * 3, np.float32))
    with pytest.raises(_lib.A2PError, match="guide transformer"):
        _cont(pose=_pair(104))


def test_continue_passes_the_host_checks():
    """A valid call stops where the GPU work starts: the fake models have no device."""
    with pytest.raises(AttributeError, match="null_cond_embed"):
        _cont(context_frames=120, num_repetitions=2)


@pytest.mark.parametrize("s,e", [(0, 0), (60, 30), (10, 60), (0, 61), (-30, 60), (0, 270), (210, 270), (30.5, 60)])
def test_regenerate_refuses_bounds(s, e):
    with pytest.raises(_lib.A2PError, match="segment"):
        regenerate_segment(FACE, POSE, STATS, _result(), s, e)


@pytest.mark.parametrize("parts", [(), ("body",), ("face", "hands"), "lips"])
def test_regenerate_refuses_parts(parts):
    with pytest.raises(_lib.A2PError, match="parts"):
        regenerate_segment(FACE, POSE, STATS, _result(), 0, 60, parts=parts)


def test_regenerate_refuses_non_finite_result():
    res = _result()
    res["pose"][1, 3, 2] = np.nan
    with pytest.raises(_lib.A2PError, match="non-finite"):
        regenerate_segment(FACE, POSE, STATS, res, 0, 60)


def test_regenerate_refuses_a_segment_longer_than_the_window():
    with pytest.raises(_lib.A2PError, match="does not fit"):
        regenerate_segment(FACE, POSE, STATS, _result(T=1200), 0, 630)


def test_segment_window():
    assert segment_window(240, 90, 180, 600) == (0, 240)
    assert segment_window(600, 0, 600, 600) == (0, 600)
    for T_, s, e in ((1200, 0, 60), (1200, 570, 630), (1200, 1140, 1200), (1800, 900, 1500), (1230, 600, 630), (1200, 0, 600)):
        ws, we = segment_window(T_, s, e, 600)
        assert we - ws == 600 and ws % 30 == 0 and 0 <= ws <= s and e <= we <= T_, (T_, s, e, ws, we)
    assert segment_window(1200, 570, 630, 600) == (300, 900)                         # centred where the clip allows
    with pytest.raises(_lib.A2PError, match="does not fit"):
        segment_window(1200, 0, 630, 600)
