"""Long recordings on the host: the window plan of windowed joint sampling (sample/long_form.py plan_windows) and the argument
checks that must refuse before any GPU work."""
import numpy as np
import pytest

from audio2photoreal_amd import _lib
from audio2photoreal_amd.sample.long_form import check_batch, plan_windows, prepare_long_recording, recording_frames

STATS = {"audio_mean": np.array([0.01, -0.02]), "audio_std_flat": np.array([0.3])}


def _coverage(plan):
    cover = np.zeros(plan.T_total, np.int64)
    total = np.zeros(plan.T_total, np.float64)
    for w, s in enumerate(plan.starts):
        cover[s:s + plan.T_w] += 1
        total[s:s + plan.T_w] += plan.weights[w].astype(np.float64)
    return cover, total


@pytest.mark.parametrize("T_total", [600, 720, 1110, 1200, 1800, 3600])
def test_plan_geometry_and_weights(T_total):
    plan = plan_windows(T_total)
    assert plan.T_total == T_total and plan.T_w == 600 and plan.W == len(plan.starts)
    assert plan.W == (1 if T_total <= 600 else -(-(T_total - 600) // 480) + 1)
    assert plan.weights.dtype == np.float32 and plan.weights.shape == (plan.W, 600)
    assert plan.starts[0] == 0 and plan.starts[-1] == T_total - 600
    assert all(s % 30 == 0 for s in plan.starts)
    assert all(b > a and a + 600 - b >= 120 for a, b in zip(plan.starts, plan.starts[1:]))
    cover, total = _coverage(plan)
    assert cover.min() >= 1
    assert np.abs(total - 1.0).max() <= 2e-7
    assert (plan.weights > 0).all()


def test_plan_single_window():
    for T in (120, 360, 600):
        plan = plan_windows(T)
        assert plan.W == 1 and plan.starts == [0] and plan.T_w == T
        assert np.array_equal(plan.weights, np.ones((1, T), np.float32))


def test_plan_feather():
    """Linear feather: distance + 0.5 to the nearer edge; the recording's own ends count as infinitely far."""
    plan = plan_windows(720)
    assert plan.starts == [0, 120]
    w0, w1 = plan.weights.astype(np.float64)
    assert np.all(w0[:120] == 1.0) and np.all(w1[480:] == 1.0)            # frames only one window covers
    i = np.arange(120, 600)
    raw0, raw1 = (599 - i) + 0.5, (i - 120) + 0.5
    assert np.allclose(w0[120:], raw0 / (raw0 + raw1), rtol=0, atol=1e-7)
    assert np.allclose(w1[:480], raw1 / (raw0 + raw1), rtol=0, atol=1e-7)


def test_plan_three_windows_cover_a_frame():
    plan = plan_windows(1110)
    cover, total = _coverage(plan)
    assert plan.W == 3 and cover.max() == 3
    triple = np.nonzero(cover == 3)[0]
    assert triple.size > 0 and np.abs(total[triple] - 1.0).max() <= 2e-7
    for w, s in enumerate(plan.starts):                                      # every covering window takes part in the blend
        assert (plan.weights[w][triple - s] > 0).all()


@pytest.mark.parametrize("kw,match", [({"min_overlap": 29}, "min_overlap"), ({"min_overlap": 301}, "min_overlap"),
                                      ({"min_overlap": 0}, "min_overlap")])
def test_plan_refuses_bad_overlap(kw, match):
    with pytest.raises(_lib.A2PError, match=match):
        plan_windows(1800, **kw)


def test_plan_refuses_unaligned_length():
    with pytest.raises(_lib.A2PError, match="multiple"):
        plan_windows(1805)


def test_check_batch():
    plan = plan_windows(1800)
    check_batch(plan, 2, 8)
    with pytest.raises(_lib.A2PError, match="max_batch"):
        check_batch(plan, 3, 8)


def test_long_recording_passes_the_host_checks():
    """The 25 s recording prepare_recording refuses (test_recording_cpu.py::test_too_long_recording): 720 frames, two windows.
    On device="cpu" the host checks pass and the call stops where the GPU work would start."""
    wav = np.ones((2, 44100 * 25), np.int16)
    assert recording_frames(wav, 44100) == 720
    with pytest.raises(_lib.A2PError, match="MI355X"):
        prepare_long_recording(wav, 44100, STATS, 1, device="cpu", max_batch=2)


def test_long_recording_refusals_before_device_work():
    wav = np.ones(48000 * 61, np.float32)                  # 60 s kept: 1800 frames, 4 windows
    with pytest.raises(_lib.A2PError, match="min_overlap"):
        prepare_long_recording(wav, 48000, STATS, 1, device="cuda", min_overlap=400)
    with pytest.raises(_lib.A2PError, match="max_batch"):
        prepare_long_recording(wav, 48000, STATS, 3, device="cuda", max_batch=8)
    with pytest.raises(_lib.A2PError, match="num_repetitions"):
        prepare_long_recording(wav, 48000, STATS, 0, device="cuda")
    with pytest.raises(_lib.A2PError, match="4 s"):
        prepare_long_recording(np.ones(48000 * 3, np.float32), 48000, STATS, 1, device="cuda")
