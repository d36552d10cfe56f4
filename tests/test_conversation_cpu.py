"""Conversations without a GPU (sample/conversation.py): the restatement's routing properties, validation before any device
work, the per-person seed rule and the new C ABI symbols."""
import numpy as np
import pytest
import torch

from audio2photoreal_amd import _lib
from audio2photoreal_amd.sample import conversation as conv
from audio2photoreal_amd.sample_parallel import derive_seed
from tests.conversation_restatement import conversation_audio, person_audio

SR = 16000


def _stats(mean=(0.003, -0.001), std=0.21):
    rng = np.random.default_rng(0)
    return {"audio_mean": np.array(mean), "audio_std_flat": np.array([std]),
            "code_mean": rng.standard_normal(256), "code_std": 0.5 + rng.random(256),
            "pose_mean": rng.standard_normal(104), "pose_std": 0.5 + rng.random(104)}


def _chans(n=4000, seed=1):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.8, 0.9, (2, n)).astype(np.float32)


def test_person_one_is_person_zero_swapped_under_equal_stats():
    c, st = _chans(), _stats(mean=(0.01, 0.01))
    for normalize in ("peak", "none"):
        a, b = conversation_audio(c, (st, st), 2, normalize)
        assert a.shape == (2, c.shape[1], 2) and np.array_equal(a[..., ::-1], b)
        _, d0 = person_audio(c, 0, st, normalize)
        _, d1 = person_audio(c, 1, st, normalize)
        assert np.array_equal(d0[::-1], d1)


def test_peak_and_none_agree_at_unit_peak():
    c = _chans()
    c[:, 17] = 1.0
    st = _stats()
    for p in range(2):
        zp, dp = person_audio(c, p, st, "peak")
        zn, dn = person_audio(c, p, st, "none")
        assert np.array_equal(zp, zn) and np.array_equal(dp, dn)


def test_partner_channel_is_the_other_voice():
    c, st = _chans(), _stats(mean=(0.0, 0.0), std=1.0)
    z, _ = person_audio(c, 1, st, "none")
    assert np.array_equal(z[:, 0], c[1].astype(np.float64)) and np.array_equal(z[:, 1], c[0].astype(np.float64))
    assert conversation_audio(c, (None, st), 1, "none", people=(False, True))[0] is None


class _NoDevice:
    """Stands for a model: any attribute access means the validation reached the models or the device."""
    def __getattr__(self, name):
        raise AssertionError(f"validation touched the model ({name}) before refusing")


@pytest.fixture
def no_device(monkeypatch):
    def refuse(*a, **k):
        raise AssertionError("validation reached the device")
    to = torch.Tensor.to

    def host_only_to(self, *a, **k):
        if any(isinstance(v, (str, torch.device)) and torch.device(v).type != "cpu" for v in list(a) + list(k.values())):
            refuse()
        return to(self, *a, **k)
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(torch.Tensor, "to", host_only_to)
    monkeypatch.setattr(torch.Tensor, "cuda", refuse)


def _wav(seconds=5.0, sr=SR, channels=2):
    n = int(seconds * sr)
    return np.random.default_rng(0).uniform(-1000, 1000, (n, channels)).astype(np.float32)


def test_prepare_refuses_before_device_work(no_device):
    st = (_stats(), _stats())
    with pytest.raises(ValueError):
        conv.prepare_conversation(_wav()[:, 0], SR, st, 1)                  # mono
    with pytest.raises(ValueError):
        conv.prepare_conversation(_wav(channels=3), SR, st, 1)              # 3 channels
    with pytest.raises(ValueError):
        conv.prepare_conversation((_wav()[:, 0], _wav()[:-5, 1]), SR, st, 1)   # tracks of different lengths
    with pytest.raises(_lib.A2PError):
        conv.prepare_conversation(_wav(3.5), SR, st, 1)                     # under 4 s
    with pytest.raises(_lib.A2PError):
        conv.prepare_conversation(_wav(), SR, st, 1, normalize="rms")
    with pytest.raises(_lib.A2PError):
        conv.prepare_conversation(_wav(), SR, st, 1, people=(False, False))
    with pytest.raises(_lib.A2PError):
        conv.prepare_conversation(_wav(), SR, st, 0)
    with pytest.raises(_lib.A2PError):
        conv.prepare_conversation(_wav(), SR, st, 1, device="cpu")
    with pytest.raises(_lib.A2PError):
        conv.prepare_conversation(_wav(45), SR, st, 3, max_batch=8)         # 2 people x 3 x 3 windows


def test_generate_refuses_before_device_work(no_device, monkeypatch):
    m = _NoDevice()
    st = _stats()
    person = ((m, m), (m, m), st)
    for kw in ({"sampler": "plms"}, {"normalize": "rms"}):
        with pytest.raises(_lib.A2PError, match="sampler|normalize"):
            conv.generate_conversation((person, person), _wav(), SR, **kw)
    with pytest.raises(_lib.A2PError):
        conv.generate_conversation((None, None), _wav(), SR)
    with pytest.raises(_lib.A2PError):
        conv.generate_conversation((person, person), _wav(), SR, num_repetitions=0)


class _Den:
    """Just enough of a denoiser for the validation of generate_conversation."""
    def __init__(self, frontend=True, guide=True, max_batch=8):
        self.audio_frontend = object() if frontend else None
        self.transformer = _Cap(max_batch) if guide else None
        self.tokenizer = object() if guide else None
        self.max_batch = max_batch
        self.seq_len = 600
        self.null_cond_embed = torch.zeros(1)


class _Cap:
    def __init__(self, max_batch):
        self.max_batch = max_batch


def test_generate_validates_models_and_input(no_device):
    st = _stats()
    good = ((_Den(), None), (_Den(), None), st)
    for bad in (((_Den(frontend=False), None), (_Den(), None), st), ((_Den(), None), (_Den(guide=False), None), st),
                ((_Den(), None), (_Den(frontend=False), None), st)):
        with pytest.raises(_lib.A2PError, match="front end|guide transformer"):
            conv.generate_conversation((good, bad), _wav(), SR)
    with pytest.raises(ValueError):
        conv.generate_conversation((good, None), _wav()[:, 0], SR)
    with pytest.raises(ValueError):
        conv.generate_conversation((good, None), _wav(channels=3), SR)
    with pytest.raises(ValueError):
        conv.generate_conversation((None, good), (_wav()[:, 0], _wav()[:-1, 1]), SR)
    with pytest.raises(_lib.A2PError, match="at least 4 s"):
        conv.generate_conversation((good, good), _wav(3.9), SR)
    small = ((_Den(max_batch=2), None), (_Den(max_batch=2), None), st)
    with pytest.raises(_lib.A2PError, match="max_batch"):
        conv.generate_conversation((small, None), _wav(), SR, num_repetitions=3)          # 3 > 2 before any GPU work
    with pytest.raises(_lib.A2PError, match="max_batch"):
        conv.generate_conversation((small, None), _wav(30), SR, num_repetitions=2)        # 2 x 2 windows > 2
    with pytest.raises(_lib.A2PError, match="MI355X"):
        conv.generate_conversation((small, None), _wav(30), SR, num_repetitions=1)        # 1 x 2 windows fit: only the device is missing
    f, p = (_Den(max_batch=4), None), (_Den(max_batch=4), None)
    with pytest.raises(_lib.A2PError, match="max_batch"):
        conv.generate_conversation(((f, p, st), (f, p, st)), _wav(), SR, num_repetitions=3)   # one batch of 2 x 3 > 4


def test_seed_rule():
    s0, s1 = conv.person_seeds(10)
    assert s0 != s1 and (s0, s1) == (derive_seed(10, 11, 0), derive_seed(10, 11, 1))
    assert conv.person_seeds(11) != (s0, s1)
    assert all(derive_seed(10, t, r) not in (s0, s1) for t in range(1, 11) for r in range(4))
    assert conv.person_seeds((5, 7)) == (5, 7)
    with pytest.raises(_lib.A2PError):
        conv.person_seeds((1, 2, 3))


def test_exports():
    for name in ("a2p_resample_channels", "a2p_conversation_audio"):
        assert name in _lib.EXPORTS
    from audio2photoreal_amd.sample import recording
    assert recording.generate_conversation is conv.generate_conversation
    assert recording.prepare_conversation is conv.prepare_conversation
