"""Guidance of audio and keyframes separately, without a GPU: the float64 restatement against the pinned oracle, the host
validation (which must refuse before the HIP library is loaded), the new C ABI symbols and the entry points' parameters."""
import inspect
import os
import re

import pytest
import torch

from audio2photoreal_amd import _lib
from audio2photoreal_amd.model_util import create_model_and_diffusion, default_args
from audio2photoreal_amd.spec import face_spec, pose_spec
from audio2photoreal_amd.synthetic import synthetic_inputs, synthetic_state_dict
from conftest import ROOT, rel_max
from oracle import a2p_oracle as O
from tests.dual_guidance_restatement import forward2, guided

SEED, B, T = 10, 2, 60
MODES = tuple(_lib.GUIDANCE_MODES)      # the product's mode names: the restatement below speaks of exactly these


@pytest.fixture(scope="module")
def case():
    spec = pose_spec(num_layers=2)
    den = O.OracleDenoiser(synthetic_state_dict(spec, SEED), "pose", 2, spec.num_heads, dtype=torch.float64)
    inp = synthetic_inputs(spec, B, T, SEED)
    inp["mask"][1, :, :, 30:] = False
    args = (inp["x_T"], torch.tensor([937, 12]), inp["cond_embed"], inp["keyframes"], inp["mask"])
    return den, args


def test_restatement_with_equal_drops_is_the_oracle_forward(case):
    den, (x, t, ce, kf, mask) = case
    for drop in (0.0, 1.0):
        want = den.forward(x, t, ce, kf, mask, drop)
        got = forward2(den, x, t, ce, kf, mask, drop, drop)
        assert float((got - want).abs().max()) <= 1e-12, drop
    # and the two drops do reach different things: the keyframes-only branch is neither of the reference's two
    k = forward2(den, x, t, ce, kf, mask, 1.0, 0.0)
    assert float((k - den.forward(x, t, ce, kf, mask, 0.0)).abs().max()) > 1e-3
    assert float((k - den.forward(x, t, ce, kf, mask, 1.0)).abs().max()) > 1e-3


def test_dual_with_equal_scales_is_joint_guidance(case):
    den, (x, t, ce, kf, mask) = case
    s = torch.tensor([2.0, 3.5])
    want = den.forward_cfg(x, t, ce, s, kf, mask)
    assert sorted(MODES) == ["audio", "dual", "joint"]
    assert rel_max(guided(den, "dual", x, t, ce, kf, mask, s, s), want) <= 1e-12
    assert rel_max(guided(den, "joint", x, t, ce, kf, mask, s), want) <= 1e-12


def test_dual_with_keyframe_scale_one_is_audio_guidance(case):
    den, (x, t, ce, kf, mask) = case
    s = torch.tensor([2.0, 3.5])
    a = guided(den, "audio", x, t, ce, kf, mask, s)
    assert rel_max(guided(den, "dual", x, t, ce, kf, mask, s, torch.ones(B)), a) <= 1e-12
    assert rel_max(a, den.forward_cfg(x, t, ce, s, kf, mask)) > 1e-3      # ... which is not joint guidance


# ----------------------------------------------------------------------------- host validation
@pytest.fixture
def no_library(monkeypatch):
    loaded = []

    def refuse(*a, **k):
        loaded.append(1)
        raise AssertionError("validation reached the HIP library")
    monkeypatch.setattr(_lib, "load", refuse)
    return loaded


def _model(fmt, max_batch=4):
    model, _ = create_model_and_diffusion(default_args(fmt, layers=2), "test", precision="fp32", max_batch=max_batch)
    return model.eval()


def _y(spec, n, **extra):
    inp = synthetic_inputs(spec, n, T, SEED)
    y = {k: inp[k] for k in ("cond_embed", "keyframes", "mask") if k in inp}
    y["scale"] = torch.full((n,), 2.0)
    y.update(extra)
    return inp["x_T"], y


def _calls(model, x, t, y):
    """Every way a guided evaluation is asked for: each must refuse on the host."""
    n = x.shape[0]
    tab, tmap, idx = torch.zeros(11, 5), torch.arange(5), torch.zeros(n, dtype=torch.int64)
    return {
        "forward_cfg": lambda: model.forward_cfg(x, t, y),
        "sample_step": lambda: model.sample_step(0, x, idx, tmap, tab, y, None, 0.0, False),
        "sample_step_inpaint": lambda: model.sample_step_inpaint(0, x, idx, tmap, tab, y, None, 0.0, False, torch.zeros_like(x),
                                                                 torch.zeros_like(x, dtype=torch.uint8)),
        "sample_step_multistep": lambda: model.sample_step_multistep(x, idx, tmap, torch.zeros(4, 5), y, None, False),
        "sample_step_windowed": lambda: model.sample_step_windowed(0, x, idx, tmap, tab, y, None, 0.0, False, [0], torch.ones(1, T), T),
        "sample_step_windowed_multistep": lambda: model.sample_step_windowed_multistep(x, idx, tmap, torch.zeros(4, 5), y, None, False,
                                                                                       [0], torch.ones(1, T), T),
    }


BAD = [
    ("unknown mode", "pose", 2, {"guidance": "keyframes"}, "'keyframes'"),
    ("mode that is no string", "pose", 2, {"guidance": 2}, "2"),
    ("face model, audio", "face", 2, {"guidance": "audio"}, "face"),
    ("face model, dual", "face", 2, {"guidance": "dual", "scale_keyframes": torch.ones(2)}, "face"),
    ("dual without scale_keyframes", "pose", 2, {"guidance": "dual"}, "scale_keyframes"),
    ("scale_keyframes of the wrong shape", "pose", 2, {"guidance": "dual", "scale_keyframes": torch.ones(3)}, "(3,)"),
    ("scale_keyframes of the wrong dtype", "pose", 2, {"guidance": "dual", "scale_keyframes": torch.ones(2, dtype=torch.float64)}, "float64"),
    ("scale_keyframes that is no tensor", "pose", 2, {"guidance": "dual", "scale_keyframes": 1.5}, "float"),
    ("3B over capacity", "pose", 3, {"guidance": "dual", "scale_keyframes": torch.ones(3)}, "max_batch >= 5"),
]


@pytest.mark.parametrize("what,fmt,n,extra,names", BAD, ids=[b[0] for b in BAD])
def test_bad_guidance_is_refused_before_the_library_is_loaded(no_library, what, fmt, n, extra, names):
    spec = face_spec(num_layers=2) if fmt == "face" else pose_spec(num_layers=2)
    model = _model(fmt)
    x, y = _y(spec, n, **extra)
    for name, call in _calls(model, x, torch.zeros(n, dtype=torch.int64), y).items():
        with pytest.raises(_lib.A2PError) as e:
            call()
        assert names in str(e.value), (name, str(e.value))
    assert not no_library and model._ctx is None


def test_forward_drop_arguments(no_library):
    spec = pose_spec(num_layers=2)
    x, y = _y(spec, 2)
    t = torch.zeros(2, dtype=torch.int64)
    assert "keyframe_drop_prob" in inspect.signature(_model("pose").forward).parameters
    with pytest.raises(NotImplementedError, match="keyframe_drop_prob=1"):
        _model("pose").forward(x, t, y, cond_drop_prob=0.0, keyframe_drop_prob=1.0)
    with pytest.raises(NotImplementedError):
        _model("pose").forward(x, t, y, cond_drop_prob=1.0, keyframe_drop_prob=0.5)
    xf, yf = _y(face_spec(num_layers=2), 2)
    with pytest.raises(_lib.A2PError, match="no keyframes"):
        _model("face").forward(xf, t, yf, cond_drop_prob=1.0, keyframe_drop_prob=0.0)
    assert not no_library


def test_entry_point_arguments_are_checked_on_the_host(no_library):
    from audio2photoreal_amd.sample.generate import PoseGuidance, check_pose_capacity, pose_guidance_plan, pose_scale_entries
    assert pose_guidance_plan(2.0) == 2.0 and pose_guidance_plan(2.0, "joint", None) == 2.0
    assert pose_guidance_plan(2.0, "audio") == PoseGuidance(2.0, "audio", None)
    assert pose_guidance_plan(2, "dual", 1.5) == PoseGuidance(2.0, "dual", 1.5)
    for args, names in (((2.0, "keys"), "'keys'"), ((2.0, "dual"), "pose_keyframe_scale"), ((2.0, "audio", 1.5), "1.5"),
                        ((2.0, "dual", float("nan")), "nan"), ((2.0, "dual", "1.5"), "'1.5'")):
        with pytest.raises(_lib.A2PError) as e:
            pose_guidance_plan(*args)
        assert names in str(e.value), str(e.value)
    assert set(pose_scale_entries(2.0, 3, "cpu")) == {"scale"}
    y = pose_scale_entries(PoseGuidance(2.0, "dual", 1.5), 3, "cpu")
    assert y["guidance"] == "dual" and y["scale_keyframes"].dtype == torch.float32 and y["scale_keyframes"].tolist() == [1.5] * 3
    assert y["scale"].tolist() == [2.0] * 3 and "scale_keyframes" not in pose_scale_entries(PoseGuidance(2.0, "audio", None), 3, "cpu")

    class M:
        max_batch = 4
    check_pose_capacity(PoseGuidance(2.0, "dual", 1.5), M, 2)
    check_pose_capacity(PoseGuidance(2.0, "audio", None), M, 4)
    with pytest.raises(_lib.A2PError, match="max_batch >= 5"):
        check_pose_capacity(PoseGuidance(2.0, "dual", 1.5), M, 3)


def test_sharding_carries_the_guidance_keys():
    from audio2photoreal_amd.sample_parallel import shard_model_kwargs
    y = {"scale": torch.arange(4.0), "scale_keyframes": torch.arange(4.0) + 10, "guidance": "dual"}
    out = shard_model_kwargs({"y": y}, 1, 3)["y"]
    assert out["guidance"] == "dual" and out["scale_keyframes"].tolist() == [11.0, 12.0] and out["scale"].tolist() == [1.0, 2.0]


# ----------------------------------------------------------------------------- surface
def test_new_exports_are_declared_everywhere():
    header = open(os.path.join(ROOT, "include", "a2p_hip.h")).read()
    assert re.search(r"\bint a2p_set_guidance\(", header) and "a2p_set_guidance" in _lib.EXPORTS
    for name, value in (("A2P_PASS_KEYS", _lib.PASS_KEYS), ("A2P_PASS_CFG_AUDIO", _lib.PASS_CFG_AUDIO), ("A2P_PASS_CFG_DUAL", _lib.PASS_CFG_DUAL),
                        ("A2P_GUIDE_JOINT", _lib.GUIDE_JOINT), ("A2P_GUIDE_AUDIO", _lib.GUIDE_AUDIO), ("A2P_GUIDE_DUAL", _lib.GUIDE_DUAL),
                        ("A2P_KERNEL_GUIDE_COMBINE", _lib.KERNEL_GUIDE_COMBINE)):
        m = re.search(rf"#define {name} (\d+)", header)
        assert m and int(m.group(1)) == value, name
    declared = set(re.findall(r"\b(a2p_[a-z0-9_]+)\(", header))
    assert declared == set(_lib.EXPORTS), declared ^ set(_lib.EXPORTS)


def test_entry_points_take_the_two_parameters():
    from audio2photoreal_amd.sample import conversation, dataset, inpaint, long_form, recording
    for fn in (recording.generate_from_recording, long_form.generate_from_long_recording, conversation.generate_conversation,
               inpaint.continue_recording, inpaint.regenerate_segment):
        p = inspect.signature(fn).parameters
        assert p["pose_guidance"].default == "joint" and p["pose_keyframe_scale"].default is None, fn.__name__
    cli = dataset.build_parser().parse_args(["--model_path", "m", "--data_root", "d", "--pose_guidance", "dual", "--pose_keyframe_scale", "1.5"])
    assert cli.pose_guidance == "dual" and cli.pose_keyframe_scale == 1.5
    assert dataset.build_parser().parse_args(["--model_path", "m", "--data_root", "d"]).pose_guidance == "joint"
