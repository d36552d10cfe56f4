"""The guided DDPM step tail inside the last decoder layer's tall POST kernel (csrc/kernels_chain4.h, chain4_kernel<3, POST, 3>: paired panels of 24 frames of the
conditional and of the unconditional sequence, guidance combine + transpose + posterior update in the epilogue) against the two launches it replaces (the same kernel
storing the model output rows, then csrc/kernels_misc.h step_tail_kernel; A2P_FUSED_TAIL=0): the SAME BITS, and every other tail still takes step_tail_kernel."""
import ctypes as C

import pytest
import torch

from audio2photoreal_amd import _lib
from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel
from audio2photoreal_amd.model_util import create_model_and_diffusion, default_args, load_model
from audio2photoreal_amd.spec import face_spec
from audio2photoreal_amd.synthetic import synthetic_inputs, synthetic_state_dict
from conftest import record

pytestmark = pytest.mark.gpu
SEED = 10
SWITCHES = ("A2P_CHAIN_V", "A2P_CHAIN_ROWS", "A2P_FUSED_TAIL")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _counter(model):
    if model._ctx is None:
        return 0
    n = C.c_int64(0)
    _lib.check(model._lib().a2p_debug_read(model._ctx, b"fused_tail_launches", C.byref(n), 8), "a2p_debug_read")
    return int(n.value)


def _setup(dev, B, T, precision, scale, monkeypatch):
    spec = face_spec()
    inp = synthetic_inputs(spec, B, T, SEED)
    model, diffusion = create_model_and_diffusion(default_args("face"), "test", precision=precision, max_batch=B)
    load_model(model, synthetic_state_dict(spec, SEED))
    model = model.to(dev).eval()
    y = {"cond_embed": inp["cond_embed"].to(dev), "scale": torch.tensor(scale, dtype=torch.float32, device=dev)}
    gen = torch.Generator().manual_seed(SEED + 1)
    noise = torch.randn(inp["x_T"].shape, generator=gen).to(dev)
    monkeypatch.setenv("A2P_CHAIN_V", "4")
    if 2 * B * T < 1100:
        monkeypatch.setenv("A2P_CHAIN_ROWS", "1")        # below the chain threshold the small-forward kernels would run
    return model, diffusion, inp["x_T"].to(dev), y, noise


def _both(model, monkeypatch, step):
    """step() with the fused tail and with A2P_FUSED_TAIL=0: ({name: outputs}, {name: fused launches})."""
    outs, fused = {}, {}
    for name, flag in (("fused", None), ("launches", "0")):
        if flag is None:
            monkeypatch.delenv("A2P_FUSED_TAIL", raising=False)
        else:
            monkeypatch.setenv("A2P_FUSED_TAIL", flag)
        before = _counter(model)
        out = step()
        outs[name] = {k: v.cpu() for k, v in out.items()}
        fused[name] = _counter(model) - before
    return outs, fused


def _finish(model, monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    model.check_finite()
    model.release()


def _assert_same_bits(outs, what):
    for k in ("sample", "pred_xstart"):
        a, b = outs["fused"][k], outs["launches"][k]
        assert torch.isfinite(a).all(), (what, k)
        diff = float((a - b).abs().max())
        record(f"fused_step_tail_vs_launches/{what}/{k}", max_abs_diff=diff)
        assert torch.equal(a, b), (what, k, diff)


@pytest.mark.parametrize("T", [240, 248])
def test_fused_ddpm_tail_is_bit_identical(dev, T, monkeypatch):
    """One p_sample with given noise, B = 2, fp16, at t = 999, a middle timestep and t = 0 (the noise mask is zero there), with and without the clamp.  T = 240 is ten whole
    half-panels of 24 frames; T = 248 leaves a last half-panel of 8 frames, masked in the epilogue."""
    B = 2
    model, diffusion, x, y, noise = _setup(dev, B, T, "fp16", [10.0] * B, monkeypatch)
    cfg = ClassifierFreeSampleModel(model)
    for ts, clip in ((999, False), (417, True), (0, False)):
        t = torch.full((B,), ts, device=dev)
        outs, fused = _both(model, monkeypatch, lambda: diffusion.p_sample(cfg, x, t, clip_denoised=clip, model_kwargs={"y": y}, noise=noise))
        assert fused == {"fused": 1, "launches": 0}, (ts, fused)
        _assert_same_bits(outs, f"B{B}_T{T}_t{ts}")
        if ts == 0:                                            # no noise enters the last step
            assert torch.equal(outs["fused"]["sample"], outs["fused"]["pred_xstart"])
    _finish(model, monkeypatch)


@pytest.mark.parametrize("B,scale", [(2, [10.0, 2.5]), (3, [10.0, 2.5, 0.0])])
def test_fused_ddpm_tail_per_sample_scale_and_timestep(dev, B, scale, monkeypatch):
    """A guidance scale and a timestep of its own for every sample (the epilogue reads both per sequence pair), at an even and at an odd batch."""
    T = 240
    model, diffusion, x, y, noise = _setup(dev, B, T, "fp16", scale, monkeypatch)
    cfg = ClassifierFreeSampleModel(model)
    t = torch.tensor([901, 0, 417][:B], device=dev)
    outs, fused = _both(model, monkeypatch, lambda: diffusion.p_sample(cfg, x, t, clip_denoised=False, model_kwargs={"y": y}, noise=noise))
    _finish(model, monkeypatch)
    assert fused == {"fused": 1, "launches": 0}, fused
    _assert_same_bits(outs, f"B{B}_T{T}_scales")
    a = outs["fused"]["sample"]
    assert not torch.equal(a[0], a[1])


def test_fused_ddpm_tail_bf16(dev, monkeypatch):
    """The bf16 library's instance of the kernel."""
    B, T = 2, 240
    model, diffusion, x, y, noise = _setup(dev, B, T, "bf16", [10.0, 2.5], monkeypatch)
    cfg = ClassifierFreeSampleModel(model)
    t = torch.tensor([650, 33], device=dev)
    outs, fused = _both(model, monkeypatch, lambda: diffusion.p_sample(cfg, x, t, clip_denoised=False, model_kwargs={"y": y}, noise=noise))
    _finish(model, monkeypatch)
    assert fused == {"fused": 1, "launches": 0}, fused
    _assert_same_bits(outs, f"B{B}_T{T}_bf16")


def test_other_tails_keep_the_step_tail_kernel(dev, monkeypatch):
    """A DDIM step and a forward without guidance never take the fused tail, and the switch changes none of their bits."""
    B, T = 2, 240
    model, diffusion, x, y, noise = _setup(dev, B, T, "fp16", [10.0, 2.5], monkeypatch)
    cfg = ClassifierFreeSampleModel(model)
    t = torch.tensor([650, 33], device=dev)
    outs, fused = _both(model, monkeypatch, lambda: diffusion.ddim_sample(cfg, x, t, clip_denoised=False, model_kwargs={"y": y}, eta=0.0))
    assert fused == {"fused": 0, "launches": 0}, fused
    _assert_same_bits(outs, f"B{B}_T{T}_ddim")
    monkeypatch.setenv("A2P_CHAIN_ROWS", "1")
    plain, fused = _both(model, monkeypatch, lambda: {"out": model(x, t, y)})
    _finish(model, monkeypatch)
    assert fused == {"fused": 0, "launches": 0}, fused
    assert torch.isfinite(plain["fused"]["out"]).all() and torch.equal(plain["fused"]["out"], plain["launches"]["out"])
