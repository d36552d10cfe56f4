"""Guidance of audio and keyframes separately on the GPU (`pytest -m gpu`): y["guidance"] = "audio" / "dual" through the C ABI
against the float64 restatement (tests/dual_guidance_restatement.py), the untouched default, batch independence, every sampler
step variant, and the capacity rule.  Full body model (pose_spec(): 6 layers), synthetic weights, max_batch = 4.

Gates: the guided forwards use s = 2, s_k = 1.5, whose coefficient magnitudes |1 - s_k| + |s_k - s| + |s| = 3 equal those of joint
guidance at scale 2 (|1 - s| + |s| = 3), so they are held to the gates tests/test_hip_parity.py::test_forward_vs_reference_golden
holds the guided pose forward to (fp32 2e-4, fp16 9.5e-4, bf16 1.8e-2), the single keyframes-only branch to its cond / uncond gates;
sampling to the project's 1e-3 bar in fp32.  Every measured error goes through conftest.record."""
import pytest
import torch

from audio2photoreal_amd import _lib
from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel
from audio2photoreal_amd.model_util import create_gaussian_diffusion, create_model_and_diffusion, default_args, load_model
from audio2photoreal_amd.sample.inpaint import inpaint_sample_loop
from audio2photoreal_amd.sample.long_form import plan_windows, windowed_sample_loop
from audio2photoreal_amd.spec import pose_spec
from audio2photoreal_amd.synthetic import cond_tokens_for_frames, synthetic_inputs, synthetic_state_dict
from conftest import record, rel_l2, rel_max
from oracle import a2p_oracle as O
from tests.dual_guidance_restatement import branches, model_fn

pytestmark = pytest.mark.gpu
SEED, T = 10, 240
S, S_K = 2.0, 1.5
GATE_GUIDED = {"fp32": 2e-4, "fp16": 9.5e-4, "bf16": 1.8e-2}
GATE_BRANCH = {"fp32": 2e-4, "fp16": 9.5e-4, "bf16": 1.1e-2}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


_MODELS, _REF = {}, {}


def get_model(precision, dev, max_batch=4):
    key = (precision, max_batch)
    if key not in _MODELS:
        spec = pose_spec()
        model, _ = create_model_and_diffusion(default_args("pose", timestep_respacing="ddim5"), "test", precision=precision,
                                              max_batch=max_batch)
        load_model(model, synthetic_state_dict(spec, SEED))
        _MODELS[key] = model.to(dev).eval()
    return _MODELS[key]


def oracle():
    if "den" not in _REF:
        spec = pose_spec()
        _REF["den"] = O.OracleDenoiser(synthetic_state_dict(spec, SEED), "pose", spec.num_layers, spec.num_heads, dtype=torch.float64)
    return _REF["den"]


def inputs(B, frames=T):
    """Synthetic inputs of B samples; B = 2 at 240 frames masks the second sample's keyframes from frame 90 on."""
    inp = synthetic_inputs(pose_spec(), B, frames, SEED)
    if B == 2 and frames == T:
        inp["mask"][1, :, :, 90:] = False
    inp["t"] = torch.tensor([937, 12, 401][:B])
    return inp


def reference_branches(B, frames=T):
    """e(K,A), e(K,0), e(0,0) of `inputs(B, frames)` in float64: computed once, shared, never written to.  The B = 1 case is the
    first sample of the B = 2 batch (the same synthetic streams, the same timestep, a full mask): no operation mixes samples."""
    key = (B, frames)
    if key not in _REF:
        if key == (1, T):
            _REF[key] = {n: v[:1] for n, v in reference_branches(2).items()}
        else:
            inp = inputs(B, frames)
            _REF[key] = branches(oracle(), inp["x_T"], inp["t"], inp["cond_embed"], inp["keyframes"], inp["mask"])
    return _REF[key]


def combine(e, mode, s, s_k=None):
    if mode == "joint":
        return e["0"] + s * (e["ka"] - e["0"])
    if mode == "audio":
        return e["k"] + s * (e["ka"] - e["k"])
    return e["0"] + s_k * (e["k"] - e["0"]) + s * (e["ka"] - e["k"])


def y_for(inp, dev, mode=None, s=S, s_k=None, rows=None):
    sl = slice(None) if rows is None else slice(*rows)
    B = inp["x_T"][sl].shape[0]
    y = {k: inp[k][sl].clone().to(dev) for k in ("cond_embed", "keyframes", "mask")}
    y["scale"] = torch.full((B,), s, device=dev)
    if mode is not None:
        y["guidance"] = mode
    if s_k is not None:
        y["scale_keyframes"] = torch.full((B,), s_k, device=dev)
    return y


# ----------------------------------------------------------------------------- 1. forward vs the float64 restatement
@pytest.mark.parametrize("precision", ["fp32", "fp16", "bf16"])
@pytest.mark.parametrize("B", [1, 2], ids=["B1_per_op", "B2_chain"])
def test_forward_vs_restatement(dev, B, precision):
    """B = 1: 3B T = 720 rows, below the body model's 960-row chain threshold (per-op kernels); B = 2: 1440 rows, chain kernels."""
    model = get_model(precision, dev)
    cfg = ClassifierFreeSampleModel(model)
    inp = inputs(2)
    rows = (0, B)
    x, t = inp["x_T"][:B].to(dev), inp["t"][:B].to(dev)
    e = reference_branches(B)
    errs = {}
    for mode, s_k in (("audio", None), ("dual", S_K)):
        y = y_for(inp, dev, mode, S, s_k, rows)
        got = cfg(x, t, y).cpu()
        errs[mode] = rel_l2(got, combine(e, mode, S, s_k))
        if B == 2:   # the reference zeroes masked keyframes in y, in place (model/diffusion.py:320)
            assert float(y["keyframes"][1, 3:].abs().max()) == 0.0
    y = y_for(inp, dev, None, S, None, rows)
    errs["keys_only"] = rel_l2(model(x, t, y, cond_drop_prob=1.0, keyframe_drop_prob=0.0).cpu(), e["k"])
    if precision == "fp32":
        y = y_for(inp, dev, "dual", 2.5, 0.0, rows)
        errs["dual_sk0_s2.5"] = rel_l2(cfg(x, t, y).cpu(), combine(e, "dual", 2.5, 0.0))
    model.check_finite()
    record(f"dual_guidance/fwd240/B{B}/{precision}", **errs)
    print(errs)
    assert errs["audio"] < GATE_GUIDED[precision] and errs["dual"] < GATE_GUIDED[precision], errs
    assert errs["keys_only"] < GATE_BRANCH[precision], errs
    assert errs.get("dual_sk0_s2.5", 0.0) < GATE_GUIDED["fp32"], errs


# ----------------------------------------------------------------------------- 2. the default is untouched
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_joint_is_the_default_bit_for_bit(dev, precision):
    model = get_model(precision, dev)
    cfg = ClassifierFreeSampleModel(model)
    inp = inputs(2)
    x, t = inp["x_T"].to(dev), inp["t"].to(dev)
    diff = create_gaussian_diffusion(default_args("pose", timestep_respacing="ddim5"))
    plain = cfg(x, t, y_for(inp, dev)).cpu()
    dual = cfg(x, t, y_for(inp, dev, "dual", S, S_K)).cpu()            # a separately guided call in between leaves nothing behind
    named = cfg(x, t, y_for(inp, dev, "joint")).cpu()
    assert torch.equal(plain, named) and not torch.equal(plain, dual)
    loop = lambda y: diff.ddim_sample_loop(cfg, tuple(x.shape), clip_denoised=False, model_kwargs={"y": y}, noise=x).cpu()
    a, b = loop(y_for(inp, dev)), loop(y_for(inp, dev, "joint"))
    assert torch.isfinite(a).all() and torch.equal(a, b)


# ----------------------------------------------------------------------------- 3. batch independence
@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_dual_forward_does_not_depend_on_the_batch(dev, precision):
    """A sample's bits depend neither on B nor on its index, under a2p_set_batch_hint's contract (tests/test_shard_invariance_hip.py):
    a "dual" forward at B = 2 equals two B = 1 forwards that name the unsharded batch."""
    model = get_model(precision, dev)
    cfg = ClassifierFreeSampleModel(model)
    inp = inputs(2)
    x, t = inp["x_T"].to(dev), inp["t"].to(dev)

    def call(lo, hi, hint):
        model.global_batch_hint = hint
        return cfg(x[lo:hi].contiguous(), t[lo:hi].contiguous(), y_for(inp, dev, "dual", S, S_K, (lo, hi))).cpu()
    try:
        whole = call(0, 2, 0)
        parts = torch.cat([call(0, 1, 2), call(1, 2, 2)])
    finally:
        model.global_batch_hint = 0
    diff = float((parts - whole).abs().max())
    record(f"dual_guidance/batch_independence/{precision}", max_abs_diff=diff)
    assert torch.isfinite(whole).all() and torch.equal(parts, whole), diff


# ----------------------------------------------------------------------------- 4. sampling vs the oracle sampler
def test_ddim5_dual_vs_oracle_sampler(dev):
    model = get_model("fp32", dev)
    inp = inputs(2)
    fn = model_fn(oracle(), "dual", inp["cond_embed"], inp["keyframes"], inp["mask"], S, S_K)
    _, want = O.OracleSampler("ddim5").ddim_sample_loop(fn, inp["x_T"].double())
    diff = create_gaussian_diffusion(default_args("pose", timestep_respacing="ddim5"))
    got = diff.ddim_sample_loop(ClassifierFreeSampleModel(model), tuple(inp["x_T"].shape), clip_denoised=False,
                                model_kwargs={"y": y_for(inp, dev, "dual", S, S_K)}, noise=inp["x_T"].to(dev)).cpu()
    e2, em = rel_l2(got, want), rel_max(got, want)
    record("dual_guidance/ddim5/fp32", rel_l2=e2, rel_max=em)
    assert e2 < 1e-3 and em < 1e-3, (e2, em)


# ----------------------------------------------------------------------------- 5. every other step variant carries three branches
def _variants(dev):
    inp = inputs(2)
    x = inp["x_T"].to(dev)
    shape = tuple(x.shape)
    g = torch.Generator().manual_seed(3)
    step_noise = torch.randn((5,) + shape, generator=g).to(dev)
    known = torch.randn(shape, generator=g).to(dev)
    held = torch.zeros(2, T, dtype=torch.bool, device=dev)
    held[:, 40:101] = True
    plan = plan_windows(900)                     # two windows of 600 frames, 300 shared
    assert plan.W == 2 and plan.T_w == 600
    wg = torch.Generator().manual_seed(4)
    yw = {"cond_embed": torch.randn(2, cond_tokens_for_frames(600), 1024, generator=wg).to(dev),
          "keyframes": torch.randn(2, 20, 104, generator=wg).to(dev), "mask": torch.ones(2, 1, 1, 600, dtype=torch.bool, device=dev)}
    noise_w = torch.randn(1, 104, 1, 900, generator=wg).to(dev)
    y_clip = lambda extra: {**y_for(inp, dev), **extra}
    y_win = lambda extra: {**{k: v.clone() for k, v in yw.items()}, "scale": torch.full((2,), S, device=dev), **extra}
    return {
        "p_sample_loop": lambda d, m, extra: d.p_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": y_clip(extra)}, noise=x,
                                                             step_noise=lambda n: step_noise[n]),
        "dpm++2m": lambda d, m, extra: d.dpm_solver_sample_loop(m, shape, clip_denoised=False, model_kwargs={"y": y_clip(extra)}, noise=x),
        "inpaint": lambda d, m, extra: inpaint_sample_loop(d, m, y_clip(extra), known, held, x),
        "windowed": lambda d, m, extra: windowed_sample_loop(d, m, plan, 1, y_win(extra), noise_w),
    }


@pytest.mark.parametrize("variant", ["p_sample_loop", "dpm++2m", "inpaint", "windowed"])
def test_step_variants_carry_three_branches(dev, variant):
    """"dual" with s_k = s is joint guidance at s (tests/test_dual_guidance_cpu.py) computed from three branches and two fused
    multiply-adds instead of two and one: fp32 rounding apart (~1e-6).  A wrong branch order or stride shows as O(1)."""
    model = get_model("fp32", dev)
    cfg = ClassifierFreeSampleModel(model)
    diff = create_gaussian_diffusion(default_args("pose", timestep_respacing="ddim5"))
    run = _variants(dev)[variant]
    joint = run(diff, cfg, {}).cpu()
    dual = run(diff, cfg, {"guidance": "dual", "scale_keyframes": torch.full((2,), S, device=dev)}).cpu()
    e2, em = rel_l2(dual, joint), rel_max(dual, joint)
    record(f"dual_guidance/variants/{variant}/fp32", rel_l2=e2, rel_max=em)
    assert torch.isfinite(joint).all() and e2 < 1e-3 and em < 1e-3, (e2, em)


# ----------------------------------------------------------------------------- 6. capacity
def test_three_branches_need_capacity(dev):
    frames = 90
    inp = inputs(3, frames)
    x, t = inp["x_T"].to(dev), inp["t"].to(dev)
    small = ClassifierFreeSampleModel(get_model("fp32", dev))
    with pytest.raises(_lib.A2PError, match="max_batch >= 5"):
        small(x, t, y_for(inp, dev, "dual", S, S_K))
    model = get_model("fp32", dev, max_batch=5)
    got = ClassifierFreeSampleModel(model)(x, t, y_for(inp, dev, "dual", S, S_K)).cpu()      # 3B = 9 sequences: an odd count
    err = rel_l2(got, combine(reference_branches(3, frames), "dual", S, S_K))
    model.check_finite()
    model.release()
    _MODELS.pop(("fp32", 5))
    record("dual_guidance/capacity/B3_T90/fp32", rel_l2=err)
    assert err < GATE_GUIDED["fp32"], err
