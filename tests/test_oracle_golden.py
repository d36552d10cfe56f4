"""Pin the oracle (oracle/a2p_oracle.py) against the golden vectors the REFERENCE
produced in the build container (tests/golden/make_golden.py).  CPU only."""
import numpy as np
import pytest
import torch

from audio2photoreal_amd.spec import face_spec, pose_spec
from audio2photoreal_amd.synthetic import synthetic_inputs, synthetic_state_dict, synthetic_tensor
from conftest import rel_l2, rel_max
from oracle import a2p_oracle as O

SEED = 10
TOL = 2e-5   # fp32 restatement vs fp32 reference: different op order only


def _spec(fmt):
    return face_spec() if fmt == "face" else pose_spec()


def _den(fmt, dtype=torch.float32):
    spec = _spec(fmt)
    return spec, O.OracleDenoiser(synthetic_state_dict(spec, SEED), fmt, spec.num_layers, spec.num_heads, dtype)


@pytest.mark.parametrize("name,resp", [("full", ""), ("ddim10", "ddim10"), ("ddim100", "ddim100"), ("ddim500", "ddim500")])
def test_schedule_tables_bit_exact(golden, name, resp):
    tab = O.make_schedule(resp)
    for k in ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_recip_alphas_cumprod",
              "sqrt_recipm1_alphas_cumprod", "posterior_variance", "posterior_log_variance_clipped",
              "posterior_mean_coef1", "posterior_mean_coef2", "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod"):
        assert np.array_equal(tab[k], golden[f"sched/{name}/{k}"]), k      # float64, bit exact
    assert list(golden[f"sched/{name}/timestep_map"]) == tab["timestep_map"]


def test_space_timesteps(golden):
    assert sorted(O.space_timesteps(1000, "ddim50")) == list(golden["sched/space/ddim50"])
    assert sorted(O.space_timesteps(300, "10,15,20")) == list(golden["sched/space/10,15,20"])
    with pytest.raises(ValueError):
        O.space_timesteps(1000, "ddim999")


@pytest.mark.parametrize("fmt", ["face", "pose"])
def test_decoder_layer(golden, fmt):
    spec, den = _den(fmt)
    d = spec.latent_dim
    lx = synthetic_tensor(SEED, "layer_x", (2, 48, d))
    lmem = synthetic_tensor(SEED, "layer_mem", (2, 80, d))
    lt = synthetic_tensor(SEED, "layer_t", (2, d))
    lmem2 = synthetic_tensor(SEED, "layer_mem2", (2, 8, d)) if spec.is_pose else None
    got = O.decoder_layer(den.sd, "seqTransDecoder.stack.0.", lx, lmem, lt, spec.num_heads, den.freqs, lmem2)
    assert rel_l2(got, golden[f"{fmt}/layer0"]) < TOL


@pytest.mark.parametrize("fmt", ["face", "pose"])
def test_forward_cond_uncond_cfg(golden, fmt):
    spec, den = _den(fmt)
    inp = synthetic_inputs(spec, 2, 240, SEED)
    if spec.is_pose:
        inp["mask"][1, :, :, 90:] = False
    times = torch.tensor([937, 12])
    kf, mk = inp.get("keyframes"), inp.get("mask")
    c = den.forward(inp["x_T"], times, inp["cond_embed"], kf, mk, 0.0)
    u = den.forward(inp["x_T"], times, inp["cond_embed"], kf, mk, 1.0)
    assert rel_l2(c, golden[f"{fmt}/fwd_cond"]) < TOL
    assert rel_l2(u, golden[f"{fmt}/fwd_uncond"]) < TOL
    scale = torch.full((2,), 10.0 if fmt == "face" else 2.0)
    g = den.forward_cfg(inp["x_T"], times, inp["cond_embed"], scale, kf, mk)
    assert rel_l2(g, golden[f"{fmt}/fwd_cfg"]) < 5 * TOL


@pytest.mark.parametrize("fmt", ["face", "pose"])
def test_ddpm10_and_first_steps(golden, fmt):
    spec, den = _den(fmt)
    scale = torch.full((1,), 10.0 if fmt == "face" else 2.0)
    inp = synthetic_inputs(spec, 1, 240, SEED, steps_of_noise=10)
    fn = lambda x, ts: den.forward_cfg(x, ts, inp["cond_embed"], scale, inp.get("keyframes"), inp.get("mask"))
    s = O.OracleSampler("ddim10")
    sample, _ = s.p_sample_loop(fn, inp["x_T"], [inp["step_noise"][i] for i in range(10)])
    assert rel_l2(sample, golden[f"{fmt}/ddpm10"]) < 1e-4
    assert rel_max(sample, golden[f"{fmt}/ddpm10"]) < 1e-4
    inp = synthetic_inputs(spec, 1, 240, SEED, steps_of_noise=3)
    s = O.OracleSampler("")
    sample, _ = s.p_sample_loop(fn, inp["x_T"], [inp["step_noise"][i] for i in range(3)], max_steps=3)
    assert rel_l2(sample, golden[f"{fmt}/ddpm1000_first3"]) < 1e-4


def test_ddim10_face_config0(golden):
    """BASELINE.json configs[0]: face, ddim10, B=1, T=240."""
    spec, den = _den("face")
    inp = synthetic_inputs(spec, 1, 240, SEED)
    scale = torch.full((1,), 10.0)
    fn = lambda x, ts: den.forward_cfg(x, ts, inp["cond_embed"], scale)
    x0, _ = O.OracleSampler("ddim10").ddim_sample_loop(fn, inp["x_T"])
    assert rel_l2(x0, golden["face/ddim10"]) < 1e-4
    assert rel_max(x0, golden["face/ddim10"]) < 1e-4


@pytest.mark.parametrize("fmt,order", [("face", 2), ("face", 4), ("pose", 3)])
def test_plms_loop_vs_reference(golden_plms, fmt, order):
    """the oracle's PLMS restatement against the reference's plms_sample_loop output."""
    spec, den = _den(fmt)
    B, frames = (1, 240) if fmt == "face" else (2, 240)
    inp = synthetic_inputs(spec, B, frames, SEED)
    scale = torch.full((B,), 10.0 if fmt == "face" else 2.0)
    fn = lambda x, ts: den.forward_cfg(x, ts, inp["cond_embed"], scale, inp.get("keyframes"), inp.get("mask"))  # noqa: E731
    sample, _ = O.OracleSampler("ddim10").plms_sample_loop(fn, inp["x_T"], order=order)
    assert rel_l2(sample, golden_plms[f"{fmt}/plms10_order{order}"]) < 5 * TOL


def test_plms_first_steps_and_ddim_reverse_vs_reference(golden_plms):
    spec, den = _den("face")
    inp = synthetic_inputs(spec, 1, 240, SEED)
    scale = torch.full((1,), 10.0)
    fn = lambda x, ts: den.forward_cfg(x, ts, inp["cond_embed"], scale)  # noqa: E731
    s = O.OracleSampler("ddim10")
    o0 = s.plms_sample(fn, inp["x_T"], torch.tensor([9]), 2, None)
    o1 = s.plms_sample(fn, o0["sample"], torch.tensor([8]), 2, o0["old_eps"])
    for i, o in enumerate((o0, o1)):
        for k in ("sample", "pred_xstart"):
            assert rel_l2(o[k], golden_plms[f"face/plms_step{i}/{k}"]) < 5 * TOL, (i, k)
    r = s.ddim_reverse_sample(fn, inp["x_T"], torch.tensor([5]))
    assert rel_l2(r["sample"], golden_plms["face/ddim_reverse_t5"]) < 5 * TOL



def test_chain_fixture_is_what_the_committed_generator_produces(tmp_path):
    """tests/golden/golden_chain_body_v1.npz (the oracle's ddim100 chain of the body workload, gated against by the GPU suite) must be reproducible from
    tests/tools/chain_vs_oracle.py --side oracle: the first 10 steps re-run here (3 s) land on the stored state after step 10; the face fixture (21
    CPU-minutes) is checked for its layout only."""
    import os
    import sys
    import numpy as np
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
    import chain_vs_oracle as CVO

    class A:
        workload, T, threads, steps, out = "body", 600, 4, 10, str(tmp_path / "chain_body_first10.npz")
    CVO.side_oracle(A)
    got, want = np.load(A.out), np.load(CVO.golden_path("body"))
    assert sorted(k for k in want.files if k.startswith("step")) == ["step10", "step100", "step50", "step90"]
    err = np.linalg.norm(got["step10"].astype(np.float64) - want["step10"]) / np.linalg.norm(want["step10"])
    assert err < 1e-6, err
    face = np.load(CVO.golden_path("face"))
    assert sorted(k for k in face.files if k.startswith("step")) == ["step100", "step1000", "step500", "step900"]
    assert face["step1000"].shape == (1, 256, 1, 600) and np.isfinite(face["step1000"]).all()


@pytest.mark.parametrize("workload", ["body", "face"])
def test_oracle_chain_states_equal_the_references_own_chain(workload):
    """The oracle's FULL chains (body ddim100, face 1000-step DDPM with per-step noise) against the same chains run by the reference itself
    (tests/golden/make_golden_chain.py -> golden_chain_<workload>_ref_v1.npz): every stored state to 1e-5 (measured: body 7.4e-7 after 100 steps)."""
    import os
    import sys
    import numpy as np
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "tools"))
    import chain_vs_oracle as CVO
    orc = np.load(CVO.golden_path(workload))
    ref = np.load(CVO.golden_path(workload).replace("_v1.npz", "_ref_v1.npz"))
    steps = sorted(k for k in orc.files if k.startswith("step"))
    assert steps == sorted(k for k in ref.files if k.startswith("step"))
    for k in steps:
        a, b = ref[k].astype(np.float64), orc[k].astype(np.float64)
        assert np.linalg.norm(a - b) / np.linalg.norm(a) < 1e-5, (workload, k)
