"""The 16-bit logit envelope on the benchmarked kernels and loops (`pytest -m gpu`).

precision="fp16" promises the 1e-3 parity bar, or the sampling call moves itself to fp32 and returns the fp32 answer.  The switch is
decided by one number, the largest row maximum of q.k/sqrt(d_head) any denoiser attention saw (a2p_precision_verdict against
A2P_LOGIT_ENVELOPE_16BIT, include/a2p_hip.h; _lib.LOGIT_ENVELOPE_FP16).  tests/test_hip_round4.py checks it at B=1, T=240 -- the
small path (key-split attention).  Here:

  a. the headline path -- face B=8 T=600 (attn3_kernel for all 16 attentions, the tall chain kernels, final_layer fused into the
     last POST kernel) and body B=16 T=600 with keyframes -- and the B=1 small path at the scenarios near the bound, on synthetic
     weights pushed towards trained statistics (audio2photoreal_amd.synthetic.trained_like_state_dict), against the float64
     oracle: the device's logit maximum, the contract (inside => fp16 < 1e-3), and that the grid reaches the edge of the bound;
  b. the ddim10 loop's return value at the inside scenarios nearest the bound;
  c. escalation returns the fp32 bits in every sampling loop (ddim, ddpm with step noise, plms, inpainting, windowed).

Every number goes to record(...).  The CPU model of the same rounding sites (oracle/lowprec_model.py, attn_kernel and attn3
variants; tests/tools/trained_like_budget.py -> profiles/trained_like_envelope_*_T600.json) predicts these errors."""
import ctypes as C
import os
import warnings
from contextlib import contextmanager

import pytest
import torch

from audio2photoreal_amd import _lib
from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel
from audio2photoreal_amd.model_util import create_model_and_diffusion, default_args, load_model
from audio2photoreal_amd.spec import face_spec, pose_spec
from audio2photoreal_amd.synthetic import cond_tokens_for_frames, synthetic_inputs, synthetic_tensor, trained_like_state_dict
from conftest import record, rel_l2

pytestmark = pytest.mark.gpu
SEED = 10
BOUND = _lib.LOGIT_ENVELOPE_FP16

# name -> (trained_like_state_dict gains, {shape: (band of the float64 oracle's max |logit|, the device verdict at the shipped
# bound)}).  The bands (+-5 % around the measured peak) catch drift in the synthetic weights: a scenario that no longer peaks where
# it was placed fails here instead of quietly testing something else.
IN, OUT = "inside", "outside"


def _band(peak, verdict):
    return (round(0.95 * peak, 2), round(1.05 * peak, 2), verdict)


SCENARIOS = {
    "xavier": ({}, {"face_B8_T600": _band(3.50, IN), "body_B16_T600": _band(3.87, IN)}),
    "weights_x2": ({"weight_gain": 2.0}, {"face_B8_T600": _band(13.28, IN), "body_B16_T600": _band(15.40, IN)}),
    "qk_x2": ({"qk_gain": 2.0}, {"face_B8_T600": _band(13.89, IN), "body_B16_T600": _band(14.61, IN)}),
    "resid_1e3": ({"resid_gain": 1e3}, {"face_B8_T600": _band(3.44, IN), "body_B16_T600": _band(4.18, IN)}),
    "weights_x2_qk_x1.05": ({"weight_gain": 2.0, "qk_gain": 1.05}, {"face_B8_T600": _band(14.89, IN), "body_B16_T600": _band(17.14, IN),
                                                                    "face_B1_T240": _band(13.05, IN)}),
    "weights_x2_qk_x1.1": ({"weight_gain": 2.0, "qk_gain": 1.1}, {"face_B8_T600": _band(16.53, IN), "body_B16_T600": _band(18.82, IN),
                                                                  "face_B1_T240": _band(14.05, IN)}),
    "weights_x2_qk_x1.2": ({"weight_gain": 2.0, "qk_gain": 1.2}, {"face_B8_T600": _band(19.80, IN), "body_B16_T600": _band(21.61, OUT),
                                                                  "face_B1_T240": _band(17.43, IN)}),
    "qk_x2.2": ({"qk_gain": 2.2}, {"face_B8_T600": _band(17.04, IN), "body_B16_T600": _band(17.90, IN), "face_B1_T240": _band(15.72, IN)}),
    "qk_x2.5": ({"qk_gain": 2.5}, {"face_B8_T600": _band(22.09, OUT), "body_B16_T600": _band(23.38, OUT), "face_B1_T240": _band(19.34, IN)}),
    "qk_x3": ({"qk_gain": 3.0}, {"face_B8_T600": _band(30.36, OUT), "body_B16_T600": _band(35.03, OUT)}),
}
# KNOWN GAP of the one-number bound (measured; kept as expected failures until the envelope is redesigned): ordinary weight growth
# with slightly peaked attention misses the 1e-3 bar INSIDE the bound of 20 -- the error follows the activations' scale as much
# as the logit maximum (body rows at 18.8 hold 9.2e-4; face rows at 14.05 on the B=1 path do not).  Lowering the bound cannot
# close it: the B=1 path already reaches 9.1e-4 at 13.05, below the 13.5 the round-4 inside cases need.
VIOLATIONS = {
    ("face_B8_T600", "weights_x2_qk_x1.2"): (True, "fp16 1.19e-3 inside the bound (device max 19.0)"),
    ("face_B1_T240", "weights_x2_qk_x1.2"): (True, "fp16 1.39e-3 inside the bound (device max 16.4)"),
    ("face_B1_T240", "weights_x2_qk_x1.1"): (False, "fp16 1.04e-3 inside the bound (device max 14.1): 4 % over the bar"),
}
# bf16 is gated at about 2x what the GPU measured (the larger of the scenario's inside shapes; round 4's rule)
BF16_GATE = {"xavier": 7e-3, "weights_x2": 1.3e-2, "qk_x2": 9e-3, "resid_1e3": 2.5e-4, "weights_x2_qk_x1.05": 1.5e-2, "qk_x2.2": 1.1e-2,
             "weights_x2_qk_x1.1": 1.6e-2, "weights_x2_qk_x1.2": 2.2e-2, "qk_x2.5": 1.5e-2, "qk_x3": 8e-2}
SHAPES = {   # name -> (format, B, T, timesteps of the B samples)
    "face_B8_T600": ("face", 8, 600, [901, 417, 33, 650, 999, 0, 250, 777]),
    "body_B16_T600": ("pose", 16, 600, [901, 417, 33, 650, 999, 0, 250, 777] * 2),
    "face_B1_T240": ("face", 1, 240, [700]),
}
GRID = [(shape, name) for name, (_, bands) in SCENARIOS.items() for shape in SHAPES if shape in bands]
# attn3_kernel launches of one guided 16-bit forward (launch_attn's rule, a2p_lib.hip): face B=8 -- every self (600 keys, 256 or
# fewer attn3 workgroups) and cross (2000 keys) attention of the 8 layers; body B=16 -- head_dim 32 takes attn3 only from 1024 keys
# on: the audio cross attention of each of the 6 layers (its self attention has 600 keys, its keyframe attention 20 and is fused
# into the MID2 | keyframe | POST kernel); face B=1 T=240 -- the small path (key-split attention), no attn3 at all
ATTN3_LAUNCHES = {"face_B8_T600": 16, "body_B16_T600": 6, "face_B1_T240": 0}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    torch.set_num_threads(max(1, min(16, int(os.environ.get("OMP_NUM_THREADS") or 16))))   # the float64 oracle: 16 CPUs at most
    return torch.device("cuda:0")


def _debug_i64(model, name):
    n = C.c_int64(0)
    _lib.check(model._lib().a2p_debug_read(model._ctx, name, C.byref(n), 8), "a2p_debug_read")
    return int(n.value)


@contextmanager
def _logit_probe():
    """Records max |q.k/sqrt(dh)| over every DENOISER attention the float64 oracle computes (decoder_layer's self, cross and
    keyframe attentions; the conditioning encoder is not part of the device statistic either)."""
    from oracle import a2p_oracle as O
    mha, layer, state = O.mha, O.decoder_layer, {"in_layer": False, "peak": 0.0}

    def probed_mha(q_in, k_in, v_in, in_w, in_b, out_w, out_b, nheads):
        if state["in_layer"]:
            d = q_in.shape[-1]
            dh = d // nheads
            q = (q_in @ in_w[:d].T + in_b[:d]).unflatten(-1, (nheads, dh)).transpose(1, 2)
            k = (k_in @ in_w[d:2 * d].T + in_b[d:2 * d]).unflatten(-1, (nheads, dh)).transpose(1, 2)
            state["peak"] = max(state["peak"], float((q @ k.transpose(-1, -2)).abs().amax()) / dh ** 0.5)
        return mha(q_in, k_in, v_in, in_w, in_b, out_w, out_b, nheads)

    def probed_layer(*a, **kw):
        state["in_layer"] = True
        try:
            return layer(*a, **kw)
        finally:
            state["in_layer"] = False
    O.mha, O.decoder_layer = probed_mha, probed_layer
    try:
        yield state
    finally:
        O.mha, O.decoder_layer = mha, layer


def _scenario(shape, name):
    """State dict with the output head rescaled so that the float64 oracle's guided output of the batch has unit scale (the last
    linear map: the oracle output scales by exactly 1/g), inputs, timesteps, the oracle's output and its logit peak."""
    from oracle import a2p_oracle as O
    fmt, B, T, ts = SHAPES[shape]
    spec = face_spec() if fmt == "face" else pose_spec()
    sd = trained_like_state_dict(spec, SEED, **SCENARIOS[name][0])
    inp = synthetic_inputs(spec, B, T, SEED)
    times = torch.tensor(ts)
    scale = torch.full((B,), 10.0 if fmt == "face" else 2.0)
    den = O.OracleDenoiser(sd, fmt, spec.num_layers, spec.num_heads, torch.float64)
    outs = []
    with torch.no_grad(), _logit_probe() as probe:
        for b in range(0, B, 4):                       # 4 samples at a time: float64 scores of 600 x 2000 keys per head
            s = slice(b, b + 4)
            kf, mk = (inp["keyframes"][s], inp["mask"][s]) if spec.is_pose else (None, None)
            outs.append(den.forward_cfg(inp["x_T"][s], times[s], inp["cond_embed"][s], scale[s], kf, mk))
    raw = torch.cat(outs)
    g = float(raw.std())
    head = [k for k in sd if k.startswith("final_conv.")] if spec.is_pose else ["final_layer.weight", "final_layer.bias"]
    for k in head:
        sd[k] = sd[k] / g
    return spec, sd, inp, times, scale, raw / g, probe["peak"]


def _y(spec, inp, scale, dev):
    y = {"cond_embed": inp["cond_embed"].to(dev), "scale": scale.to(dev)}
    if spec.is_pose:
        y["keyframes"], y["mask"] = inp["keyframes"].to(dev), inp["mask"].to(dev)
    return y


def _verdict(model):
    """(outside?, device logit maximum): a2p_precision_verdict through check_finite (auto_escalate off: warn and return)."""
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        model.check_finite()
    return any(issubclass(x.category, _lib.A2PPrecisionWarning) for x in w), model.last_logit_max


# ----------------------------------------------------------------------------- a. the headline forward grid
def test_the_grid_reaches_the_edge_of_the_envelope():
    """At least one scenario pinned inside the bound peaks at >= 0.9 x the bound on the headline face path and on the B=1 path
    (its band and verdict are asserted against the oracle and the device in the grid below), so the bound is measured where it
    bites."""
    for shape in ("face_B8_T600", "face_B1_T240"):
        edge = [n for n, (_, bands) in SCENARIOS.items() if shape in bands and bands[shape][2] == IN and bands[shape][0] >= 0.9 * BOUND]
        assert edge, (shape, BOUND)


@pytest.mark.parametrize("shape,name", GRID)
def test_16bit_forward_inside_the_envelope_holds_the_bar(dev, shape, name, monkeypatch):
    spec, sd, inp, times, scale, want, peak = _scenario(shape, name)
    fmt, B, T, _ = SHAPES[shape]
    lo, hi, expected = SCENARIOS[name][1][shape]
    if fmt == "face" and B >= 8:
        monkeypatch.setenv("A2P_CHAIN_V", "4")     # the tall family, as tests/test_hip_round6.py forces it
    y = _y(spec, inp, scale, dev)
    x, t = inp["x_T"].to(dev), times.to(dev)
    res = {}
    for precision in ("fp32", "fp16", "bf16"):
        model, _ = create_model_and_diffusion(default_args(fmt), "test", precision=precision, max_batch=B, auto_escalate=False)
        load_model(model, sd)
        cfg = ClassifierFreeSampleModel(model.to(dev).eval())
        cfg(x, t, y)                                    # context + hoisted conditioning (its cond-encoder attentions: first call only)
        _verdict(model)
        before = {k: _debug_i64(model, k.encode()) for k in ("attn3_launches", "chain4_launches", "final_fused_launches")}
        got = cfg(x, t, y).cpu()
        launched = {k: _debug_i64(model, k.encode()) - v for k, v in before.items()}
        outside, dmax = _verdict(model)
        model.release()
        res[precision] = {"rel_l2": rel_l2(got, want), "worst_sample_rel_l2": max(rel_l2(got[b], want[b]) for b in range(B)),
                          "device_logit_max": dmax, "outside": outside, **launched}
    record(f"envelope/{shape}/{name}", oracle_logit_peak=peak, bound=BOUND, **{f"{p}_{k}": v for p, r in res.items() for k, v in r.items()})
    f32, f16, b16 = res["fp32"], res["fp16"], res["bf16"]
    # the path is the headline one
    assert f32["attn3_launches"] == 0 and f16["attn3_launches"] == b16["attn3_launches"] == ATTN3_LAUNCHES[shape], res
    if fmt == "face" and B >= 8:
        assert f16["chain4_launches"] == b16["chain4_launches"] == 17, res          # 8 MID + 8 POST + the fused input projection / PRE
        assert f16["final_fused_launches"] == b16["final_fused_launches"] == 1, res
    # the device statistic (attn3: m_ref + the relative running maximum, in natural units) against the oracle's peak
    assert f32["device_logit_max"] <= peak * 1.001 + 1e-3 and f32["device_logit_max"] > 0.3 * peak, (res, peak)
    for p in ("fp16", "bf16"):
        assert abs(res[p]["device_logit_max"] - f32["device_logit_max"]) < 0.08 * abs(f32["device_logit_max"]) + 0.05, (p, res)
    # teeth: the scenario peaks where it was placed
    assert lo <= peak <= hi, (peak, lo, hi)
    assert f32["rel_l2"] < 1e-4 and not f32["outside"], res
    # the contract: inside the bound fp16 holds the bar, outside it the oracle is outside too
    assert f16["outside"] == b16["outside"], res
    assert f16["outside"] == (expected == OUT), (expected, res, peak)
    if not f16["outside"]:
        assert b16["rel_l2"] < BF16_GATE[name], res
        holds = f16["rel_l2"] < 1e-3 and f16["worst_sample_rel_l2"] < 1.5e-3
        strict, why = VIOLATIONS.get((shape, name), (None, None))
        if why is not None and not holds:
            pytest.xfail(why)                         # every other assertion above ran for real
        assert not strict, f"{shape}/{name} was a known violation of the bar and now holds it: update VIOLATIONS ({res})"
        assert holds, res
    else:
        assert peak > BOUND and f16["device_logit_max"] > BOUND, (res, peak)


# ----------------------------------------------------------------------------- b. the loop's return value at the edge
# the two scenarios pinned inside the bound nearest to it on the headline face path
EDGE = sorted((n for n, (_, b) in SCENARIOS.items() if "face_B8_T600" in b and b["face_B8_T600"][2] == IN),
              key=lambda n: SCENARIOS[n][1]["face_B8_T600"][0])[-2:]


@pytest.mark.parametrize("name", EDGE)
def test_fp16_ddim10_loop_at_the_edge_of_the_envelope(dev, name):
    """Face B=8 T=600 ddim10 in fp16 (auto_escalate on) against the float64 oracle's ddim10 loop on two of the eight samples (the
    samples of a batch are independent).  Not escalated: < 1e-3.  Escalated: the fp32 answer (the escalation test below)."""
    from oracle import a2p_oracle as O
    spec = face_spec()
    B, T, pick = 8, 600, [0, 5]
    sd = trained_like_state_dict(spec, SEED, **SCENARIOS[name][0])
    inp = synthetic_inputs(spec, B, T, SEED)
    scale = torch.full((B,), 10.0)
    den = O.OracleDenoiser(sd, "face", spec.num_layers, spec.num_heads, torch.float64)
    with torch.no_grad():
        g = float(den.forward_cfg(inp["x_T"][:1], torch.tensor([700]), inp["cond_embed"][:1], scale[:1]).std())
    for k in ("final_layer.weight", "final_layer.bias"):
        sd[k] = sd[k] / g
    den = O.OracleDenoiser(sd, "face", spec.num_layers, spec.num_heads, torch.float64)
    with torch.no_grad():
        fn = lambda xx, ts: den.forward_cfg(xx, ts, inp["cond_embed"][pick], scale[pick])
        want = O.OracleSampler("ddim10").ddim_sample_loop(fn, inp["x_T"][pick].double())[0]           # pred_xstart [2, C, 1, T]
    model, diffusion = create_model_and_diffusion(default_args("face", timestep_respacing="ddim10"), "test", precision="fp16", max_batch=B)
    load_model(model, sd)
    cfg = ClassifierFreeSampleModel(model.to(dev).eval())
    y = {"cond_embed": inp["cond_embed"].to(dev), "scale": scale.to(dev)}
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        got = diffusion.ddim_sample_loop(cfg, (B, spec.nfeats, 1, T), clip_denoised=False, model_kwargs={"y": y},
                                         noise=inp["x_T"].to(dev)).cpu()
    warned = sum(issubclass(x.category, _lib.A2PPrecisionWarning) for x in w)
    escalated, dmax = model.escalated_from is not None, model.last_logit_max
    model.release()
    err = rel_l2(got[pick], want)
    record(f"envelope_loop/face_B8_T600_ddim10/{name}", rel_l2=err, escalated=escalated, warnings=warned, device_logit_max=dmax, bound=BOUND)
    assert torch.isfinite(got).all()
    if not escalated:
        assert warned == 0, (err, dmax)
        if err >= 1e-3 and ("face_B8_T600", name) in VIOLATIONS:
            pytest.xfail("the forward misses the bar here: " + VIOLATIONS["face_B8_T600", name][1])
        assert err < 1e-3, (err, dmax)
    else:
        assert warned == 1 and model.precision == "fp32" and err < 1e-3, (err, dmax)


# ----------------------------------------------------------------------------- c. escalation returns the fp32 bits in every loop
def _qk3(B, T):
    from oracle import a2p_oracle as O
    spec = face_spec()
    sd = trained_like_state_dict(spec, SEED, qk_gain=3.0)
    inp = synthetic_inputs(spec, 1, T, SEED)
    with torch.no_grad():
        g = float(O.OracleDenoiser(sd, "face", spec.num_layers, spec.num_heads).forward_cfg(
            inp["x_T"], torch.tensor([700]), inp["cond_embed"], torch.full((1,), 10.0)).std())
    for k in ("final_layer.weight", "final_layer.bias"):
        sd[k] = sd[k] / g
    return spec, sd


def _escalation_pair(dev, B, respacing, run):
    """run(diffusion, cfg, spec, dev) -> output, once on an fp16 model with auto_escalate and once on a fresh fp32 model."""
    spec, sd = _qk3(B, 240)
    out = {}
    for precision in ("fp16", "fp32"):
        model, diffusion = create_model_and_diffusion(default_args("face", timestep_respacing=respacing), "test", precision=precision,
                                                      max_batch=B)
        load_model(model, sd)
        cfg = ClassifierFreeSampleModel(model.to(dev).eval())
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter("always")
            got = run(diffusion, cfg, spec, dev).cpu()
        out[precision] = {"out": got, "warnings": sum(issubclass(x.category, _lib.A2PPrecisionWarning) for x in w),
                          "precision_after": model.precision, "escalated_from": model.escalated_from, "logit_max": model.last_logit_max}
        model.release()
    return out


def _face_y(B, T, dev, seed=SEED):
    return {"cond_embed": synthetic_tensor(seed, "cond_embed", (B, cond_tokens_for_frames(T), face_spec().cond_feature_dim)).to(dev),
            "scale": torch.full((B,), 10.0, device=dev)}


def _loop_ddim(diffusion, cfg, spec, d, B=2, T=240):
    return diffusion.ddim_sample_loop(cfg, (B, spec.nfeats, 1, T), clip_denoised=False, model_kwargs={"y": _face_y(B, T, d)},
                                      noise=synthetic_tensor(SEED, "x_T", (B, spec.nfeats, 1, T)).to(d))


def _loop_ddpm(diffusion, cfg, spec, d, B=2, T=240):
    steps = synthetic_tensor(SEED, "step_noise", (diffusion.num_timesteps, B, spec.nfeats, 1, T)).to(d)
    return diffusion.p_sample_loop(cfg, (B, spec.nfeats, 1, T), clip_denoised=False, model_kwargs={"y": _face_y(B, T, d)},
                                   noise=synthetic_tensor(SEED, "x_T", (B, spec.nfeats, 1, T)).to(d), step_noise=list(steps))


def _loop_plms(diffusion, cfg, spec, d, B=2, T=240):
    return diffusion.plms_sample_loop(cfg, (B, spec.nfeats, 1, T), clip_denoised=False, model_kwargs={"y": _face_y(B, T, d)},
                                      noise=synthetic_tensor(SEED, "x_T", (B, spec.nfeats, 1, T)).to(d))


def _loop_inpaint(diffusion, cfg, spec, d, B=2, T=240):
    from audio2photoreal_amd.sample.inpaint import inpaint_sample_loop
    known = synthetic_tensor(SEED, "known", (B, spec.nfeats, 1, T)).to(d)
    mask = torch.zeros(B, T, dtype=torch.bool)
    mask[:, :60] = True                                  # held context frames, as clip continuation holds them
    mask[1, 200:] = True
    return inpaint_sample_loop(diffusion, cfg, _face_y(B, T, d), known, mask.to(d),
                               synthetic_tensor(SEED, "x_T", (B, spec.nfeats, 1, T)).to(d))


def _loop_windowed(diffusion, cfg, spec, d, B=2, T=240):
    from audio2photoreal_amd.sample.long_form import plan_windows, windowed_sample_loop
    plan = plan_windows(360, T_w=T)
    assert plan.W == B == 2, plan
    return windowed_sample_loop(diffusion, cfg, plan, 1, _face_y(B, T, d), synthetic_tensor(SEED, "x_T", (1, spec.nfeats, 1, 360)).to(d))


@pytest.mark.parametrize("loop", ["ddim", "ddpm", "plms", "inpaint", "windowed"])
def test_escalated_fp16_loop_returns_the_fp32_bits(dev, loop):
    """q/k rows x3 (row maxima ~29, outside the bound), face B=2 T=240, ddim5: an fp16 model with auto_escalate returns exactly what
    a fresh fp32 model returns from the same inputs, warns once and stays in fp32 (`escalated_from` = "fp16")."""
    run = {"ddim": _loop_ddim, "ddpm": _loop_ddpm, "plms": _loop_plms, "inpaint": _loop_inpaint, "windowed": _loop_windowed}[loop]
    out = _escalation_pair(dev, 2, "ddim5", run)
    e, f = out["fp16"], out["fp32"]
    equal = torch.equal(e["out"], f["out"])
    record(f"envelope_escalation/face_B2_T240/{loop}", equal=equal, max_abs_diff=float((e["out"] - f["out"]).abs().max()),
           warnings=e["warnings"], precision_after=e["precision_after"], escalated_from=e["escalated_from"], logit_max=e["logit_max"])
    assert e["precision_after"] == "fp32" and e["escalated_from"] == "fp16" and e["warnings"] == 1, e
    assert f["warnings"] == 0 and f["escalated_from"] is None, f
    assert torch.isfinite(f["out"]).all() and equal


def test_escalated_fp16_loop_at_the_headline_shape_returns_the_fp32_bits(dev):
    """The same at face B=8 T=600 ddim5: the first step runs the headline kernels (attn3, tall chain) before the switch."""
    B, T = 8, 600
    out = _escalation_pair(dev, B, "ddim5", lambda diffusion, cfg, spec, d: _loop_ddim(diffusion, cfg, spec, d, B, T))
    e, f = out["fp16"], out["fp32"]
    equal = torch.equal(e["out"], f["out"])
    record("envelope_escalation/face_B8_T600/ddim", equal=equal, max_abs_diff=float((e["out"] - f["out"]).abs().max()),
           warnings=e["warnings"], precision_after=e["precision_after"], escalated_from=e["escalated_from"], logit_max=e["logit_max"])
    assert e["precision_after"] == "fp32" and e["escalated_from"] == "fp16" and e["warnings"] == 1, e
    assert torch.isfinite(f["out"]).all() and equal
