"""oracle/lowprec_model.py (the CPU model of the GPU's 16-bit rounding sites behind tests/tools/error_budget.py) against the
oracle: with every site in fp32 it IS the oracle, and with IEEE-half sites it reproduces the orders of magnitude the GPU
measures (profiles/r03_error_budget.json holds the full-size run)."""
import torch

from audio2photoreal_amd.spec import face_spec, pose_spec
from audio2photoreal_amd.synthetic import synthetic_inputs, synthetic_state_dict, trained_like_state_dict
from oracle import a2p_oracle as O
from oracle import lowprec_model as LP


def _run(fmt, rounding, T=48, layers=2, **trained_like):
    spec = (face_spec if fmt == "face" else pose_spec)(num_layers=layers)
    sd = trained_like_state_dict(spec, 10, **trained_like) if trained_like else synthetic_state_dict(spec, 10)
    inp = synthetic_inputs(spec, 2, T, 10)
    kf, mk = (inp["keyframes"], inp["mask"]) if spec.is_pose else (None, None)
    scale = torch.full((2,), 10.0 if fmt == "face" else 2.0)
    t = torch.tensor([700, 12])
    with torch.no_grad():
        want = O.OracleDenoiser(sd, fmt, layers, spec.num_heads).forward_cfg(inp["x_T"], t, inp["cond_embed"], scale, kf, mk)
        got = LP.LowPrecDenoiser(sd, fmt, layers, spec.num_heads, rounding).forward_cfg(inp["x_T"], t, inp["cond_embed"], scale, kf, mk)
    return float((got - want).norm() / want.norm())


def test_all_sites_fp32_is_the_oracle():
    for fmt in ("face", "pose"):
        assert _run(fmt, LP.Rounding("fp32")) < 5e-6


def test_half_sites_are_ordered_like_the_formats():
    e16, eb16 = _run("face", LP.Rounding("fp16")), _run("face", LP.Rounding("bf16"))
    assert 1e-5 < e16 < 3e-3 and 4.0 * e16 < eb16 < 16.0 * e16          # 3 mantissa bits apart
    exact_tail = {s: "fp32" for s in ("fin.a", "fin.w", "in.a", "in.w")}
    assert _run("face", LP.Rounding("fp16", exact_tail)) < e16
    assert _run("face", LP.Rounding("fp16", {"fin.a": "fp16x2"})) < e16  # the hi + lo pair is as good as exact for that site


def test_attn3_variant_with_fp32_sites_is_the_oracle():
    """Rounding(attn="attn3") restates kernels_attn3.h (Q pre-scaled by log2(e)/sqrt(dh), exp2 numerators, row sums over P):
    with nothing rounded it is the same softmax."""
    for fmt in ("face", "pose"):
        assert _run(fmt, LP.Rounding("fp32", attn="attn3")) < 5e-6


def test_attn3_variant_rounds_like_attn_kernel_and_more_with_peaked_logits():
    """IEEE-half sites: the attn3 restatement has an error of its own, of the attn_kernel variant's order (one extra rounding of
    Q, row sums over the rounded P), and like it the error grows as q / k rows grow (peakier softmax rows, larger logits)."""
    for fmt in ("face", "pose"):
        e1 = _run(fmt, LP.Rounding("fp16"))
        e3 = _run(fmt, LP.Rounding("fp16", attn="attn3"))
        assert e3 > 1e-5 and e3 != e1 and 0.3 * e1 < e3 < 3.0 * e1, (fmt, e1, e3)
    e = {g: _run("face", LP.Rounding("fp16", attn="attn3"), qk_gain=g) for g in (1.0, 2.0, 3.0)}
    assert e[1.0] < e[2.0] < e[3.0], e


def test_the_probe_reports_the_same_logit_peak_for_both_kernels():
    """The probe records max |q.k/sqrt(dh)| in natural units whichever kernel's rounding is modelled (attn3 computes in log2 units)."""
    peaks = {}
    for attn in ("attn_kernel", "attn3"):
        probe = LP.Rounding("fp32", attn=attn)
        probe.logit_peak = 0.0
        _run("face", probe, qk_gain=2.0)
        peaks[attn] = probe.logit_peak
    assert peaks["attn_kernel"] > 1.0 and abs(peaks["attn3"] - peaks["attn_kernel"]) < 1e-4 * peaks["attn_kernel"], peaks


def test_envelope_constant_of_the_header_is_the_python_mirror():
    """A2P_LOGIT_ENVELOPE_16BIT (include/a2p_hip.h: the device verdict a2p_precision_verdict) and _lib.LOGIT_ENVELOPE_FP16 (the
    warning text, the tests) are two copies of one bound."""
    import os
    import re
    from audio2photoreal_amd import _lib
    from conftest import ROOT
    src = open(os.path.join(ROOT, "include", "a2p_hip.h")).read()
    m = re.findall(r"^\s*#define\s+A2P_LOGIT_ENVELOPE_16BIT\s+([0-9.eE+-]+)f?\b", src, re.M)
    assert len(m) == 1, m
    assert float(m[0]) == _lib.LOGIT_ENVELOPE_FP16, (m[0], _lib.LOGIT_ENVELOPE_FP16)
