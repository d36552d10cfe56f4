"""The reference side of tests/test_forward_paths_{cpu,hip}.py: inputs of a shallow case, the float64 oracle of the same depth, the per-element
statistic, the envelope of the CPU model of the 16-bit rounding sites (oracle/lowprec_model.py) and the seeded faults the gate has to see.
Test infrastructure: pure CPU, no library.

Statistic of an output against the float64 oracle: e = |got - want| / rms(want over that sequence), reported as (max e, rms e).
Envelope of a (case shape, mode): the statistic of LP.LowPrecDenoiser with the site formats of the mode, the larger of the two attention variants;
float64 between the sites, so that the numbers do not depend on the CPU's fp32 summation order (threads 1 / 3 / 8: the same to 3e-7; in fp32 they
moved by up to 5 %).
Gate: 4 x the envelope -- the margin tests/test_steer_hip.py gives a restatement's own rounding error; it covers what the model does not restate
(accumulation order, the hardware exp2, LayerNorm tree order) and is far below the seeded faults (1e-2 .. 1)."""
import contextlib
import json
import os

import torch

import chain_plan_restatement as R
from audio2photoreal_amd.spec import face_spec, pose_spec
from audio2photoreal_amd.synthetic import synthetic_inputs, synthetic_state_dict
from oracle import a2p_oracle as O
from oracle import lowprec_model as LP

SEED = 10
MARGIN = 4.0
FP32_GATE = 1e-3                                       # the project's parity bar, for precision="fp32"
TIMES, SCALES = (901, 417, 33), (0.5, 2.0, 1.5)        # per sample, cycled: FiLM rows differ per sample, both guidance halves carry O(1) weight
ENVELOPE_FILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_paths_envelope.json")
EXACT_SITES = ("fin.a", "fin.w", "in.a", "in.w", "tail.a", "tail.w")      # the split-operand islands (tests/tools/trained_like_budget.py)


@contextlib.contextmanager
def oracle_threads():
    """The oracle is sized for up to 16 CPU threads, whatever the suite's default."""
    before = torch.get_num_threads()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    try:
        yield
    finally:
        torch.set_num_threads(before)


def spec_of(case):
    return (face_spec if case.fmt == "face" else pose_spec)(num_layers=case.layers)


_SD = {}


def state_dict(case):
    key = (case.fmt, case.layers)
    if key not in _SD:
        _SD[key] = synthetic_state_dict(spec_of(case), SEED)
    return _SD[key]


def inputs(case):
    """CPU tensors of the case: x [B, C, 1, T], t, scale, cond_embed, keyframes / mask (body; sample 1's keyframes are masked out from frame 40 on),
    noise (the DDPM step)."""
    spec, B, T = spec_of(case), case.B, case.T
    inp = synthetic_inputs(spec, B, T, SEED)
    out = {"x": inp["x_T"], "cond_embed": inp["cond_embed"], "t": torch.tensor((TIMES * 9)[:B]), "scale": torch.tensor((SCALES * 9)[:B]),
           "keyframes": None, "mask": None}
    if spec.is_pose:
        out["keyframes"], out["mask"] = inp["keyframes"], inp["mask"].clone()
        out["mask"][1, :, :, 40:] = False
    if case.ddpm_step:
        out["noise"] = torch.randn(inp["x_T"].shape, generator=torch.Generator().manual_seed(SEED + 1))
    return out


def smix_samples(case):
    """The samples of a mixed-height launch the oracle runs on (sequences are independent): those whose conditional or unconditional rows contain row
    64 * n_tall -- where the 64-row panels end and the 48-row panels begin --, sample 0 and the last one."""
    mix = [p for p in R.expected(case)["picks"] if p[R.FIELDS.index("variant")] == R.MIX]
    rows = {64 * p[R.FIELDS.index("n_tall")] for p in mix}
    return sorted({0, case.B - 1} | {(r // case.T) % case.B for r in rows})


def run_denoiser(den, case, inp, samples=None):
    """{name: [B', T, C]} of the case on a denoiser of the oracle's interface: the (guided) forward, or sample / pred_xstart of one DDPM step."""
    idx = slice(None) if samples is None else list(samples)
    pick = lambda v: None if v is None else v[idx]
    x, t, ce, sc, kf, mk = (pick(inp[k]) for k in ("x", "t", "cond_embed", "scale", "keyframes", "mask"))
    dt = den.dtype
    with torch.no_grad():
        if case.ddpm_step:
            fn = lambda xx, ts: den.forward_cfg(xx, ts, ce, sc, kf, mk)
            res = O.OracleSampler("").p_sample(fn, x.to(dt), t, pick(inp["noise"]).to(dt))
            return {k: res[k].squeeze(2).permute(0, 2, 1) for k in ("sample", "pred_xstart")}
        if case.guided:
            return {"out": den.forward_cfg(x, t, ce, sc, kf, mk)}
        return {"out": den.forward(x, t, ce, kf, mk, 0.0)}


def shape_key(case):
    """What the float64 oracle and the envelope depend on: not on the switches."""
    return (f"{case.fmt}/L{case.layers}/B{case.B}xT{case.T}/" + ("ddpm" if case.ddpm_step else "guided" if case.guided else "unguided"))


_REF = {}


def reference(case, samples=None):
    """The float64 oracle's outputs of the case, computed once per shape and shared (read-only)."""
    key = (shape_key(case), None if samples is None else tuple(samples))
    if key not in _REF:
        spec = spec_of(case)
        den = O.OracleDenoiser(state_dict(case), case.fmt, case.layers, spec.num_heads, torch.float64)
        with oracle_threads():
            _REF[key] = run_denoiser(den, case, inputs(case), samples)
    return _REF[key]


def element_errors(got, want):
    """e [B, T, C] in float64."""
    got, want = got.double(), want.double()
    rms = want.pow(2).mean(dim=(1, 2), keepdim=True).sqrt()
    return (got - want).abs() / rms


def statistic(got, want):
    e = element_errors(got, want)
    return float(e.max()), float(e.pow(2).mean().sqrt())


def worst_element(got, want):
    e = element_errors(got, want)
    b, f, c = (int(v) for v in torch.unravel_index(e.argmax(), e.shape))
    return b, f, c, float(e[b, f, c])


def mode_of(precision, tail16=False):
    return precision + ("_tail16" if tail16 else "")


def rounding(mode, attn):
    """Site formats of a mode: the split-operand islands see a hi + lo half pair (fp16) or are modelled exact (bf16); under A2P_TAIL16 they are plain
    16-bit operands of the build's format."""
    base = mode.split("_")[0]
    island = base if mode.endswith("_tail16") else ("fp16x2" if base == "fp16" else "fp32")
    return LP.Rounding(base, {s: island for s in EXACT_SITES}, attn=attn)


def lowprec_outputs(case, mode, attn, samples=None, inp=None):
    spec = spec_of(case)
    # float64 between the rounding sites: the envelope is then the same on every CPU and thread count (fp32 accumulation order is not)
    den = LP.LowPrecDenoiser(state_dict(case), case.fmt, case.layers, spec.num_heads, rounding(mode, attn), dtype=torch.float64)
    with oracle_threads():
        return run_denoiser(den, case, inp or inputs(case), samples)


def compute_envelope(case, mode):
    """{output name: [max e, rms e]}: the larger of the two attention variants, element for element of the pair."""
    samples = smix_samples(case) if case.B == R.SMIX[0] else None
    want = reference(case, samples)
    env = {}
    for attn in ("attn_kernel", "attn3"):
        got = lowprec_outputs(case, mode, attn, samples)
        for k in want:
            mx, rm = statistic(got[k], want[k])
            env[k] = [max(mx, env.get(k, [0, 0])[0]), max(rm, env.get(k, [0, 0])[1])]
    return env


def load_envelopes():
    with open(ENVELOPE_FILE) as f:
        return json.load(f)


def envelope(case, mode, name="out"):
    """(max e, rms e) of the committed envelope file."""
    return tuple(load_envelopes()[shape_key(case)][mode][name])


def envelope_cases():
    """One case per (shape key, tail16) of SHALLOW_CASES: what the envelope file holds."""
    seen = {}
    for c in R.SHALLOW_CASES:
        seen.setdefault((shape_key(c), c.tail16), c)
    return seen


# ---- seeded faults (tests/test_forward_paths_cpu.py): each returns a faulted copy of the low-precision model's output `got` [B, T, C] of `case`
def fault_zero_row(case, got):
    out = got.clone()
    out[1, case.T // 2] = 0.0
    return out


def fault_film_of_previous_sequence(case, mode, got, panel=48):
    """The rows of the first `panel`-row panel that straddles sequences 0 and 1 which belong to sequence 1 get sequence 0's FiLM: recomputed with
    sample 0's timestep for sample 1."""
    T = case.T
    first = (T // panel) * panel                       # the panel [first, first + panel) holds rows of sequence 0 and of sequence 1
    assert first < T < first + panel, (T, panel)
    inp = inputs(case)
    inp["t"] = inp["t"].clone()
    inp["t"][1] = inp["t"][0]
    wrong = lowprec_outputs(case, mode, "attn_kernel", inp=inp)["out"]
    out = got.clone()
    n = first + panel - T                              # frames of sequence 1 inside that panel
    out[1, :n] = wrong[1, :n]
    return out


def fault_stale_last_panel(case, got, panel=48):
    """The last M mod panel rows hold the previous panel's rows."""
    B, T, C = got.shape
    flat = got.reshape(B * T, C).clone()
    r = (B * T) % panel
    assert r, (B, T, panel)
    flat[B * T - r:] = flat[B * T - r - panel: B * T - panel]
    return flat.reshape(B, T, C)


def fault_scaled_slice(case, got):
    """One 16-column slice of one row times 1 + 2^-6: the slice that holds sample 0's largest element (a relative fault shows where the values are)."""
    out = got.clone()
    f, c = (int(v) for v in torch.unravel_index(got[0].abs().argmax(), got[0].shape))
    c0 = min(c // 16 * 16, got.shape[2] - 16)
    out[0, f, c0:c0 + 16] *= 1.0 + 2.0 ** -6
    return out
