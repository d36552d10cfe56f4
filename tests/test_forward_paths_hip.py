"""Every chain kernel instance of csrc/a2p_lib_run.h kChainInst -- and the small-forward, per-op and fp32 paths -- element by element against the
float64 oracle, on 1- and 2-layer synthetic models at the smallest shapes that have the edges (tests/chain_plan_restatement.py SHALLOW_CASES: ragged
last panels, panels and 16-row tiles that straddle sequences, V^T groups that straddle sequences, mixed panel heights).  Per case: the pick log equals
the restated rule (the instance meant is the instance run), the output is finite and repeats bit for bit, and e = |got - want| / rms(want of that
sequence) stays within 4 x the envelope of the CPU model of the 16-bit rounding sites (tests/golden/forward_paths_envelope.json, reproduced by
tests/test_forward_paths_cpu.py; gate and margin: tests/forward_paths_oracle.py).  The gate comes from the reference side and is not tuned on the kernels.
Bit equality is asserted where the project claims it (families, wave counts, fused input / final kernels, mixed against uniform launches), never across
panel heights or between MIDPOST and A2P_NO_FUSED_KF.

Measured / envelope ratios of every case are recorded (conftest.record) under forward_paths/<mode>/<case>.
Worst measured / envelope ratio per mode on the MI355X (max e, rms e; the gate is 4): fp16 1.09, 1.01 (the DDPM step's pred_xstart); fp16 with
A2P_TAIL16 1.11, 0.99; bf16 1.06, 1.00 (body, 3 x 50, 32-row panels); bf16 with A2P_TAIL16 0.84, 1.01.  Every rms ratio lies in 0.98 .. 1.01: the CPU
model predicts the kernels' error.  fp32 mode: max e 6.4e-6 against the 1e-3 bar.  The whole file takes 11 s.
"""
import ctypes as C
import dataclasses

import pytest
import torch

import chain_plan_restatement as R
import forward_paths_oracle as FP
from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel
from audio2photoreal_amd.model_util import create_model_and_diffusion, default_args, load_model
from conftest import record
from test_chain_plan_hip import COUNTERS, describe, read_int, read_picks, switches

pytestmark = pytest.mark.gpu
PRECISIONS = ("fp16", "bf16")

# the forward paths beside the chain kernels, through the same harness; their pick log is empty
_face = dict(fmt="face", guided=True, layers=2)
OTHER_CASES = (
    R.Case("face_S88_small", B=2, T=88, **_face),                                       # 352 and 300 rows: below the chain threshold, the small-forward kernels
    R.Case("face_S50_small", B=3, T=50, **_face),
    R.Case("face_S88_per_op", B=2, T=88, env=R._e(NO_CHAIN=1, NO_SMALL=1), **_face),
    R.Case("pose_S88_per_op", "pose", 2, 88, True, R._e(NO_CHAIN=1, NO_SMALL=1), layers=2),
)
OTHER_BY_NAME = {c.name: c for c in OTHER_CASES}
NO_MIX = dataclasses.replace(R.SHALLOW_BY_NAME["face_SMIX"], name="face_SMIX_no_mix", env=R._e(CHAIN_V=1, CHAIN_NO_MIX=1),
                             hits=tuple(R._gen1_hits(512, 3, 8, 1, pre=(1, 512, 2, 8, R.PRE, R.UNIFORM))))
# pairs whose full outputs the project claims to be the same bits, at S88 (and the mixed launch on all 24960 rows)
BIT_PAIRS = (
    ("face_S88_tall_mt3", "face_S88_gen1_mt3_nw8"),                                     # tall == generation 1
    ("face_S88_tall_mt4", "face_S88_gen1_mt4_nw8"),
    ("face_S88_gen1_mt3_nw4", "face_S88_gen1_mt3_nw8"),                                 # 4 waves == 8 waves
    ("pose_S88_midpost_mt3_nw4", "pose_S88_midpost_mt3_nw8"),
    ("face_S88_tall_mt3_no_fused_in", "face_S88_tall_mt3"),
    ("face_S88_tall_mt4_no_fused_in", "face_S88_tall_mt4"),
    ("face_S88_tall_mt3_no_fused_final", "face_S88_tall_mt3"),
    ("face_S88_tall_mt5_no_fused_final", "face_S88_tall_mt5"),
    ("face_SMIX", "face_SMIX_no_mix"),
)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models():
    """Contexts shared by the cases of one (model, precision, layers, A2P_TAIL16, batch capacity); outputs shared by the tests that compare them."""
    cache = {"outputs": {}}
    yield cache
    for key, val in cache.items():
        if key != "outputs":
            val[0].release()


def case_of(name):
    return NO_MIX if name == NO_MIX.name else R.SHALLOW_BY_NAME.get(name) or OTHER_BY_NAME[name]


def get_model(models, case, precision, dev):
    cap = 26 if case.B > 8 else 8
    key = (case.fmt, precision, case.layers, case.tail16, cap)
    if key not in models:
        with switches(case, case.tail16):          # A2P_TAIL16 is read when the context is created and the weights are finalized
            model, diffusion = create_model_and_diffusion(default_args(case.fmt, layers=case.layers), "test", precision=precision, max_batch=cap)
            load_model(model, FP.state_dict(case))
            model = model.to(dev).eval()
            model._ensure_ctx(dev, cap)
            model._ensure_weights(model._lib(), dev)
        models[key] = (model, diffusion)
    return models[key]


def make_step(case, model, diffusion, dev):
    """The case's forward (or guided DDPM step) as a closure over its inputs: () -> {name: [B, T, C] on the CPU}."""
    inp = FP.inputs(case)
    x, t = inp["x"].to(dev), inp["t"].to(dev)
    y = {"cond_embed": inp["cond_embed"].to(dev), "scale": inp["scale"].to(dev)}
    if inp["keyframes"] is not None:
        y["keyframes"], y["mask"] = inp["keyframes"].to(dev), inp["mask"].to(dev)
    cfg = ClassifierFreeSampleModel(model)
    if case.ddpm_step:
        noise = inp["noise"].to(dev)

        def step():
            res = diffusion.p_sample(cfg, x, t, clip_denoised=False, model_kwargs={"y": y}, noise=noise)
            return {k: res[k].squeeze(2).permute(0, 2, 1).cpu() for k in ("sample", "pred_xstart")}
        return step
    if case.guided:
        return lambda: {"out": cfg(x, t, y).cpu()}
    return lambda: {"out": model(x, t, y).cpu()}


def run_case(models, case, precision, dev):
    """The case's outputs, run once per (case, precision): pick log, counters, finiteness and repeatability are asserted on that run."""
    key = (case.name, precision)
    if key in models["outputs"]:
        return models["outputs"][key]
    model, diffusion = get_model(models, case, precision, dev)
    with switches(case, case.tail16):
        step = make_step(case, model, diffusion, dev)
        before = {k: read_int(model, k, C.c_int64) for k in COUNTERS}
        out = step()
        got = read_picks(model)
        added = {k: read_int(model, k, C.c_int64) - before[k] for k in COUNTERS}
        nw, family = read_int(model, "chain_nw", C.c_int32), read_int(model, "chain_family", C.c_int32)
        again = step()
    model.check_finite()
    assert model.precision == precision, (case.name, model.precision)
    if R.takes_chain_path(case) and precision != "fp32":
        want = R.expected(case)
        assert len(got) == len(want["picks"]), (case.name, describe(got), describe(want["picks"]))
        for i, (g, w) in enumerate(zip(got, want["picks"])):
            assert g == w, (case.name, f"launch {i}", dict(zip(R.FIELDS, g)), dict(zip(R.FIELDS, w)))
        assert [g[:6] for g in got] == list(case.hits), (case.name, describe(got))
        assert nw == want["nw"] and family == want["family"], (case.name, nw, family, want["nw"], want["family"])
        assert added == R.counters(want["picks"]) == R.counters(got), (case.name, added, R.counters(want["picks"]))
    else:
        assert got == [] and not any(added.values()), (case.name, describe(got), added)
    for k, v in out.items():
        assert torch.isfinite(v).all(), (case.name, k)
        assert torch.equal(v, again[k]), (case.name, k, "a second call returns other bits")
    models["outputs"][key] = out
    return out


def where(case, samples, b, f):
    """The rows of the 2B-sequence pass that hold frame f of sample b, with the panel and 16-row tile of each for every panel height of the case."""
    b = b if samples is None else samples[b]
    rows = {"conditional": b * case.T + f}
    if case.guided:
        rows["unconditional"] = (case.B + b) * case.T + f
    heights = sorted({h[2] for h in case.hits}) or [2]
    mixed = any(h[5] == R.MIX for h in case.hits)
    return {"sample": b, **{half: {"row": r, "tile16": r // 16, **{f"panel{16 * mt}": r // (16 * mt) for mt in heights}}
                            for half, r in rows.items()}, **({"mixed_heights": "64-row panels first"} if mixed else {})}


def check_elements(case, precision, out, gate_of, label=None):
    samples = FP.smix_samples(case) if case.B == R.SMIX[0] else None
    want = FP.reference(case, samples)
    failures = []
    for name, ref in want.items():
        got = out[name] if samples is None else out[name][samples]
        mx, rm = FP.statistic(got, ref)
        gate_max, gate_rms, env = gate_of(name)
        record(f"forward_paths/{FP.mode_of(precision, case.tail16)}/{label or case.name}" + ("" if name == "out" else "/" + name),
               max_e=mx, rms_e=rm, max_ratio=mx / env[0], rms_ratio=rm / env[1], envelope_max=env[0], envelope_rms=env[1])
        if not (mx <= gate_max and rm <= gate_rms):
            b, f, c, e = FP.worst_element(got, ref)
            failures.append(dict(case=case.name, precision=precision, output=name, max_e=mx, gate_max=gate_max, rms_e=rm, gate_rms=gate_rms,
                                 frame=f, channel=c, e=e, got=float(got[b, f, c]), want=float(ref[b, f, c]), **where(case, samples, b, f),
                                 launches=describe([h + (0,) * 4 for h in case.hits])))
    if failures:                                   # (a string: pytest prints it whole, the repr of a list it would cut short)
        pytest.fail("\n".join(", ".join(f"{k}={v}" for k, v in f.items()) for f in failures))


def gate_16bit(case, precision):
    def gate(name):
        env = FP.envelope(case, FP.mode_of(precision, case.tail16), name)
        return FP.MARGIN * env[0], FP.MARGIN * env[1], env
    return gate


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", [c.name for c in R.SHALLOW_CASES])
def test_chain_instances_per_element(dev, models, name, precision):
    case = R.SHALLOW_BY_NAME[name]
    check_elements(case, precision, run_case(models, case, precision, dev), gate_16bit(case, precision))


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", [c.name for c in OTHER_CASES])
def test_small_and_per_op_paths_per_element(dev, models, name, precision):
    case = OTHER_BY_NAME[name]
    assert not R.takes_chain_path(case)
    check_elements(case, precision, run_case(models, case, precision, dev), gate_16bit(case, precision))


@pytest.mark.parametrize("name", ["face_S88_small", "pose_S88_per_op"])
def test_fp32_mode_per_element(dev, models, name):
    """precision="fp32": the project's 1e-3 bar on every element (the measured value is recorded: 1e-6 .. 1e-5 is what exact fp32 MFMA gives)."""
    case = OTHER_BY_NAME[name]
    out = run_case(models, case, "fp32", dev)
    check_elements(case, "fp32", out, lambda _: (FP.FP32_GATE, FP.FP32_GATE, (FP.FP32_GATE, FP.FP32_GATE)), label=case.name.rsplit("_", 1)[0] + "_fp32")


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("a,b", BIT_PAIRS)
def test_bits_where_the_project_claims_them(dev, models, a, b, precision):
    out_a, out_b = (run_case(models, case_of(n), precision, dev) for n in (a, b))
    for k in out_a:
        same = out_a[k] == out_b[k]
        if not bool(same.all()):
            bb, f, c = (int(v) for v in torch.unravel_index((~same).int().argmax(), same.shape))
            raise AssertionError((a, b, precision, k, f"{int((~same).sum())} elements differ, the first at", where(case_of(a), None, bb, f), "channel", c))
