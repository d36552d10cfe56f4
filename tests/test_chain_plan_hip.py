"""The chain dispatch of csrc/a2p_lib_run.h (forward_plan, chain_pick, launch_chain) against tests/chain_plan_restatement.py: for
every case the pick log of the forward (a2p_debug_read "chain_picks", recorded by launch_chain from the pick it launched) equals the
restated rule record for record, and the names that were there before the log -- chain_nw, chain_family, the *_launches counters
and the launch count of each KERNEL_CHAIN_* timing class -- agree with it.  Families are forced (A2P_CHAIN_V), so no case depends on
the in-situ calibration; `test_unforced_family_alternates_then_settles` covers the calibration's schedule alone.

Each case is one forward on the synthetic face or body model, plus one per timing class (the timer selects one class at a time)."""
import contextlib
import ctypes as C
import os

import pytest
import torch

import chain_plan_restatement as R
from audio2photoreal_amd import _lib
from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel
from audio2photoreal_amd.model_util import create_model_and_diffusion, default_args, load_model
from audio2photoreal_amd.spec import face_spec, pose_spec
from audio2photoreal_amd.synthetic import synthetic_inputs, synthetic_state_dict

pytestmark = pytest.mark.gpu
SEED = 10
PRECISIONS = ("fp16", "bf16")
CLASSES = {"PRE": _lib.KERNEL_CHAIN_PRE, "MID": _lib.KERNEL_CHAIN_MID, "POST": _lib.KERNEL_CHAIN_POST, "MIDPOST": _lib.KERNEL_CHAIN_MIDPOST}
COUNTERS = ("chain4_launches", "chain_in_launches", "final_fused_launches", "fused_tail_launches")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def models():
    """Contexts shared by the cases of one (model, precision, batch capacity, A2P_TAIL16) -- the switches of a case are re-read per call."""
    cache = {}
    yield cache
    for model, _ in cache.values():
        model.release()


@contextlib.contextmanager
def switches(case, tail16=False):
    """The case's switches in the environment, every other switch of the dispatch unset; restored on exit."""
    names = R.SWITCHES + ("A2P_TAIL16",)
    saved = {k: os.environ.get(k) for k in names}
    try:
        for k in names:
            os.environ.pop(k, None)
        os.environ.update(case.switches)
        if tail16:
            os.environ["A2P_TAIL16"] = "1"
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def get_model(models, case, precision, dev):
    cap = 1 if case.B == 1 else 26
    key = (case.fmt, precision, cap, case.tail16)
    if key not in models:
        spec = face_spec() if case.fmt == "face" else pose_spec()
        with switches(case, case.tail16):          # A2P_TAIL16 is read when the context is created and the weights are finalized
            model, diffusion = create_model_and_diffusion(default_args(case.fmt), "test", precision=precision, max_batch=cap)
            load_model(model, synthetic_state_dict(spec, SEED))
            model = model.to(dev).eval()
            model._ensure_ctx(dev, cap)
            model._ensure_weights(model._lib(), dev)
        models[key] = (model, diffusion)
    return models[key]


def make_step(case, model, diffusion, dev):
    """The case's forward (or guided DDPM step) as a closure over seeded inputs: () -> {name: tensor}."""
    spec = face_spec() if case.fmt == "face" else pose_spec()
    inp = synthetic_inputs(spec, case.B, case.T, SEED)
    x = inp["x_T"].to(dev)
    y = {"cond_embed": inp["cond_embed"].to(dev), "scale": torch.full((case.B,), 10.0 if case.fmt == "face" else 2.0, device=dev)}
    if spec.is_pose:
        y["keyframes"], y["mask"] = inp["keyframes"].to(dev), inp["mask"].to(dev)
    t = torch.tensor(([901, 417, 33] * 9)[:case.B], device=dev)
    cfg = ClassifierFreeSampleModel(model)
    if case.ddpm_step:
        noise = torch.randn(inp["x_T"].shape, generator=torch.Generator().manual_seed(SEED + 1)).to(dev)
        return lambda: dict(diffusion.p_sample(cfg, x, t, clip_denoised=False, model_kwargs={"y": y}, noise=noise))
    if case.guided:
        return lambda: {"out": cfg(x, t, y)}
    return lambda: {"out": model(x, t, y)}


def read_int(model, name, ctype):
    v = ctype(0)
    _lib.check(model._lib().a2p_debug_read(model._ctx, name.encode(), C.byref(v), C.sizeof(v)), "a2p_debug_read")
    return int(v.value)


def read_picks(model):
    """a2p_debug_read "chain_picks": [launches, ints per record] then the records, in launch order."""
    buf = (C.c_int32 * (2 + R.MAX_PICKS * len(R.FIELDS)))()
    _lib.check(model._lib().a2p_debug_read(model._ctx, b"chain_picks", buf, C.sizeof(buf)), "a2p_debug_read")
    n, width = buf[0], buf[1]
    assert width == len(R.FIELDS) and 0 <= n <= R.MAX_PICKS, (n, width)
    return [tuple(buf[2 + i * width: 2 + (i + 1) * width]) for i in range(n)]


def class_launches(model, step, kind):
    lib = model._lib()
    _lib.check(lib.a2p_kernel_timing(model._ctx, kind, 1), "a2p_kernel_timing")
    step()
    ms, n = C.c_double(0), C.c_int64(0)
    _lib.check(lib.a2p_kernel_time_ms(model._ctx, C.byref(ms), C.byref(n)), "a2p_kernel_time_ms")
    _lib.check(lib.a2p_kernel_timing(model._ctx, kind, 0), "a2p_kernel_timing")
    return int(n.value)


def describe(picks):
    return [dict(zip(R.FIELDS, p)) for p in picks]


def check_case(case, precision, dev, models, picks_of=read_picks):
    """Run the case once and compare everything the library reports about the launch with the restated rule; returns the outputs."""
    model, diffusion = get_model(models, case, precision, dev)
    want = R.expected(case)
    with switches(case, case.tail16):
        step = make_step(case, model, diffusion, dev)
        before = {k: read_int(model, k, C.c_int64) for k in COUNTERS}
        out = {k: v.cpu() for k, v in step().items()}
        got = picks_of(model)
        added = {k: read_int(model, k, C.c_int64) - before[k] for k in COUNTERS}
        nw, family = read_int(model, "chain_nw", C.c_int32), read_int(model, "chain_family", C.c_int32)
        classes = {name: class_launches(model, step, kind) for name, kind in CLASSES.items()}
    model.check_finite()
    assert all(torch.isfinite(v).all() for v in out.values()), case.name
    assert len(got) == len(want["picks"]), (case.name, describe(got), describe(want["picks"]))
    for i, (g, w) in enumerate(zip(got, want["picks"])):
        assert g == w, (case.name, f"launch {i}", dict(zip(R.FIELDS, g)), dict(zip(R.FIELDS, w)))
    # the long-standing names against the restated rule, and therefore against the log
    assert nw == want["nw"] and family == want["family"], (case.name, nw, family, want["nw"], want["family"])
    assert added == R.counters(want["picks"]) == R.counters(got), (case.name, added, R.counters(want["picks"]))
    assert classes == R.class_counts(want["picks"]) == R.class_counts(got), (case.name, classes, R.class_counts(want["picks"]))
    assert all(p[R.FIELDS.index("nw")] == nw for p in got), (case.name, nw)
    return out


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_pick_log_matches_the_restated_rule(dev, models, name, precision):
    check_case(R.BY_NAME[name], precision, dev, models)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_unforced_family_alternates_then_settles(dev, models, precision):
    """A2P_CHAIN_V unset: forwards 0-9 of a size alternate (tall, tall) and (tall MID, generation-1 POST); from forward 10 on the
    size keeps one of the two.  Which one is this machine's measurement; the log follows the family the library reports."""
    case = R.Case("unforced", "face", 1, 88, True, (("A2P_CHAIN_ROWS", "1"),))      # a size no other case calibrates
    model, diffusion = get_model(models, case, precision, dev)
    seen = []
    with switches(case):
        step = make_step(case, model, diffusion, dev)
        for i in range(13):
            step()
            family = read_int(model, "chain_family", C.c_int32)
            seen.append(family)
            assert read_picks(model) == R.expected(case, family=(family // 10, family % 10))["picks"], (i, family)
    assert seen[:10] == [44, 41] * 5, seen
    assert seen[10] in (44, 41) and seen[10:] == [seen[10]] * 3, seen
