"""Every attention kernel instance against float64, element by element (csrc/kernels_attn.h attn_kernel / attn_ksplit_kernel,
kernels_attn3.h attn3_kernel, through launch_attn of csrc/a2p_lib.hip and the test-only entry point
a2p_attention_ex, which puts every field of the kernels' parameter block in the caller's hands).

Per case (tests/attention_restatement.py) and instance:
  1. the dispatcher's decision (attn_pick, reported by the entry point) equals the restated rule;
  2. every element of O outside the exact write set (rows >= Tq, the gaps of ldo > d and between sequences, 64 guard rows on both
     sides) is bit-identical to the sentinel the image was filled with;
  3. every written element is finite, is not the sentinel and lies within a bound DERIVED from unit roundoffs -- not measured;
  4. a second launch returns the same bits;
  5. the logit maximum the launch reports is the float64 maximum over the VALID keys, to the derived logit bound: K pad rows (NaN
     bit patterns in half of the cases, +-12 -- a 6x spike -- in the other half) must not leak into it.
Instances reached: attn_kernel<float, 32 | 64>, attn_kernel<h16_t, 32 | 64>, attn_ksplit_kernel<32 | 64, 4 | 8, 1>,
attn3_kernel<32 | 64>, the 16-bit ones in the IEEE-half and the bfloat16 build.  Deliberately not reached: attn_kernel<float, 128>, which exists only on
the audio front end's own context (a2p_ctx_create refuses head_dim 128; tests/test_frontend_hip.py covers it through the lip
regressor).  The keyframe attention fused into the chain kernel is not an AttnP kernel."""
import ctypes as C
import math
import os

import pytest
import torch

import attention_restatement as R
from audio2photoreal_amd import _lib
from conftest import record

pytestmark = pytest.mark.gpu

# The relative error of the hardware exp2 (v_exp_f32) is the one number that cannot be derived.  It enters the bound like a logit
# perturbation (attention_restatement.bound, exp2_rel); every run measures it as the excess over the derived terms, expressed as the
# exp2 error that would explain it (record "attention_family/exp2_dev/<mode>"), and the gate allows twice the constant.  NOT YET
# MEASURED ON HARDWARE: 0.0, i.e. no allowance at all.  Whoever records a non-zero deviation writes it here and nowhere else.
EXP2_DEV_MEASURED = 0.0
EXP2_GATE = 2.0 * EXP2_DEV_MEASURED

SENT_BITS = torch.tensor([R.SENTINEL], dtype=torch.float32).view(torch.int32).item()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


_CTX = {}


def ctx_for(mode, H):
    """A bare context of the mode with d = 256 and H heads (no weights: the entry point uses its precision, head geometry, scratch
    allocator and logit-maximum slot only)."""
    if (mode, H) not in _CTX:
        lib = _lib.load(mode == "fp16")
        cfg = _lib.A2PConfig(data_format=_lib.FACE, nfeats=104, latent_dim=R.D_MODEL, ff_size=64, num_layers=1, num_heads=H, cond_feature_dim=64,
                             max_frames=16, emb_len=16, keyframe_dim=104, keyframe_step=30,
                             precision=_lib.PREC_F32 if mode == "fp32" else _lib.PREC_BF16, max_batch=1, reserved=0)
        ctx = C.c_void_p()
        _lib.check(lib.a2p_ctx_create(C.byref(cfg), C.byref(ctx)), "a2p_ctx_create")
        _CTX[mode, H] = (lib, ctx)
    return _CTX[mode, H]


@pytest.fixture(scope="module", autouse=True)
def _destroy_contexts():
    saved = {n: os.environ.get(n) for n in R.ENV_NAMES}
    yield
    for n, v in saved.items():
        os.environ.pop(n, None)
        if v is not None:
            os.environ[n] = v
    for lib, ctx in _CTX.values():
        lib.a2p_ctx_destroy(ctx)
    _CTX.clear()


def set_instance(lib, ctx, inst):
    for n in R.ENV_NAMES:
        os.environ.pop(n, None)
    os.environ.update(R.INSTANCES[inst][0])
    _lib.check(lib.a2p_reload_env(ctx), "a2p_reload_env")


def case_struct(case, lay, dimg, slots, ran):
    q = _lib.A2PAttentionCase(qbuf=dimg["q"].data_ptr(), kbuf=None if lay.k_in_q else dimg["k"].data_ptr(), vt=dimg["vt"].data_ptr(),
                              out=dimg["out"].data_ptr(), ran_host=ran, q_elems=lay.q_elems, k_elems=lay.k_elems, vt_elems=lay.vt_elems,
                              out_elems=lay.out_elems, tail_elems=lay.tail_elems, q_off=lay.q_off, k_off=lay.k_off, vt_off=lay.vt_off, out_off=lay.out_off,
                              q_seq_stride=lay.q_seq_stride, ldq=lay.ldq, k_slot_stride=lay.k_slot_stride, ldk=lay.ldk, vt_slot_stride=lay.vt_slot_stride,
                              ldvt=lay.ldvt, o_seq_stride=lay.o_seq_stride, ldo=lay.ldo, tail_sample_stride=lay.tail_sample_stride,
                              tail_row_stride=lay.tail_row_stride, nseq=case.nseq, Tq=case.Tq, S_main=case.S_main, S_tail=case.S_tail, nslots=case.nslots,
                              slot_rule=case.slot_rule, slot_b=case.slot_b, tail_mod=case.tail_mod, kv_stream=case.kv_stream, ksplit=case.ksplit,
                              nseq_rule=case.nseq_rule)
    if case.S_tail:
        q.ktail, q.vtail = dimg["ktail"].data_ptr(), dimg["vtail"].data_ptr()
    if slots is not None:
        q.kv_slot_host = slots
    return q


_RUNS = {}   # (case, mode, instance) -> output image, for the kv_stream comparison


def check_case(dev, mode, case):
    """Failures of one case over all of its instances as strings (empty: passed); records the worst ratios."""
    fails, stats = [], {}
    lib, ctx = ctx_for(mode, case.H)
    ops, lay = R.make_operands(case, mode), R.layout(case, mode)
    r = R.restate(case, ops)
    img = R.make_images(case, ops, lay)
    dimg = {k: v.to(dev) for k, v in img.items() if k != "k" or not lay.k_in_q}
    table = case.slot_table()
    slots = (C.c_int32 * case.nseq)(*table) if table else None
    for inst in R.instances_of(case, mode):
        tag = f"{case.name} as {inst}"
        set_instance(lib, ctx, inst)
        want = R.pick(mode, case, R.INSTANCES[inst][0])
        images, logit = [], None
        for rep in range(2):
            dimg["out"].fill_(R.SENTINEL)
            ran = (C.c_int32 * 8)()
            _lib.check(lib.a2p_attention_ex(ctx, C.byref(case_struct(case, lay, dimg, slots, ran)), _lib.current_stream()), f"a2p_attention_ex({tag})")
            if rep == 0:
                lm = C.c_float()
                _lib.check(lib.a2p_attention_logit_max(ctx, C.byref(lm), _lib.current_stream()), "a2p_attention_logit_max")
                logit = lm.value
            torch.cuda.synchronize()
            images.append(dimg["out"].cpu())
        out = images[0]
        _RUNS[case.name, mode, inst] = out
        if tuple(ran) != want:                                                                        # 1
            fails.append(f"{tag}: dispatcher chose {tuple(ran)}, the rule says {want}")
        kernel = want[0]
        bad = ((out.view(torch.int32) != SENT_BITS) & ~lay.written).nonzero().flatten()               # 2
        if bad.numel():
            i = int(bad[0]) - lay.out_off
            fails.append(f"{tag}: {bad.numel()} elements outside the write set changed; first at O element {i} (row {i // lay.ldo}, column {i % lay.ldo}) "
                         f"= {float(out[int(bad[0])])!r}")
        got = out[lay.out_index].double()                                                             # 3
        err = (got - r["ref"]).abs()
        derived = R.bound(case, mode, kernel, r)
        ratio = torch.nan_to_num(err / R.bound(case, mode, kernel, r, exp2_rel=EXP2_GATE).clamp(min=1e-300), nan=math.inf)
        worst = float(ratio.max())
        # the excess over the derived terms as the relative exp2 error that would explain it: excess = expm1(2 e) Dv (1 + u)
        excess = ((err - derived).clamp(min=0) / (r["mag_dv"] * (1 + R.U_OUT[mode])).clamp(min=1e-300))
        exp2_dev = float(0.5 * torch.log1p(torch.nan_to_num(excess, nan=0.0, posinf=0.0)).max())
        n_sent = int((out[lay.out_index].view(torch.int32) == SENT_BITS).sum())
        if not torch.isfinite(got).all() or n_sent or worst > 1.0:
            seq, t, col = (int(v) for v in torch.unravel_index(ratio.argmax(), ratio.shape))
            fails.append(f"{tag}: error / bound = {worst:.3g} at (seq {seq}, row {t}, head {col // case.dh}, column {col % case.dh}): got {float(got[seq, t, col])!r}, "
                         f"reference {float(r['ref'][seq, t, col])!r}, bound {float(derived[seq, t, col]):.3g}; {int((ratio > 1).sum())} elements over, "
                         f"{int((~torch.isfinite(got)).sum())} not finite, {n_sent} still the sentinel")
        if not torch.equal(images[1].view(torch.int32), out.view(torch.int32)):                       # 4
            fails.append(f"{tag}: the second launch differs in {int((images[1].view(torch.int32) != out.view(torch.int32)).sum())} elements")
        lb = R.logit_max_bound(case, mode, kernel, r)                                                 # 5
        if not abs(logit - r["logit_max"]) <= lb:
            fails.append(f"{tag}: reported logit maximum {logit!r}, float64 maximum over valid keys {r['logit_max']!r}, bound {lb:.3g}")
        key = R.KERNEL_NAMES[kernel] + (f"<{want[2]},{want[3]},{want[4]}>" if kernel == R.K_KSPLIT else f"<{want[1]}-bit,{want[2]}>")
        s = stats.setdefault(key, dict(ratio=0.0, exp2_dev=0.0, logit_ratio=0.0))
        s["ratio"], s["exp2_dev"] = max(s["ratio"], min(worst, 1e30)), max(s["exp2_dev"], exp2_dev)
        s["logit_ratio"] = max(s["logit_ratio"], min(abs(logit - r["logit_max"]) / lb, 1e30) if math.isfinite(logit) else 1e30)
    return fails, stats


def _group(c):
    return c.name.split("/", 1)[0]


GROUPS = [(m, g) for m in R.MODES for g in sorted({_group(c) for c in R.CASES})]
_WORST = {}


@pytest.mark.parametrize("mode,group", GROUPS)
def test_attention_cases(dev, mode, group):
    cases = [c for c in R.CASES if _group(c) == group and R.instances_of(c, mode)]
    assert cases
    fails = []
    for c in cases:
        f, stats = check_case(dev, mode, c)
        fails += f
        for key, s in stats.items():
            w = _WORST.setdefault((mode, key), dict(ratio=0.0, exp2_dev=0.0, logit_ratio=0.0))
            for k in w:
                w[k] = max(w[k], s[k])
    for (m, key), w in _WORST.items():
        if m == mode:
            record(f"attention_family/{mode}/{key}", **w)
    record(f"attention_family/exp2_dev/{mode}", exp2_dev=max([w["exp2_dev"] for (m, _), w in _WORST.items() if m == mode] or [0.0]), gate=EXP2_GATE)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("mode", R.MODES)
def test_kv_stream_changes_no_bit(dev, mode):
    """The non-temporal policy of the K/V tile loads (kv_stream, slots other than 0) is a cache hint: same bits."""
    for plain, stream in (("slots/rule3", "slots/rule3_stream"), ("slots/table", "slots/table_stream")):
        for inst in R.instances_of(R.BY_NAME[plain], mode):
            for name in (plain, stream):
                if (name, mode, inst) not in _RUNS:
                    check_case(dev, mode, R.BY_NAME[name])
            a, b = _RUNS[plain, mode, inst], _RUNS[stream, mode, inst]
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f"{plain} as {inst}: kv_stream = 1 differs"


@pytest.mark.parametrize("mode", R.MODES)
def test_bad_cases_are_refused_before_any_launch(dev, mode):
    case = R.BY_NAME["slots/rule3"]
    lib, ctx = ctx_for(mode, case.H)
    set_instance(lib, ctx, "attn")
    ops, lay = R.make_operands(case, mode), R.layout(case, mode)
    dimg = {k: v.to(dev) for k, v in R.make_images(case, ops, lay).items()}
    base = case_struct(case, lay, dimg, None, None)

    def call(**over):
        q = _lib.A2PAttentionCase.from_buffer_copy(base)
        for k, v in over.items():
            setattr(q, k, v)
        return lib.a2p_attention_ex(ctx, C.byref(q), _lib.current_stream())

    assert call() == 0
    dimg["out"].fill_(R.SENTINEL)
    Sp, d = case.Sp, R.D_MODEL
    for over in (dict(nseq=0), dict(Tq=0), dict(S_main=0), dict(out_elems=lay.out_elems - 2 * lay.out_off), dict(q_elems=lay.q_elems - 32), dict(k_elems=lay.k_elems - 65 * lay.ldk),
                 dict(vt_elems=lay.vt_elems - 8 * lay.ldvt - 72), dict(ldvt=Sp - 8), dict(ldvt=lay.ldvt + 4), dict(ldo=d - 8), dict(ldq=d - 8), dict(ldk=d - 8),
                 dict(o_seq_stride=lay.ldo), dict(k_slot_stride=lay.ldk * 8), dict(vt_slot_stride=lay.ldvt * 8), dict(nslots=case.nslots - 1), dict(slot_rule=1),
                 dict(slot_rule=4), dict(tail_mod=0), dict(tail_elems=lay.tail_elems - 24), dict(tail_row_stride=d - 4), dict(tail_sample_stride=lay.tail_row_stride),
                 dict(ktail=None), dict(S_tail=3, ksplit=1), dict(S_main=case.S_main + 128), dict(out_off=lay.out_off + 4), dict(q_off=-8), dict(kv_stream=2),
                 dict(qbuf=dimg["q"].data_ptr() + 4)):
        assert call(**over) == -1, over
    del _lib._failed[:]
    torch.cuda.synchronize()
    assert bool((dimg["out"].cpu().view(torch.int32) == SENT_BITS).all()), "a refused case must not launch"
