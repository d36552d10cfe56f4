"""tests/attention_restatement.py checked against itself and against torch, without a GPU: the float64 restatement, the dispatcher's
rule, the derived bound (a plain emulation of every kernel family stays under it on every case; every planted fault leaves it by
10x or more), the write-set bookkeeping and the header / ctypes mirror of a2p_attention_ex."""
import ctypes as C
import math
import os
import re

import pytest
import torch

import attention_restatement as R
from audio2photoreal_amd import _lib
from conftest import ROOT, record

_REF = {}


def reference(case, mode):
    """(operands, restatement) of a case, computed once and shared."""
    if (case.name, mode) not in _REF:
        ops = R.make_operands(case, mode)
        _REF[case.name, mode] = (ops, R.restate(case, ops))
    return _REF[case.name, mode]


def ratio_of(out, r, bnd):
    """Worst |out - ref| / bound; a non-finite output is infinitely far out."""
    return float(torch.nan_to_num((out.double() - r["ref"]).abs() / bnd.clamp(min=1e-300), nan=math.inf).max())


# ----------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", ["keys/s65", "queries/t33", "grid/noremap", "data/spike"])
def test_restatement_is_scaled_dot_product_attention(name):
    case = R.BY_NAME[name]
    assert case.slots == "seq" and not case.S_tail
    ops, r = reference(case, "fp32")
    heads = lambda t: t.double().view(t.shape[0], t.shape[1], case.H, case.dh).transpose(1, 2)
    want = torch.nn.functional.scaled_dot_product_attention(heads(ops["Q"]), heads(ops["K"]), heads(ops["V"]))
    want = want.transpose(1, 2).reshape(case.nseq, case.Tq, R.D_MODEL)
    assert (r["ref"] - want).abs().max() < 1e-12
    # the magnitudes: sum_j w_j |v_j - out| <= sum_j w_j |v_j| + |out|, and |out| <= sum_j w_j |v_j|
    assert (r["ref"].abs() <= r["mag_v"] * (1 + 1e-12)).all() and (r["mag_dv"] <= (r["mag_v"] + r["ref"].abs()) * (1 + 1e-12)).all()


@pytest.mark.parametrize("name", ["slots/table", "slots/rule3", "tail/m63t2", "tail/m64t1", "layout/gaps"])
def test_restatement_with_slots_and_tails_is_gather_then_concatenate(name):
    case = R.BY_NAME[name]
    ops, r = reference(case, "bf16")
    table = case.slot_table()
    for seq in range(case.nseq):
        slot = {0: table[seq] if table else seq, 1: 1 + seq, 2: 0, 3: 1 + seq if seq < case.nseq // 2 else 0}[case.slot_rule]
        k, v = ops["K"][slot].double(), ops["V"][slot].double()
        if case.S_tail:
            k = torch.cat([k, ops["ktail"][seq % case.tail_mod].double()])
            v = torch.cat([v, ops["vtail"][seq % case.tail_mod].double()])
        assert k.shape[0] == case.S
        for h in range(case.H):
            cols = slice(h * case.dh, (h + 1) * case.dh)
            s = ops["Q"][seq][:, cols].double() @ k[:, cols].T / math.sqrt(case.dh)
            want = torch.softmax(s, -1) @ v[:, cols]
            assert (r["ref"][seq][:, cols] - want).abs().max() < 1e-12
    # the float64 maximum is over valid keys of the sequences' own slots
    assert r["logit_max"] == pytest.approx(max(float((ops["Q"][q][:, h * case.dh:(h + 1) * case.dh].double()
                                                       @ R.gather(case, ops, q)[0][:, h * case.dh:(h + 1) * case.dh].T).max()) / math.sqrt(case.dh)
                                               for q in range(case.nseq) for h in range(case.H)), rel=1e-12)


def test_operands_are_exact_in_the_mode_and_distinct_per_slot_head_and_sample():
    case = R.BY_NAME["slots/rule3"]
    for mode in R.B16:
        ops = R.make_operands(case, mode)
        for t in ops.values():
            assert torch.equal(R.round_to(t, mode), t)
    ops = R.make_operands(case, "fp32")
    means = ops["V"].view(case.nslots, case.S_main, case.H, case.dh).mean((1, 3))           # [slot, head]
    design = (torch.arange(case.nslots).view(-1, 1) + 1.0) + 0.1 * torch.arange(case.H)      # distinct by 0.1 or more by construction
    flat = sorted(design.flatten().tolist())
    assert min(b - a for a, b in zip(flat, flat[1:])) > 0.09 and (means - design).abs().max() < 0.1, "every (slot, head) has its own mean of V"
    tmeans = ops["vtail"].mean((1, 2))
    assert (tmeans[0] - tmeans[1]).abs() > 1.0 and tmeans.max() < means.min() - 1.0


def test_every_case_is_inside_the_documented_16_bit_envelope():
    """INTEGRATION.md "validity envelope": the 16-bit modes are validated up to a largest scaled logit of A2P_LOGIT_ENVELOPE_16BIT; a
    case outside it proves nothing about a kernel."""
    header = open(os.path.join(ROOT, "include", "a2p_hip.h")).read()
    assert float(re.search(r"#define A2P_LOGIT_ENVELOPE_16BIT ([0-9.]+)f", header).group(1)) == R.ENVELOPE_16BIT
    worst = {}
    for mode in R.MODES:
        for case in R.CASES:
            worst[mode] = max(worst.get(mode, -math.inf), reference(case, mode)[1]["logit_max"])
            assert reference(case, mode)[1]["logit_max"] <= R.ENVELOPE_16BIT, case.name
    record("attention_family/largest_logit", **worst)
    assert max(worst.values()) > 0.5 * R.ENVELOPE_16BIT, "the spikes should reach well into the envelope"


# ----------------------------------------------------------------------------- the dispatcher's rule
def _case(**k):
    f = dict(name="x", H=4, nseq=1, Tq=600, S_main=600)
    f.update(k)
    return R.Case(**f)


def test_pick_restates_the_documented_rule():
    A, KS, A3 = R.K_ATTN, R.K_KSPLIT, R.K_ATTN3
    kern = lambda mode, env=None, **k: R.pick(mode, _case(**k), env)[0]
    # fp32 never leaves attn_kernel, whatever is forced
    for env in ({}, {"A2P_ATTN3": "2"}, {"A2P_ATTN_KSPLIT": "1"}):
        assert R.pick("fp32", _case(nseq=16, ksplit=1), env)[:5] == (A, 32, 64, 4, 2)
    # attn3 by size: head_dim 64, >= 160 queries, more than 256 attn_kernel workgroups of the RULE's batch, and at most 256 of its own
    assert kern("bf16", nseq=16) == A3                        # 5 * 4 * 16 = 320 > 256; 2 * 4 * 16 = 128 <= 256
    assert kern("bf16", nseq=12) == A                         # 240 attn_kernel workgroups: one round
    assert kern("bf16", nseq=2, nseq_rule=16) == A3 and kern("bf16", nseq=16, nseq_rule=2) == A   # the unsharded batch decides
    assert kern("bf16", nseq=40, Tq=159, S_main=65) == A and kern("bf16", nseq=40, Tq=160, S_main=65) == A3
    assert kern("bf16", nseq=64) == A                         # 512 attn3 workgroups, 600 keys: several rounds of short key ranges
    assert kern("bf16", nseq=64, S_main=1022, S_tail=2) == A3 and kern("bf16", nseq=64, S_main=1021, S_tail=2) == A   # the key count rule
    assert kern("bf16", H=8, nseq=8) == A and kern("bf16", H=8, nseq=8, S_main=1024) == A3       # head_dim 32: long key ranges only
    assert kern("bf16", {"A2P_ATTN3": "0"}, nseq=16) == A and kern("fp16", {"A2P_ATTN3": "2"}, Tq=1, S_main=1) == A3
    # geometry: query blocks of 128 (attn_kernel), 320 (attn3), 16 (key split); the remap needs pairs % 8 == 0
    assert R.pick("bf16", _case(nseq=2, Tq=321), {"A2P_ATTN3": "0"}) == (A, 16, 64, 4, 2, 3, 24, 1)
    assert R.pick("bf16", _case(nseq=3, Tq=321), {"A2P_ATTN3": "2"}) == (A3, 16, 64, 4, 5, 2, 24, 0)
    # key split: on request or forced; 8 waves above 8 tiles unless the switch says otherwise; never remapped; at most two tail rows
    assert R.pick("bf16", _case(nseq=2, Tq=33, S_main=510, S_tail=2, ksplit=1)) == (KS, 16, 64, 4, 1, 3, 24, 0)
    assert R.pick("bf16", _case(nseq=2, Tq=33, S_main=511, S_tail=2, ksplit=1)) == (KS, 16, 64, 8, 1, 3, 24, 0)
    assert R.pick("bf16", _case(nseq=2, Tq=33, S_main=65), {"A2P_ATTN_KSPLIT": "1", "A2P_KSPLIT_NW": "8"}) == (KS, 16, 64, 8, 1, 3, 24, 0)
    assert R.pick("bf16", _case(nseq=2, Tq=33, S_main=900), {"A2P_ATTN_KSPLIT": "1", "A2P_KSPLIT_NW": "4"})[3] == 4
    assert kern("bf16", Tq=33, S_main=65, S_tail=3, ksplit=1) == A and kern("bf16", {"A2P_NO_KSPLIT": "1"}, Tq=33, S_main=65, ksplit=1) == A


def test_the_case_list_reaches_every_instance():
    """attn_kernel<float | h16, 32 | 64>, the four key-split instances, attn3 at 64 and 32 -- each in the modes that have it."""
    for mode in R.MODES:
        seen = {R.pick(mode, c, R.INSTANCES[i][0])[:5] for c in R.CASES for i in R.instances_of(c, mode)}
        want = {(R.K_ATTN, 32 if mode == "fp32" else 16, dh, 4, 2) for dh in (32, 64)}
        if mode != "fp32":
            want |= {(R.K_KSPLIT, 16, dh, nw, 1) for dh in (32, 64) for nw in (4, 8)}
            want |= {(R.K_ATTN3, 16, dh, 4, 5) for dh in (32, 64)}
        assert seen == want, seen ^ want
    # ... and the default rule reaches attn3, attn_kernel and the requested key split (4 and 8 waves) with no switch set
    by_rule = {c.name: R.pick("bf16", c)[:4] for c in R.CASES if c.instances == ("default",)}
    assert by_rule == {"rule/attn3_by_size": (R.K_ATTN3, 16, 64, 4), "rule/attn_below_160": (R.K_ATTN, 16, 64, 4),
                       "rule/ksplit_request": (R.K_KSPLIT, 16, 32, 4), "keys/s577_ksplit_request": (R.K_KSPLIT, 16, 64, 8)}


def test_the_case_list_covers_the_edges_the_kernels_have():
    tails = {(c.S_main % 64, c.S_tail, c.S_main < 64) for c in R.CASES if c.S_tail and c.name.startswith("tail/")}
    assert {(r, t) for r, t, _ in tails} == {(r, t) for r in (0, 1, 62, 63) for t in (1, 2)}
    assert {(r, lt) for r, _, lt in tails} >= {(1, True), (62, True), (63, True), (0, False), (1, False), (62, False), (63, False)}
    assert {c.tail_mod for c in R.CASES if c.S_tail} >= {1, 2} and any(c.S_tail and c.tail_mod == c.nseq // 2 > 1 for c in R.CASES)
    assert {c.S for c in R.CASES} >= {1, 5, 63, 64, 65, 127, 128, 129, 190, 513, 577}
    assert {c.Tq for c in R.CASES} >= {1, 15, 16, 17, 33, 127, 128, 129, 321}
    assert {c.slots for c in R.CASES} == {"seq", "table", "rule1", "rule2", "rule3"} and {c.pad for c in R.CASES} == {"nan", "big"}
    assert {c.data for c in R.CASES} == {"plain", "spike", "spike_last", "spike_pad0", "neg"}
    assert max(c.S for c in R.CASES) <= 600, "key counts above 600 only where a rule needs them"
    table = R.BY_NAME["slots/table"].slot_table()
    assert table.count(0) == 2 and sorted(set(table)) == [0, 1, 2] and table != sorted(table)


# ----------------------------------------------------------------------------- the bound
@pytest.mark.parametrize("mode", R.MODES)
def test_an_emulation_of_every_kernel_family_stays_under_the_bound(mode):
    worst, fails = {}, []
    for case in R.CASES:
        ops, r = reference(case, mode)
        for inst in R.instances_of(case, mode):
            k = R.pick(mode, case, R.INSTANCES[inst][0])
            fam = R.FAMILY_OF[k[0]]
            ratio = ratio_of(R.emulate(case, mode, fam, ops, nw=k[3]), r, R.bound(case, mode, k[0], r))
            if ratio > worst.get(fam, (-1.0, ""))[0]:
                worst[fam] = (ratio, case.name)
            if not ratio <= 1.0:
                fails.append(f"{case.name} as {inst}: emulation / bound = {ratio:.3g}")
    for fam, (ratio, name) in worst.items():
        record(f"attention_family/emulation/{mode}/{fam}", ratio=ratio, case=name)
    assert not fails, "\n".join(fails)
    assert set(worst) == ({"online"} if mode == "fp32" else {"online", "ksplit", "lazy"})


# the cases a fault can show on: the fault must exist there (a tail to misplace, a rule-3 table, a second tile, padding of the right kind)
def _shows(fault, case):
    return {"pad_unmasked": case.Sp > case.S and case.pad == "big",
            "v_pad_kept": case.Sp > case.S and case.pad == "nan",
            "tail_row1_at_s_main": case.S_tail == 2,
            "tail_sample_is_seq": case.S_tail > 0 and case.tail_mod > 1 and case.nseq > case.tail_mod,
            "rule3_last_cond_slot0": case.slots == "rule3",
            "q_row_shift": case.Tq >= 2,
            "no_rescale": case.Sp >= 128,
            "head_shift": True}[fault]


@pytest.mark.parametrize("fault", R.FAULTS)
def test_a_planted_fault_leaves_the_bound_by_ten_times(fault):
    """The bound can tell a subtle fault from rounding: planted into the emulation of each family, every fault exceeds it by >= 10x
    on at least one case of the list (in every mode the family exists in)."""
    for mode in R.MODES:
        for fam, kernel, nw in (("online", R.K_ATTN, 4), ("ksplit", R.K_KSPLIT, 4), ("lazy", R.K_ATTN3, 4)):
            if mode == "fp32" and fam != "online":
                continue
            best = (0.0, "")
            for case in R.CASES:
                if not _shows(fault, case) or (fam == "ksplit" and (case.S_tail > 2 or (fault == "no_rescale" and case.Sp < 128))):
                    continue
                ops, r = reference(case, mode)
                ratio = ratio_of(R.emulate(case, mode, fam, ops, fault=fault, nw=nw), r, R.bound(case, mode, kernel, r))
                if ratio > best[0]:
                    best = (ratio, case.name)
                if ratio == math.inf:
                    break
            record(f"attention_family/fault/{fault}/{mode}/{fam}", factor=min(best[0], 1e30), case=best[1])
            assert best[0] >= 10.0, f"{fault} in the {fam} emulation ({mode}): at most {best[0]:.3g}x the bound ({best[1]})"


def test_the_bound_is_made_of_the_documented_terms():
    case = R.BY_NAME["data/spike"]
    _, r = reference(case, "bf16")
    u = R.U_OUT["bf16"]
    b_attn, b_3 = R.bound(case, "bf16", R.K_ATTN, r), R.bound(case, "bf16", R.K_ATTN3, r)
    # 16-bit: the P operand dominates; attn3 pays 2 u Dv for its P and another ~2 u A Dv for its rounded Q instead of u Mv
    assert (b_attn >= u * (r["mag_v"] + r["ref"].abs())).all() and (b_attn <= 1.5 * u * (r["mag_v"] + r["ref"].abs())).all()
    assert (b_3 >= 2 * u * r["mag_dv"] * (1 + r["qk_abs"])).all()
    # fp32: no 16-bit term at all
    _, r32 = reference(case, "fp32")
    want32 = torch.expm1(2 * R.logit_delta(case, "fp32", R.K_ATTN, r32)) * r32["mag_dv"] + 4 * (2 * case.S + 4 * (case.Sp // 64) + 16) * R.U32 * r32["mag_v"]
    assert torch.allclose(R.bound(case, "fp32", R.K_ATTN, r32), want32, rtol=1e-12, atol=0) and (want32 < 0.25 * b_attn).all()
    # the exp2 allowance enters as a logit perturbation
    extra = R.bound(case, "bf16", R.K_ATTN, r, exp2_rel=1e-4) - b_attn
    assert torch.allclose(extra, math.expm1(2e-4) * r["mag_dv"] * (1 + u), rtol=1e-2, atol=0)
    assert R.logit_max_bound(case, "bf16", R.K_ATTN3, r) > u * float(r["qk_abs"].max()) > R.logit_max_bound(case, "bf16", R.K_ATTN, r)


# ----------------------------------------------------------------------------- buffers
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.name)
def test_write_set_and_buffer_bookkeeping(case):
    lay = R.layout(case)
    d = R.D_MODEL
    assert int(lay.written.sum()) == case.nseq * case.Tq * case.H * case.dh == lay.out_index.numel()
    assert lay.out_index.unique().numel() == lay.out_index.numel() and bool(lay.written[lay.out_index.flatten()].all())
    guard = R.GUARD_ROWS * lay.ldo
    assert not lay.written[:guard].any() and not lay.written[-guard:].any() and lay.out_off == guard
    assert int(lay.out_index.max()) < lay.out_elems - guard
    if case.layout == "gaps":
        assert lay.ldo == d + 8 and lay.o_seq_stride > case.Tq * lay.ldo and lay.ldvt == case.Sp + 64
        assert lay.k_slot_stride > case.Sp * lay.ldk and lay.vt_slot_stride > d * lay.ldvt and lay.tail_row_stride > d
    # operands and padding do not collide, and every slot holds whole tiles
    ops = R.make_operands(case, "fp32")
    img = R.make_images(case, ops, lay)
    assert torch.equal(img["q"][lay.q_index], ops["Q"]) and torch.equal(img["k"][lay.k_index], ops["K"]) and torch.equal(img["vt"][lay.vt_index], ops["V"])
    assert lay.k_pad.shape[1] == case.Sp - case.S_main == lay.vt_pad.shape[1]
    if lay.k_pad.numel():
        pad_k, pad_v = img["k"][lay.k_pad], img["vt"][lay.vt_pad]
        if case.pad == "nan":
            assert pad_k.isnan().all() and pad_v.isnan().all()
            assert torch.equal(pad_k.half().float().view(torch.int32), pad_k.view(torch.int32)), "the NaN patterns survive the narrowing"
        else:
            assert (pad_k.abs() == R.PAD_BIG_K).all() and (pad_v.abs() == R.PAD_BIG_V).all() and (pad_k > 0).any() and (pad_k < 0).any()
            assert torch.equal(pad_v.half().float(), pad_v) and torch.equal(pad_v.bfloat16().float(), pad_v)
    assert (img["out"] == R.SENTINEL).all()
    if lay.k_in_q:
        assert img["k"] is img["q"] and lay.ldq == lay.ldk == 2 * d and lay.k_off == d
        both = torch.cat([lay.q_index.flatten(), lay.k_index.flatten(), lay.k_pad.flatten()])
        assert both.unique().numel() == both.numel()
    if case.S_tail:
        assert torch.equal(img["ktail"][lay.tail_index], ops["ktail"]) and int(lay.tail_index.max()) < lay.tail_elems


def test_header_and_ctypes_mirror_of_the_entry_point_agree():
    header = open(os.path.join(ROOT, "include", "a2p_hip.h")).read()
    body = re.search(r"typedef struct a2p_attention_case \{(.*?)\} a2p_attention_case;", header, re.S).group(1)
    names, sizes = [], {"int64_t": 8, "int32_t": 4}
    for decl in filter(None, (s.strip() for s in body.split(";"))):
        typ, rest = decl.rsplit(" ", 1)[0], decl
        if "*" in decl:
            names.append((decl.rsplit("*", 1)[1].strip(), 8))
        else:
            typ, rest = decl.split(" ", 1)
            names += [(n.strip(), sizes[typ]) for n in rest.split(",")]
    fields = [(n, C.sizeof(t)) for n, t in _lib.A2PAttentionCase._fields_]
    assert fields == names
    assert "a2p_attention_ex" in _lib.EXPORTS and re.search(r"\bint a2p_attention_ex\(a2p_ctx\* ctx, const a2p_attention_case\*", header)
