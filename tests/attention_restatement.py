"""Cases, inputs, a float64 torch restatement, the dispatcher's rule and the derived per-element error bound of the attention family
(csrc/kernels_attn.h attn_kernel / attn_ksplit_kernel, kernels_attn3.h attn3_kernel, all behind
launch_attn / attn_pick of csrc/a2p_lib.hip).  Test infrastructure: shared by tests/test_attention_family_cpu.py and
tests/test_attention_family_hip.py.

Every case is ONE launch of the dispatcher through a2p_attention_ex (include/a2p_hip.h a2p_attention_case), with every field of the
kernels' parameter block (AttnP) set by the case: K/V slot indirection, the fp32 time-token tail, padded 64-key tiles, strides with
gaps.  Operands are rounded to the mode's 16-bit type on the CPU, so the kernel's operand cast is exact and `restate` sees exactly
the kernel's inputs:

    out[seq, t, h, :] = sum_j w_j v_j,   w = softmax_j(s_j),   s_j = q . k_j / sqrt(dh)      over the S = S_main + S_tail valid keys

The bound (see `bound`) allows what separates a correct kernel from that -- fp32 accumulation, the 16-bit P operand, the 16-bit
store -- and nothing else."""
import math
import zlib
from dataclasses import dataclass
from typing import Tuple

import torch

from gemm_restatement import B16, GUARD_ROWS, MODES, SENTINEL, U_OUT, round_to, rup

D_MODEL = 256
U32 = 2.0 ** -24
THR3 = 8.0                  # attn3_kernel: log2 units a score may exceed the lazy reference by (A2P_ATTN3_THR)
ENVELOPE_16BIT = 20.0       # A2P_LOGIT_ENVELOPE_16BIT (include/a2p_hip.h; INTEGRATION.md "validity envelope")
K_ATTN, K_KSPLIT, K_ATTN3 = 0, 1, 3                     # ATTN_K_* of csrc/a2p_lib.hip; 2 is unused
KERNEL_NAMES = ("attn", "ksplit", None, "attn3")
PAD_BIG_K, PAD_BIG_V = 12.0, 28672.0   # "big" padding: finite, exact in all three types; a K row of +-12 is what a 6x spike looks like

# The instances a case runs as: name -> (environment switches, modes).  "default" leaves every switch alone.
INSTANCES = {
    "attn": ({"A2P_ATTN3": "0"}, MODES),
    "attn3": ({"A2P_ATTN3": "2"}, B16),
    "ks4q1": ({"A2P_ATTN_KSPLIT": "1", "A2P_KSPLIT_NW": "4"}, B16),
    "ks8q1": ({"A2P_ATTN_KSPLIT": "1", "A2P_KSPLIT_NW": "8"}, B16),
    "default": ({}, MODES),
}
ENV_NAMES = ("A2P_ATTN3", "A2P_ATTN_KSPLIT", "A2P_KSPLIT_NW", "A2P_NO_KSPLIT")
FORCED = ("attn", "attn3", "ks4q1", "ks8q1")


@dataclass(frozen=True)
class Case:
    name: str
    H: int                       # 4: head_dim 64, 8: head_dim 32 (d = 256)
    nseq: int
    Tq: int
    S_main: int
    S_tail: int = 0
    tail_mod: int = 1
    slots: str = "seq"           # "seq" (no table) | "table" (permuted, slot 0 shared) | "rule1" | "rule2" | "rule3"
    kv_stream: int = 0
    layout: str = "plain"        # "plain" | "self" (Q and K interleaved in one [T][2d] buffer) | "gaps" (every stride larger than its extent)
    data: str = "plain"          # "plain" | "spike" | "spike_last" | "spike_pad0" | "neg"
    pad: str = "nan"             # K pad rows / V^T pad columns: "nan" | "big"
    ksplit: int = 0              # launch_attn's ksplit request
    nseq_rule: int = 0
    instances: Tuple[str, ...] = FORCED
    data_of: str = ""            # the case whose operands this one shares (default: its own, seeded by its name)

    @property
    def dh(self):
        return D_MODEL // self.H

    @property
    def S(self):
        return self.S_main + self.S_tail

    @property
    def Sp(self):
        return rup(self.S, 64)

    @property
    def slot_b(self):
        return self.nseq // 2

    @property
    def nsamp(self):
        return min(self.tail_mod, self.nseq)

    def slot_table(self):
        """The explicit table of slots == "table": a permutation of 1 .. with slot 0 shared by every odd sequence."""
        return [0 if s % 2 else 1 + (self.nseq - 2 - s) // 2 for s in range(self.nseq)] if self.slots == "table" else None

    def slot_of(self, seq):
        if self.slots == "rule1":
            return 1 + seq
        if self.slots == "rule2":
            return 0
        if self.slots == "rule3":
            return 1 + seq if seq < self.slot_b else 0
        if self.slots == "table":
            return self.slot_table()[seq]
        return seq

    @property
    def nslots(self):
        return 1 + max(self.slot_of(s) for s in range(self.nseq))

    @property
    def slot_rule(self):
        return {"rule1": 1, "rule2": 2, "rule3": 3}.get(self.slots, 0)


def _cases():
    cs = []
    add = lambda *a, **k: cs.append(Case(*a, **k))
    alt = lambda i: dict(H=(4, 8)[i % 2], pad=("nan", "big")[(i // 2) % 2])
    # key edges: every remainder class of the 64-key tile, one to three tiles; 513 / 577: 9 and 10 tiles for the 8-wave key split
    for i, S in enumerate((1, 5, 63, 64, 65, 127, 128, 129, 190, 513, 577)):
        add(f"keys/s{S}", nseq=1, Tq=17, S_main=S, **alt(i))
    add("keys/s577_ksplit_request", H=4, nseq=1, Tq=17, S_main=577, ksplit=1, instances=("default",))
    # time-token tails: S_main % 64 = 0 (the last tile is all tail), 1, 62 (the tail just fits), 63 (the tail straddles two tiles)
    i = 0
    for S_main in (1, 62, 63, 64, 65, 126, 127, 128):
        for S_tail in (1, 2):
            nseq = (2, 4)[i % 2]
            add(f"tail/m{S_main}t{S_tail}", nseq=nseq, Tq=(16, 33)[(i // 2) % 2], S_main=S_main, S_tail=S_tail, tail_mod=(1, nseq // 2)[(i // 3) % 2],
                slots=("rule3", "seq", "rule1")[i % 3], data=("plain", "spike_last")[(i // 4) % 2], **alt(i))
            i += 1
    # query edges: the 16-query tile, the 32-query wave, the 128-query and 320-query workgroups (321: one workgroup + one query)
    for i, Tq in enumerate((1, 15, 16, 17, 33, 127, 128, 129, 321)):
        add(f"queries/t{Tq}", nseq=1, Tq=Tq, S_main=(65, 100)[i % 2], **alt(i + 1))
    # slots
    add("slots/table", H=4, nseq=4, Tq=17, S_main=70, slots="table", layout="gaps", pad="big")
    add("slots/rule1", H=8, nseq=2, Tq=17, S_main=70, slots="rule1", pad="nan")
    add("slots/rule2", H=4, nseq=3, Tq=17, S_main=70, slots="rule2", layout="gaps", pad="nan")
    add("slots/rule3", H=8, nseq=4, Tq=17, S_main=70, S_tail=2, tail_mod=2, slots="rule3", layout="gaps", pad="big")
    add("slots/rule3_stream", H=8, nseq=4, Tq=17, S_main=70, S_tail=2, tail_mod=2, slots="rule3", layout="gaps", pad="big", kv_stream=1, data_of="slots/rule3")
    add("slots/table_stream", H=4, nseq=4, Tq=17, S_main=70, slots="table", layout="gaps", pad="big", kv_stream=1, data_of="slots/table")
    # grid: (sequence, head) pairs a multiple of 8 (XCD remap on) and not (off), two query blocks in every kernel
    add("grid/remap", H=4, nseq=2, Tq=321, S_main=65, pad="big")
    add("grid/remap_h8", H=8, nseq=2, Tq=321, S_main=65, slots="rule1", pad="nan")
    add("grid/noremap", H=4, nseq=3, Tq=321, S_main=65, pad="nan")
    # layouts
    add("layout/self", H=4, nseq=2, Tq=100, S_main=100, layout="self", pad="nan")
    add("layout/self_h8", H=8, nseq=3, Tq=70, S_main=129, layout="self", pad="big")
    add("layout/gaps", H=8, nseq=2, Tq=33, S_main=129, S_tail=2, tail_mod=2, layout="gaps", pad="nan")
    # data
    add("data/spike", H=4, nseq=1, Tq=33, S_main=250, data="spike", pad="nan")
    add("data/spike_h8", H=8, nseq=1, Tq=161, S_main=577, data="spike", pad="big")
    add("data/spike_last", H=4, nseq=1, Tq=33, S_main=190, data="spike_last", pad="big")
    add("data/spike_pad0", H=8, nseq=1, Tq=33, S_main=129, data="spike_pad0", pad="nan")
    add("data/spike_pad0_tail", H=4, nseq=2, Tq=33, S_main=128, S_tail=2, data="spike_pad0", pad="big")
    add("data/neg", H=4, nseq=1, Tq=33, S_main=190, data="neg", pad="nan")
    add("data/neg_h8", H=8, nseq=1, Tq=33, S_main=129, S_tail=1, data="neg", pad="big")
    # the default rule: attn3_kernel by size alone (nseq_rule = the unsharded batch), attn_kernel below it, key split on request
    add("rule/attn3_by_size", H=4, nseq=1, Tq=160, S_main=65, nseq_rule=40, instances=("default",))
    add("rule/attn_below_160", H=4, nseq=1, Tq=159, S_main=65, nseq_rule=40, instances=("default",))
    add("rule/ksplit_request", H=8, nseq=2, Tq=33, S_main=65, S_tail=2, ksplit=1, instances=("default",))
    return cs


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def instances_of(case, mode):
    return [i for i in case.instances if mode in INSTANCES[i][1]]


# ----------------------------------------------------------------------------- operands
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def spike_keys(case):
    """(key multiplied by 6, key multiplied by -5 or None)."""
    S = case.S
    if case.data == "spike":
        return S // 2, (3 * S) // 4
    if case.data == "spike_last":
        return S - 1, None
    if case.data == "spike_pad0":
        assert S % 64, "spike_pad0 needs a partial last tile"
        return (S - 1) // 64 * 64, None
    return None, None


def make_operands(case, mode):
    """float32 CPU tensors, already rounded to the mode's operand type: Q [nseq, Tq, d], K / V [nslots, S_main, d], ktail / vtail
    [nsamp, S_tail, d].  Every (slot, head) and tail sample has its own mean of V, so a wrong slot, head or sample is a gross error."""
    g = _gen(case.data_of or case.name)
    d, H, dh = D_MODEL, case.H, case.dh
    nsl, nsa = case.nslots, case.nsamp
    Q = torch.randn(case.nseq, case.Tq, d, generator=g)
    K = 0.6 * torch.randn(nsl, case.S_main, d, generator=g)
    V = torch.randn(nsl, case.S_main, d, generator=g)
    kt = torch.randn(nsa, case.S_tail, d, generator=g)         # time tokens draw weight: a misplaced one is visible in many rows
    vt = torch.randn(nsa, case.S_tail, d, generator=g)
    head = torch.arange(d) // dh
    V += (torch.arange(nsl).view(-1, 1, 1) + 1.0) + 0.1 * head
    vt -= 2.0 * (torch.arange(nsa).view(-1, 1, 1) + 1.0) + 0.1 * head + torch.arange(case.S_tail).view(1, -1, 1)
    if case.data == "neg":      # every score near -1.2 sqrt(dh)
        base = torch.randn(H, dh, generator=g).flatten()
        Q = base + 0.3 * Q
        K = -1.2 * base + 0.5 * K
        kt = -1.2 * base + 0.5 * kt
    Q[:, case.Tq - 1] *= 1.25     # the row the clamped loads repeat
    j6, j5 = spike_keys(case)
    for j, f in ((j6, 6.0), (j5, -5.0)):
        if j is None:
            continue
        if j < case.S_main:
            K[:, j] *= f
        else:
            kt[:, j - case.S_main] *= 0.6 * f
    return {k: round_to(v, mode) for k, v in dict(Q=Q, K=K, V=V, ktail=kt, vtail=vt).items()}


def gather(case, ops, seq, dtype=torch.float64):
    """Keys and values of one sequence: ([S, d], [S, d]) -- the slot's main rows, then tail rows of sample seq % tail_mod."""
    slot = case.slot_of(seq)
    k, v = ops["K"][slot].to(dtype), ops["V"][slot].to(dtype)
    if case.S_tail:
        sa = seq % case.tail_mod
        k, v = torch.cat([k, ops["ktail"][sa].to(dtype)]), torch.cat([v, ops["vtail"][sa].to(dtype)])
    return k, v


def restate(case, ops):
    """float64: ref [nseq, Tq, d]; mag_v = sum_j w_j |v_jd| and mag_dv = sum_j w_j |v_jd - ref_d| per element; vabs = sum_j |v_jd|
    [nseq, 1, d]; qk_abs = max over the valid keys of sum_i |q_i k_ji| / sqrt(dh) and kabs = max_j sum_i |k_ji|, per row and head,
    repeated over the head's columns [nseq, Tq, d]; logit_max: the largest scaled logit over valid keys of the whole launch."""
    H, dh, Tq = case.H, case.dh, case.Tq
    out = {k: [] for k in ("ref", "mag_v", "mag_dv", "vabs", "qk_abs", "kabs")}
    lmax = -math.inf
    for seq in range(case.nseq):
        k, v = gather(case, ops, seq)
        q = ops["Q"][seq].double().view(Tq, H, dh).transpose(0, 1)             # [H, Tq, dh]
        kh, vh = k.view(-1, H, dh).transpose(0, 1), v.view(-1, H, dh).transpose(0, 1)   # [H, S, dh]
        s = q @ kh.transpose(1, 2) / math.sqrt(dh)                              # [H, Tq, S]
        lmax = max(lmax, float(s.max()))
        w = torch.softmax(s, dim=-1)
        ref = w @ vh                                                            # [H, Tq, dh]
        mag_v = w @ vh.abs()
        mag_dv = torch.stack([(w[h].unsqueeze(-1) * (vh[h].unsqueeze(0) - ref[h].unsqueeze(1)).abs()).sum(1) for h in range(H)])
        qk_abs = (q.abs() @ kh.abs().transpose(1, 2) / math.sqrt(dh)).max(-1).values          # [H, Tq]
        kabs = kh.abs().sum(-1).max(-1).values                                   # [H]
        cols = lambda t: t.transpose(0, 1).reshape(Tq, H * dh)
        out["ref"].append(cols(ref)); out["mag_v"].append(cols(mag_v)); out["mag_dv"].append(cols(mag_dv))
        out["vabs"].append(v.abs().sum(0, keepdim=True))
        out["qk_abs"].append(cols(qk_abs.unsqueeze(-1).expand(H, Tq, dh)))
        out["kabs"].append(cols(kabs.view(H, 1, 1).expand(H, Tq, dh)))
    r = {k: torch.stack(v) for k, v in out.items()}
    r["logit_max"] = lmax
    return r


# ----------------------------------------------------------------------------- the dispatcher's rule
def pick(mode, case, env=None):
    """attn_pick of csrc/a2p_lib.hip restated from launch_attn's rule: (kernel, operand bits, head_dim, waves, 16-query tiles per wave,
    query blocks per (sequence, head), workgroups, xcd_remap).  env: the A2P_* switches."""
    env = env or {}
    num = lambda n, dflt: int(env.get(n, dflt))
    b16, H, dh, Tq, S = mode != "fp32", case.H, case.dh, case.Tq, case.S
    pairs = H * case.nseq
    nseq_rule = case.nseq_rule if case.nseq_rule > 0 else case.nseq
    ceil = lambda a, b: -(-a // b)
    # the key-split kernel: on request (small forwards) or forced, 16-bit only, at most two tail rows
    if (case.ksplit or "A2P_ATTN_KSPLIT" in env) and b16 and "A2P_NO_KSPLIT" not in env and case.S_tail <= 2:
        nw = num("A2P_KSPLIT_NW", 0)
        w8 = nw == 8 or (nw == 0 and ceil(S, 64) > 8)          # 8 waves once 4 would walk more than two tiles each
        nq = ceil(Tq, 16)
        return (K_KSPLIT, 16, dh, 8 if w8 else 4, 1, nq, nq * pairs, 0)
    remap = 1 if pairs % 8 == 0 else 0
    nq, nq3 = ceil(Tq, 128), ceil(Tq, 320)
    a3 = num("A2P_ATTN3", 1)
    if b16 and a3:
        # where it wins: >= 160 queries, more than one attn_kernel workgroup per CU (256) in the rule's batch, and long key ranges
        # (>= 1024) -- or, at head_dim 64, at most one attn3 workgroup per CU
        wins = Tq >= 160 and nq * H * nseq_rule > 256 and ((dh == 64 and (S >= 1024 or nq3 * H * nseq_rule <= 256)) or (dh == 32 and S >= 1024))
        if a3 >= 2 or wins:
            return (K_ATTN3, 16, dh, 4, 5, nq3, nq3 * pairs, remap)
    return (K_ATTN, 16 if b16 else 32, dh, 4, 2, nq, nq * pairs, remap)


# ----------------------------------------------------------------------------- buffers
@dataclass
class Layout:
    q_elems: int; k_elems: int; vt_elems: int; out_elems: int; tail_elems: int
    q_off: int; k_off: int; vt_off: int; out_off: int
    q_seq_stride: int; ldq: int; k_slot_stride: int; ldk: int; vt_slot_stride: int; ldvt: int; o_seq_stride: int; ldo: int
    tail_sample_stride: int; tail_row_stride: int
    k_in_q: bool
    q_index: torch.Tensor        # element of the Q image per [nseq, Tq, d]
    k_index: torch.Tensor        # element of the K image (the Q image when k_in_q) per [nslots, S_main, d]
    k_pad: torch.Tensor          # ... of the K pad rows [nslots, Sp - S_main, d]
    vt_index: torch.Tensor       # element of the V^T image per [nslots, S_main, d] (of V, i.e. transposed access)
    vt_pad: torch.Tensor         # ... of the V^T pad columns [nslots, Sp - S_main, d]
    tail_index: torch.Tensor     # [nsamp, S_tail, d]
    out_index: torch.Tensor      # [nseq, Tq, d]
    written: torch.Tensor        # bool [out_elems]


def layout(case, mode="fp32"):
    """Element indices of every buffer of a case and the exact write set of O.  O has GUARD_ROWS rows on both sides; "gaps" adds
    ldo = d + 8 and two unwritten rows between sequences, ldvt = Sp + 64, slot strides larger than a slot, a padded tail row and sample
    stride; "self" puts Q and K into one [row][Q | K] buffer (ldq = ldk = 2d) with K's slot = the sequence."""
    d, Tq, Sm, Sp, nseq, nsl = D_MODEL, case.Tq, case.S_main, case.Sp, case.nseq, case.nslots
    gaps = case.layout == "gaps"
    ar = torch.arange
    ldo = d + 8 if gaps else d
    o_seq = Tq * ldo + (2 * ldo if gaps else 0)
    out_off = GUARD_ROWS * ldo
    out_elems = out_off + (nseq - 1) * o_seq + Tq * ldo + GUARD_ROWS * ldo
    out_index = out_off + ar(nseq).view(-1, 1, 1) * o_seq + ar(Tq).view(1, -1, 1) * ldo + ar(d)
    written = torch.zeros(out_elems, dtype=torch.bool)
    written[out_index.flatten()] = True
    if case.layout == "self":
        assert case.slots == "seq"
        rows = max(Tq, Sp)
        ldq = ldk = 2 * d
        q_seq = k_slot = rows * ldq
        q_off, k_off, q_elems, k_elems, k_in_q = 0, d, nseq * rows * ldq, 0, True
    else:
        ldq = d + 8 if gaps else d
        q_seq = Tq * ldq + (8 if gaps else 0)
        q_off, q_elems = (16 if gaps else 0), (16 if gaps else 0) + nseq * q_seq
        ldk = d + 8 if gaps else d
        k_slot = Sp * ldk + (64 * ldk if gaps else 0)
        k_off, k_elems, k_in_q = (8 if gaps else 0), (8 if gaps else 0) + nsl * k_slot, False
    q_index = q_off + ar(nseq).view(-1, 1, 1) * q_seq + ar(Tq).view(1, -1, 1) * ldq + ar(d)
    krow = lambda r: k_off + ar(nsl).view(-1, 1, 1) * k_slot + r.view(1, -1, 1) * ldk + ar(d)
    ldvt = Sp + 64 if gaps else Sp
    vt_slot = d * ldvt + (8 * ldvt if gaps else 0)
    vt_off = 24 if gaps else 0
    vt_elems = vt_off + nsl * vt_slot
    vcol = lambda r: vt_off + ar(nsl).view(-1, 1, 1) * vt_slot + ar(d).view(1, 1, -1) * ldvt + r.view(1, -1, 1)
    trs = d + 8 if gaps else d
    tss = case.S_tail * trs + (12 if gaps else 0)
    tail_index = ar(case.nsamp).view(-1, 1, 1) * tss + ar(case.S_tail).view(1, -1, 1) * trs + ar(d)
    return Layout(q_elems, k_elems, vt_elems, out_elems, max(case.nsamp * tss, 8), q_off, k_off, vt_off, out_off, q_seq, ldq, k_slot, ldk, vt_slot, ldvt,
                  o_seq, ldo, tss, trs, k_in_q, q_index, krow(ar(Sm)), krow(ar(Sm, Sp)), vcol(ar(Sm)), vcol(ar(Sm, Sp)), tail_index, out_index, written)


def _pad_values(shape, kind, big):
    """NaN bit patterns (quiet NaNs of both signs, exact in all three types) or +-big, alternating by element."""
    n = int(torch.tensor(shape).prod()) if len(shape) else 1
    sign = 1.0 - 2.0 * (torch.arange(n) % 2).float()
    if kind == "nan":
        bits = torch.where(sign > 0, torch.tensor(0x7FC00000), torch.tensor(0xFFC00000 - (1 << 32))).to(torch.int32)
        return bits.view(torch.float32).view(shape)
    return (sign * big).view(shape)


def make_images(case, ops, lay):
    """The fp32 images a2p_attention_ex takes (CPU): everything that is no operand is NaN -- a read of it shows -- except K pad rows and
    V^T pad columns, which follow the case's padding policy, and O, which is the sentinel everywhere."""
    nan = float("nan")
    img = {"q": torch.full((lay.q_elems,), nan), "vt": torch.full((lay.vt_elems,), nan), "out": torch.full((lay.out_elems,), SENTINEL),
           "ktail": torch.full((lay.tail_elems,), nan), "vtail": torch.full((lay.tail_elems,), nan)}
    img["k"] = img["q"] if lay.k_in_q else torch.full((lay.k_elems,), nan)
    img["q"][lay.q_index.flatten()] = ops["Q"].flatten()
    img["k"][lay.k_index.flatten()] = ops["K"].flatten()
    img["vt"][lay.vt_index.flatten()] = ops["V"].flatten()
    img["k"][lay.k_pad.flatten()] = _pad_values(tuple(lay.k_pad.shape), case.pad, PAD_BIG_K).flatten()
    img["vt"][lay.vt_pad.flatten()] = _pad_values(tuple(lay.vt_pad.shape), case.pad, PAD_BIG_V).flatten()
    if case.S_tail:
        img["ktail"][lay.tail_index.flatten()] = ops["ktail"].flatten()
        img["vtail"][lay.tail_index.flatten()] = ops["vtail"].flatten()
    return img


# ----------------------------------------------------------------------------- the bound
def logit_delta(case, mode, kernel, r):
    """Perturbation of a scaled logit (natural units) by the kernel's arithmetic, per element of the row's head block.

    fp32 accumulation: s_j is a dh-term dot product accumulated in fp32 (16-bit products are exact in fp32: dh + 8 roundings; fp32
    products round once more each: 2 dh + 8), in an unspecified order (factor 2, as for the GEMMs): 2 (dh | 2 dh + 8) u32 sum_i |q_i k_ji|.  The scale constant log2(e) / sqrt(dh),
    the fma against the running maximum and the difference of two running maxima in front of every rescale (one per tile) each round
    once relative to a magnitude <= max_j |s_j| <= A = max_j sum_i |q_i k_ji| / sqrt(dh): (8 + 2 ntiles) u32 A.
    attn3_kernel only: Q is multiplied by the scale in fp32 and rounded to the 16-bit type before the dot product: (u + 2 u32) A, plus
    in IEEE half the absolute 2^-25 of a subnormal result, times sum_i |k_ji|, times ln 2 (the scores are in log2 units there)."""
    ntiles = case.Sp // 64
    A = r["qk_abs"]
    terms = (2 if mode == "fp32" else 1) * case.dh + 8
    delta = U32 * (2 * terms + 8 + 2 * ntiles) * A
    if kernel == K_ATTN3:
        delta = delta + (U_OUT[mode] + 2 * U32) * A
        if mode == "fp16":
            delta = delta + 2.0 ** -25 * math.log(2.0) * r["kabs"]
    return delta


def bound(case, mode, kernel, r, exp2_rel=0.0):
    """Per-element bound on |kernel - ref| [nseq, Tq, d], from unit roundoffs only: u32 = 2^-24, u = U_OUT[mode] (the 16-bit store and P
    operand; 0 in fp32).  With w the exact softmax weights, out = ref, Mv = sum_j w_j |v_jd|, Dv = sum_j w_j |v_jd - out_d|:

      logits      a perturbation |delta_j| <= delta of the logits moves the weights by factors within e^(+-2 delta) after
                  renormalisation: |d out| <= expm1(2 delta) Dv, delta from `logit_delta` (fp32 accumulation over dh; attn3: the rounded
                  pre-scaled Q).  exp2_rel, the relative error of the hardware exp2, enters the same way (not derivable: the caller's
                  measured constant, 0.0 until measured).
      P operand   16-bit modes: P_j (1 + rho_j), |rho_j| <= u, in the numerator.  attn_kernel / ksplit keep the UNROUNDED fp32 P
                  in the row sum: d out = sum_j w_j rho_j v_j = (P rounding against the weighted mean, <= u Dv) + (mismatch of the row
                  sum, <= u |out|), bounded together by u Mv.  attn3 sums the rounded P (its row sums are MFMAs on the P operand), so
                  the rounding renormalises: expm1(2 u) Dv; its P reaches 2^8 relative to the lazy reference -- the same relative
                  rounding.  IEEE half: a P below 2^-14 is subnormal, absolute error 2^-25 against a row sum >= 1 (the key that set the
                  reference contributes exactly 1): 2^-25 sum_j |v_jd|.
      sums        numerator and row sum are fp32 sums over the S keys (product and add: 2 S roundings; fp32 mode rounds the products
                  too and is covered by the same count), rescaled once per tile and merged / normalised at the end (4 ntiles + 16),
                  order unspecified (factor 2), each relative to sum_j w_j |v_jd|: 2 * 2 (2 S + 4 ntiles + 16) u32 Mv.
      store       the result rounds to the stored type: u |out|, and scales the terms above by (1 + u)."""
    u, S, ntiles = U_OUT[mode], case.S, case.Sp // 64
    ref, Mv, Dv = r["ref"].abs(), r["mag_v"], r["mag_dv"]
    delta = logit_delta(case, mode, kernel, r) + exp2_rel
    b = torch.expm1(2 * delta) * Dv
    if u:
        b = b + (math.expm1(2 * u) * Dv if kernel == K_ATTN3 else u * Mv)
        if mode == "fp16":
            b = b + 2.0 ** -25 * r["vabs"]
    b = b + 4 * (2 * S + 4 * ntiles + 16) * U32 * Mv
    return b * (1 + u) + u * ref


def logit_max_bound(case, mode, kernel, r):
    """Bound on |reported logit maximum - float64 maximum over valid keys|: the row's logit perturbation plus the conversions between
    log2 and natural units in fp32 (three roundings relative to the maximum's magnitude <= A)."""
    return float((logit_delta(case, mode, kernel, r) + 8 * U32 * r["qk_abs"]).max())


# ----------------------------------------------------------------------------- plain emulations of the three kernel families
FAULTS = ("pad_unmasked", "v_pad_kept", "tail_row1_at_s_main", "tail_sample_is_seq", "rule3_last_cond_slot0", "q_row_shift", "no_rescale",
          "head_shift")


def _padded_kv(case, ops, seq, fault):
    """fp32 K [Sp, d] and V [Sp, d] of a sequence as the tile loop sees them: slot rows, tail rows patched in, padding as the case
    fills it."""
    slot = case.slot_of(seq)
    if fault == "rule3_last_cond_slot0" and case.slots == "rule3" and seq == case.slot_b - 1:
        slot = 0
    Sp, Sm, d = case.Sp, case.S_main, D_MODEL
    K = torch.cat([ops["K"][slot], _pad_values((Sp - Sm, d), case.pad, PAD_BIG_K)])
    V = torch.cat([ops["V"][slot], _pad_values((Sp - Sm, d), case.pad, PAD_BIG_V)])
    if case.S_tail:
        sa = seq % case.tail_mod
        if fault == "tail_sample_is_seq":
            sa = min(seq, case.nsamp - 1)
        for j in range(case.S_tail):
            at = Sm + j
            if fault == "tail_row1_at_s_main" and j == 1:
                at = Sm
            K[at], V[at] = ops["ktail"][sa, j], ops["vtail"][sa, j]
    return K.clone(), V.clone()


def emulate(case, mode, family, ops, fault=None, nw=4):
    """The kernel families in plain fp32 torch, [nseq, Tq, d] rounded to the stored type.
    "online": attn_kernel -- online softmax per 64-key tile, 16-bit P operand, fp32 row sum of the unrounded P;
    "ksplit": attn_ksplit_kernel -- wave w of nw walks tiles w, w + nw, ..; partial (m, l, O) states merged by log-sum-exp;
    "lazy":   attn3_kernel -- Q pre-scaled by log2(e) / sqrt(dh) and rounded, a reference that moves (for the 80 queries of a wave at
              once) only when a score exceeds it by more than 8, row sums of the ROUNDED P.
    fault: one of FAULTS planted into the arithmetic (None: the correct kernel)."""
    f32 = torch.float32
    H, dh, Tq, S, Sp = case.H, case.dh, case.Tq, case.S, case.Sp
    ntiles = Sp // 64
    c = torch.tensor(1.4426950408889634 / math.sqrt(dh), dtype=f32)
    rp = (lambda t: round_to(t, mode))
    out = torch.empty(case.nseq, Tq, D_MODEL, dtype=f32)
    for seq in range(case.nseq):
        K, V = _padded_kv(case, ops, seq, fault)
        Q = ops["Q"][seq].clone()
        if fault == "q_row_shift" and Tq >= 2:
            Q[Tq - 2] = Q[Tq - 1]
        q = Q.view(Tq, H, dh).transpose(0, 1)                                   # [H, Tq, dh]
        kh, vh = K.view(Sp, H, dh).transpose(0, 1), V.view(Sp, H, dh).transpose(0, 1).clone()
        valid = torch.arange(Sp) < S
        if fault == "pad_unmasked" and Sp > S:
            valid[S] = True
        if fault != "v_pad_kept":
            vh[:, S:] = 0.0
        if family == "lazy":
            q = rp(q * c)
            cc = torch.tensor(1.0, dtype=f32)
        else:
            cc = c

        def tile_scores(t):
            s = q @ kh[:, 64 * t: 64 * t + 64].transpose(1, 2)                  # [H, Tq, 64], fp32
            return s, valid[64 * t: 64 * t + 64]

        def online(tiles, skip_rescale_at=None):
            m = torch.full((H, Tq), -math.inf, dtype=f32)
            l = torch.zeros(H, Tq, dtype=f32)
            o = torch.zeros(H, Tq, dh, dtype=f32)
            for n, t in enumerate(tiles):
                s, ok = tile_scores(t)
                s = torch.where(ok, s, torch.tensor(-math.inf, dtype=f32))
                mnew = torch.maximum(m, s.max(-1).values * cc)
                alpha = torch.exp2(m - mnew)
                p = torch.exp2(s * cc - mnew.unsqueeze(-1))
                l = l * alpha + p.sum(-1)
                if not (skip_rescale_at is not None and n == skip_rescale_at):
                    o = o * alpha.unsqueeze(-1)
                o = o + rp(p) @ vh[:, 64 * t: 64 * t + 64]
                m = mnew
            return m, l, o

        if family == "online":
            m, l, o = online(range(ntiles), 1 if fault == "no_rescale" else None)
            res = o / l.unsqueeze(-1)
        elif family == "ksplit":
            parts = [online(range(w, ntiles, nw)) for w in range(min(nw, ntiles))]
            mall = torch.stack([p[0] for p in parts]).max(0).values
            lall = torch.zeros(H, Tq, dtype=f32)
            acc = torch.zeros(H, Tq, dh, dtype=f32)
            for w, (m, l, o) in enumerate(parts):
                a = torch.exp2(m - mall)
                lall = lall + a * l
                acc = acc + o * (1.0 if (fault == "no_rescale" and w == 1) else a.unsqueeze(-1))
            res = acc / lall.unsqueeze(-1)
        else:
            nwv = -(-Tq // 80)                                                  # the vote is per wave of 80 queries (of one head)
            real = torch.arange(Sp) < S
            mref = torch.zeros(H, Tq, dtype=f32)
            mrel = torch.full((H, Tq), -math.inf, dtype=f32)                    # running maximum relative to the reference
            l = torch.zeros(H, Tq, dtype=f32)
            o = torch.zeros(H, Tq, dh, dtype=f32)
            moves = 0
            for t in range(ntiles):
                s, ok = tile_scores(t)
                s = torch.where(real[64 * t: 64 * t + 64], s, s[..., :1].expand_as(s))   # K rows past the end are copies of the tile's key 0
                mrel = torch.maximum(mrel, (s - mref.unsqueeze(-1)).max(-1).values)
                over = torch.zeros(H, nwv * 80, dtype=torch.bool)
                over[:, :Tq] = mrel > THR3
                move = over.view(H, nwv, 80).any(-1, keepdim=True).expand(H, nwv, 80).reshape(H, -1)[:, :Tq] if t else torch.ones(H, Tq, dtype=torch.bool)
                dmove = torch.where(move, mrel, torch.zeros_like(mrel))         # the references move to the exact running maxima
                f = torch.exp2(-dmove)
                mref, mrel, l = mref + dmove, mrel - dmove, l * f
                planted = fault == "no_rescale" and t > 0 and moves == 0 and bool(move.any())
                if not planted:
                    o = o * f.unsqueeze(-1)
                moves += int(t > 0 and bool(move.any()))
                p = rp(torch.exp2(s - mref.unsqueeze(-1)))
                l = l + (p * ok).sum(-1)                                        # the ones fragment is zero on the padding
                o = o + p @ vh[:, 64 * t: 64 * t + 64]
            res = o / l.unsqueeze(-1)
        res = res.transpose(0, 1).reshape(Tq, H * dh)
        if fault == "head_shift":
            res = res.clone()
            res[:, dh: 2 * dh] = res[:, :dh]
        out[seq] = res
    return rp(out)


FAMILY_OF = {K_ATTN: "online", K_KSPLIT: "ksplit", K_ATTN3: "lazy"}
