"""Cases, inputs, a float64 torch restatement and the derived per-element error bound of the GEMM family
(csrc/kernels_gemm.h: gemm_kernel with its epilogues, skinny_gemm_kernel, skinny_gemm_group_kernel).  Test infrastructure:
shared by tests/test_gemm_family_cpu.py and tests/test_gemm_family_hip.py.

Every case is ONE launch of the dispatcher (a2p_gemm_ex / a2p_skinny_gemm_ex).  The restatement computes, from operands already
rounded to the mode's 16-bit type on the CPU (or split into hi / lo pieces for split rows),

    acc[m][n] = sum over tap, k of A[m + tap * dil][k] * W[tap][n][k]        pre = acc + bias

and the epilogue in `dtype` (float64: the reference; float32: the self-check of the bound).  What separates a correct kernel from it
is fp32 accumulation and the rounding of the stored value, which is what `bound` allows and nothing else:

    |got - ref| <= L * 2 * (Kc * ntaps + 8) * 2^-24 * (sum |a||w| + |bias| + epilogue terms) + u_out * |ref|

Kc: products per tap that can be non-zero (K, or 3 K for split rows); the factor 2: the MFMA's internal summation order is
unspecified; L: Lipschitz constant of the activation; u_out: unit roundoff of the stored type (0 for fp32)."""
import zlib
from dataclasses import dataclass, field
from typing import Optional, Tuple

import torch

EPI_STORE, EPI_STORE_T, EPI_FILM_RES, EPI_CONV = 0, 1, 2, 3
ACT_NONE, ACT_GELU, ACT_MISH, ACT_SILU, ACT_LRELU, ACT_RELU = 0, 1, 2, 3, 4, 5
MODES = ("fp32", "fp16", "bf16")
B16 = ("fp16", "bf16")
LIPSCHITZ = {ACT_NONE: 1.0, ACT_RELU: 1.0, ACT_LRELU: 1.0, ACT_GELU: 1.13, ACT_MISH: 1.1}
U_OUT = {"fp32": 0.0, "fp16": 2.0 ** -11, "bf16": 2.0 ** -8}
SENTINEL = -24576.0      # -1.5 * 2^14: exact in fp32, IEEE half and bfloat16, far outside the data
GUARD_ROWS = 64


def rup(v, m):
    return (v + m - 1) // m * m


def kstep(mode):
    return 32 if mode == "fp32" else 64


@dataclass(frozen=True)
class Case:
    name: str
    M: int
    N: int
    K: int
    modes: Tuple[str, ...] = MODES
    ntaps: int = 1
    dil: int = 0                 # rows between taps
    epi: int = EPI_STORE
    act: int = ACT_NONE
    out_f32: int = 0
    rows_per_seq: int = 1
    out_seq_pad: int = 0
    film: Optional[bool] = None  # EPI_FILM_RES: True = FiLM table, False = film NULL
    skip: bool = False           # EPI_CONV: averaged skip at + 2 dil rows
    split: bool = False          # split operand rows [hi | lo | hi] x [hi | hi | lo]
    split_third: bool = False    # 16-bit output row [hi | lo | hi]
    dup: bool = False
    bias: bool = True
    seq_zero_rows: int = 0       # conv: the first rows of every sequence of A are zero (left padding)
    ldo_extra: int = 0

    @property
    def a_rows(self):
        return self.M + (self.ntaps - 1) * self.dil

    @property
    def nseq(self):
        return (self.M - 1) // self.rows_per_seq + 1


def pick(mode, M, N, ntaps):
    """gemm_pick of csrc/a2p_lib.hip restated (default environment): (element bits, MT, NB)."""
    t128 = (N + 127) // 128
    blocks128 = t128 * ((M + 127) // 128)
    blocks64 = t128 * ((M + 63) // 64)
    if mode == "fp32":
        return (32, 2 if blocks128 < 512 else 4, 2)
    if ntaps > 1 and N <= 128 and blocks64 <= 3 * 256:
        return (16, 1, 2)
    if blocks64 <= 256 and ntaps == 1:
        return (16, 2, 4)
    return (16, 2, 2)


# ----------------------------------------------------------------------------- the curated list
def _cases():
    cs = []
    add = lambda *a, **k: cs.append(Case(*a, **k))
    # M edges of the 32-, 64- and 128-row tiles x the N list (16-bit: <h16, 2, NB = 4>; fp32: <float, 2>)
    for M, N in zip((1, 15, 17, 31, 33, 63, 65, 127, 129), (4, 60, 104, 128, 132, 260, 4, 132, 104)):
        add(f"store/m{M}n{N}", M, N, 100, out_f32=1)
    # K in k-steps: every branch of the 4-deep ring (rem >= 2, rem == 1, rem == 0) and its short prologue, the 2-deep ring, the fp32 loop
    for st in (1, 2, 3, 4, 5, 8):
        add(f"ring4/k{st}", 129, 104, 64 * st, modes=B16, out_f32=1)
        add(f"ring4/k{st}pad", 65, 132, 64 * st - 24, modes=B16)
        add(f"ring2/k{st}", 16401, 4, 64 * st, modes=B16)                  # 257 workgroups of 64 rows
        add(f"f32loop/k{st}", 129, 104, 32 * st, modes=("fp32",))
        add(f"f32loop/k{st}pad", 65, 132, 32 * st - 12, modes=("fp32",), out_f32=1)
    add("ring2/wide_k1", 2100, 1024, 64, modes=B16)                        # 33 x 8 = 264 workgroups
    add("ring2/wide_k2", 2100, 1024, 128, modes=B16, out_f32=1)
    add("f32big/k32", 8130, 1024, 32, modes=("fp32",))                     # 64 x 8 = 512 tiles of 128 x 128: <float, 4>
    add("f32big/k64", 8130, 1024, 64, modes=("fp32",), out_f32=1)
    # epilogues
    for rps in (7, 50, 64):
        add(f"film/rps{rps}", 129, 132, 100, epi=EPI_FILM_RES, rows_per_seq=rps, film=True)
        add(f"nofilm/rps{rps}", 130, 260, 64, epi=EPI_FILM_RES, rows_per_seq=rps, film=False)
    for rps, nseq in ((20, 4), (64, 2), (77, 3)):
        add(f"store_t/rps{rps}", rps * nseq, 132, 100, epi=EPI_STORE_T, rows_per_seq=rps)
    add("store_t/ragged", 77 * 2 + 30, 104, 64, epi=EPI_STORE_T, rows_per_seq=77)   # the last sequence is short
    add("seqpad/f32", 100, 104, 100, rows_per_seq=50, out_seq_pad=24, out_f32=1)
    add("seqpad/t", 150, 132, 64, rows_per_seq=50, out_seq_pad=24)
    add("seqpad/split_third", 100, 104, 100, modes=B16, rows_per_seq=50, out_seq_pad=24, split=True, split_third=True)
    add("dup", 129, 132, 100, out_f32=1, dup=True)
    add("dup/split", 65, 260, 100, modes=B16, out_f32=1, dup=True, split=True)
    add("gelu", 129, 260, 100, act=ACT_GELU)
    add("relu", 65, 132, 100, act=ACT_RELU)
    add("relu/f32", 65, 132, 100, act=ACT_RELU, out_f32=1)
    add("store/nobias", 33, 60, 64, bias=False, ldo_extra=8)
    # dilated conv tail: left-padded [2][50 + 24][C] rows, three taps
    conv = dict(ntaps=3, epi=EPI_CONV, act=ACT_LRELU, rows_per_seq=74, seq_zero_rows=24)
    for dil in (1, 2, 3):
        for split in (False, True):
            sp = dict(split=True, split_third=True, modes=B16) if split else {}
            tag = "x3" if split else "plain"
            add(f"conv/{tag}/skip_d{dil}", 148, 104, 104, dil=dil, skip=True, **conv, **sp)
            add(f"conv/{tag}/128_d{dil}", 148, 128, 128, dil=dil, skip=True, **conv, **sp)
            add(f"conv/{tag}/up_d{dil}", 148, 256, 104, dil=dil, **conv, **sp)      # C -> hid: two column tiles, the 2-deep ring
            add(f"conv/{tag}/down_d{dil}", 148, 104, 256, dil=dil, **conv, **sp)    # hid -> C
    return cs


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}

# (M, N, K, lda extra, ldo extra, act, bias)
SKINNY_CASES = [
    (1, 16, 64, 0, 0, ACT_NONE, True), (2, 48, 128, 4, 8, ACT_MISH, True), (15, 16, 2048, 0, 0, ACT_MISH, True),
    (16, 48, 64, 8, 0, ACT_NONE, False), (17, 1536, 128, 0, 16, ACT_NONE, True), (48, 16, 128, 4, 4, ACT_MISH, False),
    (63, 48, 2048, 0, 0, ACT_NONE, True), (64, 1536, 64, 0, 0, ACT_MISH, True), (65, 48, 128, 12, 8, ACT_MISH, True),
    (130, 16, 64, 4, 0, ACT_NONE, True), (130, 48, 2048, 0, 4, ACT_MISH, True),
]
# groups of three different (M, N, K): a block that took the wrong descriptor computes another problem
SKINNY_GROUPS = {
    "grouped": [(17, 48, 128, 4, 8, ACT_MISH, True), (64, 16, 2048, 0, 0, ACT_NONE, True), (2, 1536, 64, 8, 4, ACT_MISH, False)],
    "fallback": [(17, 48, 128, 4, 8, ACT_MISH, True), (65, 16, 2048, 0, 0, ACT_NONE, True), (2, 1536, 64, 8, 4, ACT_MISH, False)],
}


# ----------------------------------------------------------------------------- inputs
def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def make_operands(case):
    """float32 CPU tensors of a case: asymmetric random operands with one spiked row of A and one spiked column of the product, so
    that a transposition or a leak of a clamped row shows."""
    g = _gen(case.name)
    A = torch.randn(case.a_rows, case.K, generator=g) + 0.25
    W = torch.randn(case.ntaps, case.N, case.K, generator=g) / (case.K * case.ntaps) ** 0.5
    A[case.a_rows - 1] *= 8.0                 # M - 1 is the row the clamped loads repeat (conv: the deepest tap row)
    A[(case.M - 1) // 2] *= -6.0
    W[:, case.N - 1] *= 8.0                   # N - 1 is the column the clamped loads repeat
    W[:, case.N // 3] *= -6.0
    if case.seq_zero_rows:
        r = torch.arange(case.a_rows)
        A[(r % case.rows_per_seq) < case.seq_zero_rows] = 0.0
    ops = {"A": A, "W": W, "bias": torch.randn(case.N, generator=g) if case.bias else None}
    if case.epi == EPI_FILM_RES:
        ops["x"] = torch.randn(case.M, case.N, generator=g) * 2.0
        if case.film:
            ops["film_scale"] = torch.randn(case.nseq, case.N, generator=g) * 0.5
            ops["film_shift"] = torch.randn(case.nseq, case.N, generator=g)
    return ops


def make_skinny(spec, tag=""):
    M, N, K, la, lo, act, bias = spec
    g = _gen(f"skinny/{tag}/{M}x{N}x{K}")
    A = torch.randn(M, K, generator=g) + 0.25
    W = torch.randn(N, K, generator=g) / K ** 0.5
    A[M - 1] *= 8.0
    A[(M - 1) // 2] *= -6.0
    W[N - 1] *= 8.0
    W[N // 3] *= -6.0
    return {"A": A, "W": W, "bias": torch.randn(N, generator=g) if bias else None}


# ----------------------------------------------------------------------------- restatement
def round_to(t, mode):
    """float32 values after the cast to the mode's operand type."""
    if mode == "fp16":
        return t.half().float()
    if mode == "bf16":
        return t.bfloat16().float()
    return t


def _split(t, mode):
    hi = round_to(t, mode)
    return hi, round_to(t - hi, mode)


def effective_operands(case, ops, mode):
    """(A', W') float32: what the kernel multiplies.  Split rows: A' = [hi | lo | hi], W' = [hi | hi | lo] (kernels_misc.h)."""
    if case.split:
        ah, al = _split(ops["A"], mode)
        wh, wl = _split(ops["W"], mode)
        return torch.cat([ah, al, ah], -1), torch.cat([wh, wh, wl], -1)
    return round_to(ops["A"], mode), round_to(ops["W"], mode)


def activation(x, act):
    if act == ACT_NONE:
        return x
    if act == ACT_GELU:
        return 0.5 * x * (1.0 + torch.erf(x * 0.7071067811865476))
    if act == ACT_MISH:
        return x * torch.tanh(torch.log1p(torch.exp(-x.abs())) + x.clamp(min=0))
    if act == ACT_LRELU:
        return torch.where(x > 0, x, 0.2 * x)
    if act == ACT_RELU:
        return x.clamp(min=0)
    raise ValueError(act)


def linear(A, W, bias, dtype=torch.float64):
    """(A W^T + bias, sum |a||w| + |bias|) in dtype."""
    A, W = A.to(dtype), W.to(dtype)
    pre, mag = A @ W.T, A.abs() @ W.abs().T
    if bias is not None:
        pre, mag = pre + bias.to(dtype), mag + bias.to(dtype).abs()
    return pre, mag


def tap_gemm(A, W, bias, M, dil, dtype=torch.float64):
    """acc[m][n] = sum_tap A[m + tap dil] . W[tap][n] + bias: the dilated conv as accumulated GEMMs over rows."""
    pre = mag = 0
    for tap in range(W.shape[0]):
        p, g = linear(A[tap * dil: tap * dil + M], W[tap], None, dtype)
        pre, mag = pre + p, mag + g
    if bias is not None:
        pre, mag = pre + bias.to(dtype), mag + bias.to(dtype).abs()
    return pre, mag


def film_residual(x, v, scale, shift, rows_per_seq):
    """x + (scale[seq] + 1) v + shift[seq], seq = row // rows_per_seq (scale None: x + v); and the magnitudes of its terms."""
    if scale is None:
        return x + v, x.abs()
    seq = torch.arange(x.shape[0], device=x.device) // rows_per_seq
    y = (scale[seq] + 1.0) * v
    return x + y + shift[seq], x.abs() + y.abs() + shift[seq].abs()


def conv_skip(y, skip):
    return (skip + y) * 0.5


def restate(case, ops, mode, dtype=torch.float64):
    """{"ref": values the epilogue stores before the rounding of the store [M, N], "mag": the bound's magnitude sum [M, N] (float64),
    "pre": acc + bias}."""
    A, W = effective_operands(case, ops, mode)
    pre, mag = tap_gemm(A, W, ops["bias"], case.M, case.dil, dtype)
    mag = mag.double()
    if case.epi == EPI_FILM_RES:
        sc = ops["film_scale"].to(dtype) if case.film else None
        sh = ops["film_shift"].to(dtype) if case.film else None
        ref, extra = film_residual(ops["x"].to(dtype), pre, sc, sh, case.rows_per_seq)
        mag = mag + extra.double()
    else:
        ref = activation(pre, case.act)
        if case.skip:
            r = slice(2 * case.dil, 2 * case.dil + case.M)
            if case.split:   # the skip operand is a split row: hi + lo
                hi, lo = _split(ops["A"][r, :case.N], mode)
                skip = hi.to(dtype) + lo.to(dtype)
            else:
                skip = round_to(ops["A"][r, :case.N], mode).to(dtype)
            ref = conv_skip(ref, skip)
            mag = mag + skip.abs().double()
    return {"ref": ref, "mag": mag, "pre": pre}


def accumulation_bound(act, products, mag):
    return LIPSCHITZ[act] * 2.0 * (products + 8) * 2.0 ** -24 * mag


def bound(case, mode, ref, mag):
    """Per-element bound of the module docstring.  The store is 16-bit in a 16-bit mode unless it is the fp32 store or the fp32 stream."""
    products = case.K * (3 if case.split else 1) * case.ntaps
    act = ACT_NONE if case.epi == EPI_FILM_RES else case.act
    return accumulation_bound(act, products, mag) + u_out(case, mode) * ref.double().abs()


def u_out(case, mode):
    return 0.0 if (case.out_f32 or case.epi == EPI_FILM_RES) else U_OUT[mode]


def skinny_restate(o, act, dtype=torch.float64):
    pre, mag = linear(o["A"], o["W"], o["bias"], dtype)
    return activation(pre, act), mag.double()


def skinny_bound(K, act, mag):
    return accumulation_bound(act, K, mag)


# ----------------------------------------------------------------------------- output buffers
@dataclass
class Layout:
    """Where a case's epilogue writes inside its fp32 buffer image (element indices; guards of GUARD_ROWS rows on both sides)."""
    elems: int
    off: int
    ldo: int
    index: torch.Tensor                 # [M, N] int64: element of (m, n), `off` included
    t_seq_stride: int = 0
    split_third: int = 0
    dup_off: int = 0
    written: torch.Tensor = field(default=None)   # bool [elems]


def layout(case, mode):
    M, N = case.M, case.N
    m = torch.arange(M).unsqueeze(1)
    n = torch.arange(N).unsqueeze(0)
    seq, sm = m // case.rows_per_seq, m % case.rows_per_seq
    third = rup(N, 64) if case.split_third else 0
    tss = dup = 0
    if case.epi == EPI_FILM_RES:
        ld = N + 12                                       # ldx > N
        idx, span = m * ld + n, M * ld
    elif case.epi == EPI_STORE_T:
        ld = rup(case.rows_per_seq, 64)
        tss = (N + 1) * ld                                # one spare row between the sequences
        idx, span = seq * tss + n * ld + sm, case.nseq * tss
    else:
        ld = (3 * third if third else N) + case.ldo_extra
        idx = (m + seq * case.out_seq_pad) * ld + n
        span = (M + (case.nseq - 1) * case.out_seq_pad) * ld
        if case.dup:
            dup = span + 8 * ld
            span = dup + span
    off = GUARD_ROWS * ld
    lay = Layout(elems=off + span + GUARD_ROWS * ld, off=off, ldo=ld, index=idx + off, t_seq_stride=tss, split_third=third, dup_off=dup)
    w = torch.zeros(lay.elems, dtype=torch.bool)
    flat = lay.index.reshape(-1)
    w[flat] = True
    if third:
        w[flat + third] = True
        w[flat + 2 * third] = True
    if dup:
        w[flat + dup] = True
    lay.written = w
    return lay
