"""The GEMM family's float64 restatement, its case list and its derived error bound, checked without a GPU
(tests/gemm_restatement.py; the kernels themselves: tests/test_gemm_family_hip.py)."""
import pytest
import torch
import torch.nn.functional as F

import gemm_restatement as R
from audio2photoreal_amd import _lib


def _rand(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


# ----------------------------------------------------------------------------- restatement == torch.nn.functional
def test_linear_matches_functional():
    A, W, b = _rand(37, 100, seed=1), _rand(52, 100, seed=2), _rand(52, seed=3)
    pre, mag = R.linear(A, W, b)
    assert (pre - F.linear(A, W, b)).abs().max() < 1e-12
    assert (mag - (F.linear(A.abs(), W.abs()) + b.abs())).abs().max() < 1e-12
    pre, _ = R.linear(A, W, None)
    assert (pre - F.linear(A, W)).abs().max() < 1e-12


@pytest.mark.parametrize("dil", [1, 2, 3])
@pytest.mark.parametrize("ci,co", [(104, 104), (104, 256), (256, 104)])
def test_tap_gemm_matches_dilated_conv1d_leaky_relu_and_averaged_skip(dil, ci, co):
    """One layer of post_pose_layers: y = leaky_relu(conv1d(x, dilation), 0.2); (x[:, :, -len(y):] + y) / 2 when ci == co."""
    L = 50 + 24
    x, w, b = _rand(1, ci, L, seed=10 + dil), _rand(co, ci, 3, seed=20 + dil) / (3 * ci) ** 0.5, _rand(co, seed=30)
    y = F.leaky_relu(F.conv1d(x, w, b, dilation=dil), negative_slope=0.2)
    want = (x[:, :, -y.shape[-1]:] + y) / 2.0 if ci == co else y
    rows = x[0].T.contiguous()                                     # [L, ci]: one row per frame
    M = L - 2 * dil
    pre, _ = R.tap_gemm(rows, w.permute(2, 0, 1).contiguous(), b, M, dil)      # W[tap][co][ci]
    got = R.activation(pre, R.ACT_LRELU)
    if ci == co:
        got = R.conv_skip(got, rows[2 * dil: 2 * dil + M, :co])
    assert (got - want[0].T).abs().max() < 1e-12


@pytest.mark.parametrize("rps", [7, 50, 64])
def test_film_residual_matches_featurewise_affine(rps):
    """FiLM of the decoder layer: x + ((scale + 1) * v + shift), scale / shift per sequence."""
    nseq, d = 3, 36
    x, v = _rand(nseq, rps, d, seed=4), _rand(nseq, rps, d, seed=5)
    sc, sh = _rand(nseq, 1, d, seed=6), _rand(nseq, 1, d, seed=7)
    want = x + ((sc + 1.0) * v + sh)
    got, mag = R.film_residual(x.reshape(-1, d), v.reshape(-1, d), sc[:, 0], sh[:, 0], rps)
    assert (got - want.reshape(-1, d)).abs().max() < 1e-12
    assert (mag - (x.abs() + ((sc + 1) * v).abs() + sh.abs().expand_as(x)).reshape(-1, d)).abs().max() < 1e-12
    got, mag = R.film_residual(x.reshape(-1, d), v.reshape(-1, d), None, None, rps)
    assert torch.equal(got, (x + v).reshape(-1, d))


def test_activations_match_functional():
    x = torch.linspace(-30, 30, 4001, dtype=torch.float64)
    assert (R.activation(x, R.ACT_GELU) - F.gelu(x)).abs().max() < 1e-12
    assert (R.activation(x, R.ACT_MISH) - F.mish(x)).abs().max() < 1e-12
    assert (R.activation(x, R.ACT_LRELU) - F.leaky_relu(x, 0.2)).abs().max() < 1e-12
    assert (R.activation(x, R.ACT_RELU) - F.relu(x)).abs().max() < 1e-12


def test_lipschitz_constants_cover_the_activations():
    x = torch.linspace(-12, 12, 200001, dtype=torch.float64)
    for act, L in R.LIPSCHITZ.items():
        y = R.activation(x, act)
        assert ((y[1:] - y[:-1]) / (x[1:] - x[:-1])).abs().max() <= L, act


def test_split_pieces_restate_split3():
    """hi = T(v), lo = T(v - hi): the pair carries v to u^2, and [hi|lo|hi] x [hi|hi|lo] drops only lo * lo."""
    v = torch.randn(1000, generator=torch.Generator().manual_seed(8))
    for mode, u in (("fp16", 2.0 ** -11), ("bf16", 2.0 ** -8)):
        hi, lo = R._split(v, mode)
        assert ((hi.double() + lo.double() - v.double()).abs() <= u * u * v.abs().double() + 2.0 ** -25).all()
    c = R.BY_NAME["conv/x3/skip_d1"]
    ops = R.make_operands(c)
    A, W = R.effective_operands(c, ops, "bf16")
    assert A.shape[-1] == 3 * c.K and W.shape[-1] == 3 * c.K
    ah, al = R._split(ops["A"], "bf16")
    wh, wl = R._split(ops["W"], "bf16")
    want = (ah.double() @ wh[0].double().T) + (al.double() @ wh[0].double().T) + (ah.double() @ wl[0].double().T)
    assert (A.double() @ W[0].double().T - want).abs().max() < 1e-12


# ----------------------------------------------------------------------------- the case list
# the instances the list must reach under gemm_pick's rule (csrc/a2p_lib.hip), each by shape alone: mode -> (bits, MT, NB) -> a case that takes it
EXPECTED_INSTANCES = {
    "fp32": {(32, 2, 2): "store/m129n104", (32, 4, 2): "f32big/k32"},
    "fp16": {(16, 2, 4): "ring4/k3", (16, 2, 2): "ring2/wide_k1", (16, 1, 2): "conv/plain/128_d1"},
    "bf16": {(16, 2, 4): "ring4/k3", (16, 2, 2): "ring2/wide_k2", (16, 1, 2): "conv/plain/skip_d1"},
}
EXPECTED_OF_CASE = {
    "store/m1n4": {"fp32": (32, 2, 2), "fp16": (16, 2, 4), "bf16": (16, 2, 4)},
    "ring4/k1": {"fp16": (16, 2, 4), "bf16": (16, 2, 4)},
    "ring4/k8pad": {"fp16": (16, 2, 4), "bf16": (16, 2, 4)},
    "ring2/k1": {"fp16": (16, 2, 2), "bf16": (16, 2, 2)},
    "ring2/k5": {"fp16": (16, 2, 2), "bf16": (16, 2, 2)},
    "ring2/wide_k1": {"fp16": (16, 2, 2), "bf16": (16, 2, 2)},
    "f32loop/k1": {"fp32": (32, 2, 2)},
    "f32big/k32": {"fp32": (32, 4, 2)},
    "f32big/k64": {"fp32": (32, 4, 2)},
    "conv/plain/skip_d2": {"fp32": (32, 2, 2), "fp16": (16, 1, 2), "bf16": (16, 1, 2)},
    "conv/x3/128_d3": {"fp16": (16, 1, 2), "bf16": (16, 1, 2)},
    "conv/x3/down_d1": {"fp16": (16, 1, 2), "bf16": (16, 1, 2)},
    "conv/plain/up_d1": {"fp32": (32, 2, 2), "fp16": (16, 2, 2), "bf16": (16, 2, 2)},     # N = 256: two column tiles, taps: the 2-deep ring
    "film/rps7": {"fp32": (32, 2, 2), "fp16": (16, 2, 4), "bf16": (16, 2, 4)},
}


def test_case_list_reaches_every_instance():
    for mode, table in EXPECTED_INSTANCES.items():
        reached = {R.pick(mode, c.M, c.N, c.ntaps) for c in R.CASES if mode in c.modes}
        assert reached == set(table), (mode, reached)
        for inst, name in table.items():
            c = R.BY_NAME[name]
            assert mode in c.modes and R.pick(mode, c.M, c.N, c.ntaps) == inst, (mode, name)
    for name, per_mode in EXPECTED_OF_CASE.items():
        c = R.BY_NAME[name]
        assert set(per_mode) == set(c.modes), name
        for mode, inst in per_mode.items():
            assert R.pick(mode, c.M, c.N, c.ntaps) == inst, (name, mode)
    # <h16_t, 4> (128 x 128 tiles of 16-bit operands) is instantiated but no shape selects it: `small` is true in every 16-bit mode
    assert all(R.pick(m, c.M, c.N, c.ntaps) != (16, 4, 2) for c in R.CASES for m in R.B16)


def test_case_list_covers_the_issue_edges():
    cs = R.CASES
    assert {1, 15, 17, 31, 33, 63, 65, 127, 129} <= {c.M for c in cs}
    assert {4, 60, 104, 128, 132, 260} <= {c.N for c in cs}
    for mode in R.B16:   # k-tiles 1, 2, 3, 4, 5, 8 on the 4-deep ring, on the 2-deep ring
        for inst in ((16, 2, 4), (16, 2, 2)):
            tiles = {R.rup(c.K, 64) // 64 for c in cs if mode in c.modes and c.ntaps == 1 and R.pick(mode, c.M, c.N, 1) == inst}
            assert {1, 2, 3, 4, 5, 8} <= tiles, (mode, inst, tiles)
    tiles = {R.rup(c.K, 32) // 32 for c in cs if "fp32" in c.modes and c.ntaps == 1}
    assert {1, 2, 3, 4, 5, 8} <= tiles
    assert {c.rows_per_seq for c in cs if c.epi == R.EPI_FILM_RES and c.film} == {7, 50, 64}
    assert {c.rows_per_seq for c in cs if c.epi == R.EPI_FILM_RES and not c.film} == {7, 50, 64}
    assert {20, 64, 77} <= {c.rows_per_seq for c in cs if c.epi == R.EPI_STORE_T}
    assert any(c.out_seq_pad == 24 and c.epi == R.EPI_STORE for c in cs) and any(c.dup for c in cs)
    assert {(c.act, c.out_f32) for c in cs if c.epi == R.EPI_STORE} >= {(R.ACT_GELU, 0), (R.ACT_RELU, 0), (R.ACT_RELU, 1)}
    conv = [c for c in cs if c.epi == R.EPI_CONV]
    assert all(c.ntaps == 3 and c.M == 2 * (50 + 24) and c.act == R.ACT_LRELU for c in conv)
    for split in (False, True):
        for dil in (1, 2, 3):
            assert {(c.K, c.N, c.skip) for c in conv if c.split == split and c.dil == dil} == {(104, 104, True), (128, 128, True), (104, 256, False),
                                                                                              (256, 104, False)}
    assert all(c.split_third for c in conv if c.split)
    assert {s[0] for s in R.SKINNY_CASES} == {1, 2, 15, 16, 17, 48, 63, 64, 65, 130}
    assert {s[1] for s in R.SKINNY_CASES} == {16, 48, 1536} and {s[2] for s in R.SKINNY_CASES} == {64, 128, 2048}
    assert {s[5] for s in R.SKINNY_CASES} == {R.ACT_NONE, R.ACT_MISH} and {s[6] for s in R.SKINNY_CASES} == {True, False}
    assert any(s[3] for s in R.SKINNY_CASES) and any(s[4] for s in R.SKINNY_CASES)
    for name, grp in R.SKINNY_GROUPS.items():
        assert len({s[:3] for s in grp}) == 3
        assert (max(s[0] for s in grp) > 64) == (name == "fallback")


def test_layouts_keep_guards_and_padding_out_of_the_write_set():
    for c in R.CASES:
        lay = R.layout(c, c.modes[-1])
        w = lay.written
        g = R.GUARD_ROWS * lay.ldo
        assert not w[:g].any() and not w[-g:].any(), c.name
        pieces = (3 if c.split_third else 1) * (2 if c.dup else 1)
        assert int(w.sum()) == c.M * c.N * pieces, c.name          # no two elements share an address
        assert lay.off % 4 == 0 and lay.ldo % 4 == 0 and int(lay.index.max()) < lay.elems - g


def test_struct_layouts_match_the_header():
    import ctypes as C
    assert C.sizeof(_lib.A2PGemmCase) == 8 * 8 + 10 * 8 + 14 * 4
    assert C.sizeof(_lib.A2PSkinnyCase) == 4 * 8 + 3 * 8 + 4 * 4
    assert (_lib.EPI_STORE, _lib.EPI_STORE_T, _lib.EPI_FILM_RES, _lib.EPI_CONV) == (R.EPI_STORE, R.EPI_STORE_T, R.EPI_FILM_RES, R.EPI_CONV)
    assert (_lib.ACT_NONE, _lib.ACT_GELU, _lib.ACT_MISH, _lib.ACT_LRELU, _lib.ACT_RELU) == (R.ACT_NONE, R.ACT_GELU, R.ACT_MISH, R.ACT_LRELU, R.ACT_RELU)


# ----------------------------------------------------------------------------- the bound holds for a correct fp32 computation
@pytest.mark.parametrize("mode", R.MODES)
def test_float32_restatement_stays_inside_the_bound(mode):
    """float64 against the same restatement computed in float32 on the CPU: a bound that a correct fp32 computation breaks is a
    wrong bound, not a kernel bug."""
    worst = 0.0
    for c in R.CASES:
        if mode not in c.modes:
            continue
        ops = R.make_operands(c)
        r64, r32 = R.restate(c, ops, mode), R.restate(c, ops, mode, torch.float32)
        b = R.bound(c, mode, r64["ref"], r64["mag"]) - R.u_out(c, mode) * r64["ref"].abs()     # no store rounding here
        ratio = float(((r32["ref"].double() - r64["ref"]).abs() / b.clamp(min=1e-300)).max())
        assert ratio <= 1.0, (c.name, mode, ratio)
        worst = max(worst, ratio)
    assert worst > 0.0


def test_float32_skinny_restatement_stays_inside_the_bound():
    for spec in R.SKINNY_CASES + [s for g in R.SKINNY_GROUPS.values() for s in g]:
        o = R.make_skinny(spec)
        r64, mag = R.skinny_restate(o, spec[5])
        r32, _ = R.skinny_restate(o, spec[5], torch.float32)
        ratio = float(((r32.double() - r64).abs() / R.skinny_bound(spec[2], spec[5], mag).clamp(min=1e-300)).max())
        assert ratio <= 1.0, (spec, ratio)
