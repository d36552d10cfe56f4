"""Every gemm_kernel instance and epilogue, skinny_gemm_kernel and skinny_gemm_group_kernel against float64, element by element
(csrc/kernels_gemm.h through the dispatchers launch_gemm / launch_skinny / launch_skinny3 of csrc/a2p_lib.hip).

The per-operation path is what the chain, small-forward, tail and attention kernels are tied to bit for bit; these tests tie the
per-operation GEMMs themselves to a plain restatement (tests/gemm_restatement.py):
  * every written element within a bound DERIVED from fp32 accumulation and the store's rounding -- not measured;
  * every element outside the exact write set (rows >= M, columns >= N, pad rows between sequences, the padding of transposed
    sequences, 64 guard rows on both sides) bit-identical to the sentinel the buffer was filled with;
  * the instance the dispatcher chose, asserted per case.
gemm_kernel<h16_t, 4> (128 x 128 tiles of 16-bit operands) is instantiated but unreachable: launch_gemm's `small` is always true
in a 16-bit mode.  No shape here reports it, and the dispatcher's rule is left alone."""
import ctypes as C

import pytest
import torch

import gemm_restatement as R
from audio2photoreal_amd import _lib
from conftest import record

pytestmark = pytest.mark.gpu

# act_gelu_fast (the 16-bit GELU store: erf by Abramowitz-Stegun 7.1.26, v_rcp / v_exp) against erf-GELU is the one number that
# cannot be derived.  The "gelu" case measures it on every run against the float64 erf-GELU of the kernel's own fp32
# pre-activations, beyond the rounding of the 16-bit store (record "gemm_family/gelu_fast_dev/<mode>"); the gate allows twice
# GELU_FAST_DEV_MEASURED.  NOT YET MEASURED ON HARDWARE: the value stays 0.0, i.e. no allowance at all -- the fast GELU has to
# stay inside the derived bound on its own (the polynomial's 1.5e-7 on erf is ~100x below the accumulation term at K = 100).
# Whoever records a non-zero deviation writes it here; the bound must not be widened any other way.
GELU_FAST_DEV_MEASURED = 0.0
GELU_FAST_GATE = 2.0 * GELU_FAST_DEV_MEASURED

SENT_BITS = torch.tensor([R.SENTINEL], dtype=torch.float32).view(torch.int32).item()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


_CTX = {}


def ctx_for(mode):
    """A bare context of the mode (no weights: the unit entry points use its precision and scratch allocator only)."""
    if mode not in _CTX:
        lib = _lib.load(mode == "fp16")
        cfg = _lib.A2PConfig(data_format=_lib.FACE, nfeats=104, latent_dim=256, ff_size=64, num_layers=1, num_heads=4, cond_feature_dim=64,
                             max_frames=16, emb_len=16, keyframe_dim=104, keyframe_step=30,
                             precision=_lib.PREC_F32 if mode == "fp32" else _lib.PREC_BF16, max_batch=1, reserved=0)
        ctx = C.c_void_p()
        _lib.check(lib.a2p_ctx_create(C.byref(cfg), C.byref(ctx)), "a2p_ctx_create")
        _CTX[mode] = (lib, ctx)
    return _CTX[mode]


@pytest.fixture(scope="module", autouse=True)
def _destroy_contexts():
    yield
    for lib, ctx in _CTX.values():
        lib.a2p_ctx_destroy(ctx)
    _CTX.clear()


def untouched(buf, written):
    """Elements outside the write set whose bits are no longer the sentinel's."""
    bad = (buf.view(torch.int32) != SENT_BITS) & ~written
    return bad.nonzero().flatten()


def run_gemm(dev, mode, case, act=None, out_f32=None):
    """One a2p_gemm_ex launch of `case`: (whole output image on the CPU, layout, instance)."""
    lib, ctx = ctx_for(mode)
    ops, lay = R.make_operands(case), R.layout(case, mode)
    keep = {k: v.to(dev) for k, v in ops.items() if v is not None}
    buf = torch.full((lay.elems,), R.SENTINEL, device=dev)
    ran = (C.c_int32 * 3)()
    q = _lib.A2PGemmCase(A=_lib.ptr(keep["A"]), W=_lib.ptr(keep["W"]), bias=_lib.ptr(keep.get("bias")), ran_host=ran,
                         a_rows=case.a_rows, M=case.M, N=case.N, K=case.K, ntaps=case.ntaps, a_tap_rows=case.dil, epi=case.epi,
                         act=case.act if act is None else act, out_f32=case.out_f32 if out_f32 is None else out_f32,
                         rows_per_seq=case.rows_per_seq, out_seq_pad=case.out_seq_pad, split=int(case.split), split_third=lay.split_third,
                         ldo=lay.ldo, t_seq_stride=lay.t_seq_stride, dup_off=lay.dup_off)
    if case.epi == R.EPI_FILM_RES:
        buf[lay.index.to(dev)] = keep["x"]
        q.resid, q.resid_elems, q.ldx = buf.data_ptr() + 4 * lay.off, lay.elems - lay.off, lay.ldo
        if case.film:   # scale | 8 unused | shift | unused: a sequence stride larger than 2 N, everything unused is the sentinel
            N = case.N
            film = torch.full((case.nseq, 2 * N + 24), R.SENTINEL, device=dev)
            film[:, :N], film[:, N + 8: 2 * N + 8] = keep["film_scale"], keep["film_shift"]
            keep["film"] = film
            q.film, q.film_elems, q.film_seq_stride, q.film_shift_off = film.data_ptr(), film.numel(), film.shape[1], N + 8
    else:
        q.out, q.out_elems, q.out_off = buf.data_ptr(), lay.elems, lay.off
        if case.skip:
            q.skip = keep["A"].data_ptr() + 4 * 2 * case.dil * case.K
    _lib.check(lib.a2p_gemm_ex(ctx, C.byref(q), _lib.current_stream()), f"a2p_gemm_ex({case.name})")
    torch.cuda.synchronize()
    return buf.cpu(), lay, tuple(ran)


def check_gemm_case(dev, mode, case):
    """Failures of one case as strings (empty: passed); records the worst error / bound ratio and the instance."""
    fails = []
    out, lay, inst = run_gemm(dev, mode, case)
    want_inst = R.pick(mode, case.M, case.N, case.ntaps)
    if inst != want_inst:
        fails.append(f"instance {inst}, expected {want_inst}")
    if inst == (16, 4, 2):
        fails.append("gemm_kernel<h16_t, 4> ran: it is unreachable under launch_gemm's rule")
    bad = untouched(out, lay.written)
    if bad.numel():
        i = int(bad[0])
        fails.append(f"{bad.numel()} elements outside the write set changed; first at element {i} (row {i // lay.ldo - R.GUARD_ROWS}, "
                     f"column {i % lay.ldo}) = {float(out[i])!r}")
    r = R.restate(case, R.make_operands(case), mode)
    ref, bnd = r["ref"], R.bound(case, mode, r["ref"], r["mag"])
    got = out[lay.index].double()
    extra = {}
    if case.act == R.ACT_GELU and mode != "fp32" and not case.out_f32:
        # fast GELU of the 16-bit store: measure its deviation on the kernel's own pre-activations (same instance, fp32 store, no activation)
        pre_img, _, inst2 = run_gemm(dev, mode, case, act=R.ACT_NONE, out_f32=1)
        g64 = R.activation(pre_img[lay.index].double(), R.ACT_GELU)
        raw = (got - g64).abs()
        dev_fast = float((raw - R.U_OUT[mode] * g64.abs()).clamp(min=0).max())
        record(f"gemm_family/gelu_fast_dev/{mode}", beyond_store_rounding=dev_fast, with_store_rounding=float(raw.max()), gate=GELU_FAST_GATE)
        extra["gelu_fast_dev"] = dev_fast
        if inst2 != inst:
            fails.append(f"pre-activation launch took instance {inst2}")
        bnd = bnd + GELU_FAST_GATE
    err = (got - ref).abs()
    ratio = err / bnd.clamp(min=1e-300)
    worst = float(ratio.max())
    if not torch.isfinite(got).all() or worst > 1.0:
        m, n = divmod(int(torch.nan_to_num(ratio, nan=float("inf")).argmax()), case.N)
        fails.append(f"error / bound = {worst:.3g} at (m={m}, n={n}): got {float(got[m, n])!r}, reference {float(ref[m, n])!r}, "
                     f"bound {float(bnd[m, n]):.3g}; {int((ratio > 1).sum())} elements over")
    if lay.dup_off and not torch.equal(out[lay.index + lay.dup_off].view(torch.int32), out[lay.index].view(torch.int32)):
        fails.append("the dup_off copy differs from the first")
    if lay.split_third:
        u = R.U_OUT[mode]
        tiny = 2.0 ** -25 if mode == "fp16" else 0.0       # half the smallest IEEE-half subnormal: lo may be one
        lo, hi2 = out[lay.index + lay.split_third].double(), out[lay.index + 2 * lay.split_third]
        if not torch.equal(hi2.view(torch.int32), out[lay.index].view(torch.int32)):
            fails.append("split_third: the third piece differs from the first")
        # lo = T(v - hi) of the fp32 value v the epilogue held: |lo| <= u |hi| (half an ulp of hi), and hi + lo restates v to
        # u^2 |v|, so the pair must meet the reference without the store's rounding term
        if not (lo.abs() <= u * got.abs() + tiny).all():
            fails.append("split_third: a middle piece is larger than half an ulp of its first piece")
        pair = ((got + lo - ref).abs() / (bnd - u * ref.abs() + u * u * ref.abs() + tiny).clamp(min=1e-300)).max()
        extra["pair_ratio"] = float(pair)
        if not pair <= 1.0:
            fails.append(f"split_third: hi + lo misses the reference: error / bound = {float(pair):.3g}")
    record(f"gemm_family/{mode}/{case.name}", ratio=worst, instance="%d-bit/MT%d/NB%d" % inst, **extra)
    return fails


def _group(c):
    return c.name.rsplit("/", 1)[0] if "/" in c.name else c.name


# (mode, group of cases): the ring4 / ring2 groups exist in the 16-bit modes only, f32loop / f32big in fp32 only
GROUPS = [(m, g) for m in R.MODES for g in sorted({_group(c) for c in R.CASES if m in c.modes})]


@pytest.mark.parametrize("mode,group", GROUPS)
def test_gemm_cases(dev, mode, group):
    cases = [c for c in R.CASES if mode in c.modes and _group(c) == group]
    assert cases
    fails = {c.name: f for c in cases for f in [check_gemm_case(dev, mode, c)] if f}
    assert not fails, "\n".join(f"{k}: {m}" for k, v in fails.items() for m in v)


@pytest.mark.parametrize("mode", R.MODES)
def test_bad_shapes_are_refused_before_any_launch(dev, mode):
    lib, ctx = ctx_for(mode)
    case = R.BY_NAME["seqpad/f32"]
    lay = R.layout(case, mode)
    A, W = torch.zeros(case.a_rows, case.K, device=dev), torch.zeros(1, case.N, case.K, device=dev)
    buf = torch.full((lay.elems,), R.SENTINEL, device=dev)

    def call(**over):
        f = dict(A=A.data_ptr(), W=W.data_ptr(), out=buf.data_ptr(), out_elems=lay.elems, out_off=lay.off, a_rows=case.a_rows, M=case.M,
                 N=case.N, K=case.K, ntaps=1, epi=R.EPI_STORE, act=R.ACT_NONE, out_f32=1, rows_per_seq=50, out_seq_pad=24, ldo=lay.ldo)
        f.update(over)
        return lib.a2p_gemm_ex(ctx, C.byref(_lib.A2PGemmCase(**f)), _lib.current_stream())

    assert call() == 0
    buf.fill_(R.SENTINEL)
    for over in (dict(N=case.N + 2), dict(M=0), dict(out_elems=lay.off + 10), dict(out_seq_pad=10 ** 6), dict(ldo=case.N - 4), dict(a_rows=case.M - 1),
                 dict(ntaps=3, a_tap_rows=1), dict(epi=R.EPI_CONV, act=R.ACT_NONE), dict(act=R.ACT_MISH), dict(split=1, out_f32=0, split_third=100),
                 dict(dup_off=2), dict(epi=R.EPI_FILM_RES), dict(epi=R.EPI_STORE_T), dict(out_off=-4)):
        assert call(**over) == -1, over
    sk = _lib.A2PSkinnyCase(A=A.data_ptr(), W=W.data_ptr(), out=buf.data_ptr(), lda=case.K, ldw=case.K, ldo=lay.ldo, M=4, N=case.N, K=64, act=0)
    assert lib.a2p_skinny_gemm_ex(ctx, C.byref(sk), 1, _lib.current_stream()) == -1      # N = 104 is no multiple of 16
    assert lib.a2p_skinny_gemm_ex(ctx, C.byref(sk), 2, _lib.current_stream()) == -1
    del _lib._failed[:]
    torch.cuda.synchronize()
    assert not untouched(buf.cpu(), torch.zeros(lay.elems, dtype=torch.bool)).numel()


# ----------------------------------------------------------------------------- skinny GEMMs
def skinny_buffers(dev, spec, tag=""):
    """Device operands of a skinny case: A [M, lda] and out [64 + M + 64, ldo] with the sentinel in every element that is no operand."""
    M, N, K, la, lo, act, bias = spec
    o = R.make_skinny(spec, tag)
    A = torch.full((M, K + la), R.SENTINEL, device=dev)
    A[:, :K] = o["A"]
    out = torch.full((M + 2 * R.GUARD_ROWS, N + lo), R.SENTINEL, device=dev)
    keep = (A, o["W"].to(dev), None if o["bias"] is None else o["bias"].to(dev), out)
    sk = _lib.A2PSkinnyCase(A=A.data_ptr(), W=keep[1].data_ptr(), bias=_lib.ptr(keep[2]), out=out.data_ptr() + 4 * R.GUARD_ROWS * (N + lo),
                            lda=K + la, ldw=K, ldo=N + lo, M=M, N=N, K=K, act=act)
    return o, sk, keep


def check_skinny(spec, o, out, name):
    M, N, K, la, lo, act, bias = spec
    out = out.cpu()
    written = torch.zeros_like(out, dtype=torch.bool)
    written[R.GUARD_ROWS: R.GUARD_ROWS + M, :N] = True
    fails = []
    bad = untouched(out.flatten(), written.flatten())
    if bad.numel():
        i = int(bad[0])
        fails.append(f"{bad.numel()} elements outside the write set changed; first at row {i // (N + lo) - R.GUARD_ROWS}, column {i % (N + lo)}")
    ref, mag = R.skinny_restate(o, act)
    got = out[R.GUARD_ROWS: R.GUARD_ROWS + M, :N].double()
    ratio = (got - ref).abs() / R.skinny_bound(K, act, mag).clamp(min=1e-300)
    worst = float(ratio.max())
    if not torch.isfinite(got).all() or worst > 1.0:
        m, n = divmod(int(torch.nan_to_num(ratio, nan=float("inf")).argmax()), N)
        fails.append(f"error / bound = {worst:.3g} at (m={m}, n={n}): got {float(got[m, n])!r}, reference {float(ref[m, n])!r}")
    record(name, ratio=worst)
    return fails


@pytest.mark.parametrize("mode", R.MODES)
def test_skinny_cases(dev, mode):
    lib, ctx = ctx_for(mode)
    fails = {}
    for spec in R.SKINNY_CASES:
        o, sk, keep = skinny_buffers(dev, spec)
        _lib.check(lib.a2p_skinny_gemm_ex(ctx, C.byref(sk), 1, _lib.current_stream()), f"a2p_skinny_gemm_ex{spec[:3]}")
        f = check_skinny(spec, o, keep[3], "gemm_family/%s/skinny/%dx%dx%d" % ((mode,) + spec[:3]))
        if f:
            fails[spec] = f
    assert not fails, "\n".join(f"{k}: {m}" for k, v in fails.items() for m in v)


@pytest.mark.parametrize("group", sorted(R.SKINNY_GROUPS))
@pytest.mark.parametrize("mode", R.MODES)
def test_skinny_group_of_three_is_bit_identical_to_single_launches(dev, mode, group):
    lib, ctx = ctx_for(mode)
    specs = R.SKINNY_GROUPS[group]
    one, three = [skinny_buffers(dev, s, group) for s in specs], [skinny_buffers(dev, s, group) for s in specs]
    for o, sk, keep in one:
        _lib.check(lib.a2p_skinny_gemm_ex(ctx, C.byref(sk), 1, _lib.current_stream()), "a2p_skinny_gemm_ex")
    arr = (_lib.A2PSkinnyCase * 3)(*[b[1] for b in three])
    _lib.check(lib.a2p_skinny_gemm_ex(ctx, arr, 3, _lib.current_stream()), "a2p_skinny_gemm_ex x 3")
    fails = []
    for spec, a, b in zip(specs, one, three):
        if not torch.equal(a[2][3].view(torch.int32), b[2][3].view(torch.int32)):
            fails.append(f"{spec[:3]}: the grouped launch differs from the single launch")
        fails += check_skinny(spec, b[0], b[2][3], "gemm_family/%s/skinny_%s/%dx%dx%d" % ((mode, group) + spec[:3]))
    assert not fails, "\n".join(fails)
