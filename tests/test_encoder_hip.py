"""Encode layers and networks on the MI355X (csrc/kernels_encode.h, audio2photoreal_amd/encoder.py, BodySkeleton.unpose_vertices)
against the float64 restatement (tests/encoder_restatement.py).

Gate: the normalised error of every output (max |difference| / max |value|, every element) is at most 4 x max(e, 2^-24).  e is,
for the linear kernel, the error of its documented summation order restated in float32 on the same data (e_rule);
for the networks at the reference's sizes the error of the reference's own float32 modules stored in tests/golden/
golden_encoder_v1.npz (e_ref); for everything else the restatement run in float32 against itself in float64 (the second half of a
ConvDownBlock in the order its kernel documents).  All come from the CPU, never from the kernel.  The factor 4 pays
for fused multiply-adds and the kernel's order of summation; the floor 2^-24 is one float32 rounding of an output of magnitude 1.
Every measured value goes to record("enc_...") beside its allowance.  Tap tables, bit checks and refusals are compared exactly."""
import ctypes
import os

import numpy as np
import pytest
import torch

import encoder_restatement as R
import skinning_restatement as SR
import texture_restatement as TR
from audio2photoreal_amd import _lib
from audio2photoreal_amd import encoder as E
from audio2photoreal_amd import skinning as SK
from audio2photoreal_amd import surface as S
from audio2photoreal_amd._lib import A2PError
from conftest import record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def fx():
    return R.make_fixture()


def up(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


def gate(name, got, want, e):
    """Record and assert one output: got (device tensor) against want (float64) within 4 max(e, 2^-24), every element."""
    assert tuple(got.shape) == want.shape, (name, tuple(got.shape), want.shape)
    err, allowance = R.nerr(got.cpu().numpy(), want), 4 * max(float(e), FLOOR)
    record(name, err=err, allowance=allowance)
    assert np.isfinite(err) and err <= allowance, (name, err, allowance)


def own(fn):
    """(float64 result, the float32 restatement's error against it)."""
    want = fn(np.float64)
    return want, R.nerr(fn(np.float32), want)


# ------------------------------------------------------------------------------------------------ the linear kernel
LINEAR_CASES = [(1, 1, 1), (3, 70, 17), (65, 257, 33), (2, 21918, 256), (2, 256, 21918)]


@pytest.fixture(scope="module")
def linear_data():
    """Per case: x, w, bias (float32), shared by the variants."""
    out = {}
    for N, I, O in LINEAR_CASES:
        rs = np.random.RandomState(N + I + O)
        out[(N, I, O)] = (rs.randn(N, I).astype(np.float32), (rs.randn(O, I) / np.sqrt(I)).astype(np.float32), rs.randn(O).astype(np.float32))
    return out


@pytest.mark.parametrize("variant", ["plain_dense", "bias_lrelu_strided"])
@pytest.mark.parametrize("case", LINEAR_CASES, ids=lambda c: "x".join(map(str, c)))
def test_linear_against_float64_within_its_rules_error(dev, linear_data, case, variant):
    N, I, O = case
    x, w, b = linear_data[case]
    full = variant == "bias_lrelu_strided"
    bias, slope = (b, 0.2) if full else (None, None)
    want = R.linear(x, w, bias, slope)
    e_rule = R.nerr(R.linear_rule32(x, w, bias, slope), want)
    tx = up(x, dev)
    if full:                                                                   # rows of x and out inside wider matrices
        wide = torch.full((N, I + 3), float("nan"), device=dev)
        wide[:, 2:2 + I] = tx
        outw = torch.full((N, O + 5), -7.0, device=dev)
        got = E.linear(wide[:, 2:2 + I], up(w, dev), up(bias, dev), slope=slope, out=outw[:, 1:1 + O])
        assert got.data_ptr() == outw[:, 1:].data_ptr()
        assert bool((outw[:, :1] == -7).all()) and bool((outw[:, 1 + O:] == -7).all())          # nothing outside the window
    else:
        got = E.linear(tx, up(w, dev))
    gate(f"enc_linear_{N}x{I}x{O}_{variant}", got, want, e_rule)


def test_linear_bits_depend_on_neither_rows_nor_alignment(dev, linear_data):
    """A row computed alone, among 3 and as row 64 of 65 (a second row block) has the same bits; so has a weight matrix that starts 4
    and 8 bytes off a 16-byte boundary (the narrower loads); two runs agree."""
    for case in [(65, 257, 33), (2, 21918, 256)]:
        x, w, b = linear_data[case]
        tx, tw, tb = up(x, dev), up(w, dev), up(b, dev)
        ref = E.linear(tx, tw, tb, slope=0.2)
        assert torch.equal(E.linear(tx, tw, tb, slope=0.2), ref)
        last = x.shape[0] - 1
        assert torch.equal(E.linear(tx[last:], tw, tb, slope=0.2), ref[last:])
        assert torch.equal(E.linear(tx[:1], tw, tb, slope=0.2), ref[:1])
        for off in (1, 2):
            buf = torch.empty(w.size + 4, device=dev)
            shifted = buf[off:off + w.size].view(w.shape)
            shifted.copy_(tw)
            assert shifted.data_ptr() % 16 == 4 * off
            assert torch.equal(E.linear(tx, shifted, tb, slope=0.2), ref), (case, off)


# ------------------------------------------------------------------------------------------------ the tap tables, exactly
@pytest.mark.parametrize("size", [4, 5])
def test_down3_tap_table(dev, size):
    """One channel, zero biases, slope 1: a single non-zero element of h at (i, j) gives out[y][x] = w2[i - 2 y + 1][j - 2 x + 1] h
    where that tap exists, else 0; a single non-zero element of x gives wr x at (i / 2, j / 2) when i and j are even, else 0."""
    rs = np.random.RandomState(size)
    w2, wr = rs.randn(1, 1, 3, 3).astype(np.float32), rs.randn(1, 1).astype(np.float32)
    n, o = size * size, (size - 1) // 2 + 1
    h, want_h, want_x = np.zeros((n, 1, size, size), np.float32), np.zeros((n, 1, o, o), np.float32), np.zeros((n, 1, o, o), np.float32)
    for f in range(n):
        i, j = divmod(f, size)
        h[f, 0, i, j] = np.float32(1.5 + f)
        for y in range(o):
            for x in range(o):
                ky, kx = i - 2 * y + 1, j - 2 * x + 1
                if 0 <= ky < 3 and 0 <= kx < 3:
                    want_h[f, 0, y, x] = w2[0, 0, ky, kx] * h[f, 0, i, j]
                if (i, j) == (2 * y, 2 * x):
                    want_x[f, 0, y, x] = wr[0, 0] * h[f, 0, i, j]
    zero, b2 = up(np.zeros_like(h), dev), up(np.zeros((1, o, o)), dev)
    assert torch.equal(E.conv2d_down3_ub(up(h, dev), zero, up(w2, dev), b2, up(np.zeros_like(wr), dev), slope=1.0).cpu(), torch.from_numpy(want_h))
    assert torch.equal(E.conv2d_down3_ub(zero, up(h, dev), up(np.zeros_like(w2), dev), b2, up(wr, dev), slope=1.0).cpu(), torch.from_numpy(want_x))


@pytest.mark.parametrize("sizes", [((8, 8), (4, 4)), ((4, 6), (8, 12)), ((7, 5), (5, 3))], ids=["8to4", "4x6to8x12", "7x5to5x3"])
def test_face_tex_cond_tap_table(dev, sizes):
    """bias = -0.5 makes every texel but one exactly 0 before the resize (raw 0) and the one 255 a: with mask 1 the output is
    ly lx 255 a / 255 - 0.5 on the taps of a2p_resize_bilinear's float32 rule and exactly -0.5 elsewhere."""
    (Hs, Ws), (H, W) = sizes
    f32 = np.float32
    y0, y1, l0y, l1y = TR.resize_axis(Hs, H, f32)
    x0, x1, l0x, l1x = TR.resize_axis(Ws, W, f32)
    n = Hs * Ws
    raw, want = np.zeros((n, 1, Hs, Ws), f32), np.zeros((n, 1, H, W), f32)
    for f in range(n):
        i, j = divmod(f, Ws)
        raw[f, 0, i, j] = f32(1.0 + 0.25 * (f % 5))
        src = f32(255) * f32(f32(raw[f, 0] + f32(-0.5)) + f32(0.5))
        top = (l0x * src[y0][:, x0]).astype(f32) + (l1x * src[y0][:, x1]).astype(f32)
        bot = (l0x * src[y1][:, x0]).astype(f32) + (l1x * src[y1][:, x1]).astype(f32)
        r = ((l0y[:, None] * top).astype(f32) + (l1y[:, None] * bot).astype(f32)).astype(f32)
        want[f, 0] = (r / f32(255)).astype(f32) - f32(0.5)
    got = E.face_tex_cond(up(raw, dev), up(np.full((1, Hs, Ws), -0.5), dev), up(np.ones((H, W)), dev)).cpu().numpy()
    assert np.array_equal(got != f32(-0.5), want != f32(-0.5))                 # the support: which texels a tap reaches
    assert np.array_equal(got, want)


# ------------------------------------------------------------------------------------------------ the layers against float64
# name: (N, C_in, C_out, source size).  Outputs up to 16 x 16 take the 8 x 8 tile with four channel groups, larger ones 8 x 32.
DOWN3_CASES = {
    "3to5_6x10": (1, 3, 5, (6, 10)),
    "odd_5x7": (3, 2, 3, (5, 7)),
    "13to9_4x4_staging_remainder": (1, 13, 9, (4, 4)),
    "2to3_35x130_crosses_large_tiles": (2, 2, 3, (35, 130)),
    "9to33_10x12_two_chunks_small": (1, 9, 33, (10, 12)),
    "2to2_32x32_last_small": (1, 2, 2, (32, 32)),
    "2to9_34x33_first_large": (1, 2, 9, (34, 33)),
    "1to1_1x1_smallest": (3, 1, 1, (1, 1)),
}


@pytest.mark.parametrize("name", list(DOWN3_CASES))
def test_down3_against_float64(dev, name):
    N, ci, co, (Hs, Ws) = DOWN3_CASES[name]
    rs = np.random.RandomState(len(name))
    H, W = (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1
    both = rs.randn(N, 2 * ci + 1, Hs, Ws).astype(np.float32)                  # h and x as channel windows of one tensor
    h, x = both[:, :ci], both[:, ci + 1:]
    w2, wr = (rs.randn(co, ci, 3, 3) / 3).astype(np.float32), rs.randn(co, ci).astype(np.float32)
    b2, br = rs.randn(co, H, W).astype(np.float32), rs.randn(co).astype(np.float32)
    want, e = own(lambda dt: R.down3(h, x, w2, b2, wr, br, 0.2, dt))
    tb = up(both, dev)
    got = E.conv2d_down3_ub(tb[:, :ci], tb[:, ci + 1:], up(w2, dev), up(b2, dev), up(wr, dev), up(br, dev), slope=0.2)
    gate(f"enc_down3_{name}", got, want, e)
    if N > 1:                                                                  # a frame alone has the same bits
        assert torch.equal(E.conv2d_down3_ub(tb[1:2, :ci], tb[1:2, ci + 1:], up(w2, dev), up(b2, dev), up(wr, dev), up(br, dev), slope=0.2), got[1:2])


@pytest.mark.parametrize("sizes", [((20, 12), (10, 6)), ((9, 7), (16, 5)), ((33, 40), (17, 21))], ids=["half", "mixed", "odd"])
def test_face_tex_cond_against_float64(dev, sizes):
    (Hs, Ws), (H, W) = sizes
    rs = np.random.RandomState(Hs)
    raw, bias, mask = rs.randn(3, 2, Hs, Ws).astype(np.float32) * 0.3, rs.randn(2, Hs, Ws).astype(np.float32) * 0.1, rs.rand(H, W).astype(np.float32)
    want, e = own(lambda dt: R.tex_cond(raw, bias, mask, dt))
    got = E.face_tex_cond(up(raw, dev), up(bias, dev), up(mask, dev))
    gate(f"enc_tex_cond_{Hs}x{Ws}_to_{H}x{W}", got, want, e)
    assert torch.equal(E.face_tex_cond(up(raw[2:], dev), up(bias, dev), up(mask, dev)), got[2:])


# ------------------------------------------------------------------------------------------------ the networks on the fixture
def prefixed(params, prefix):
    return {prefix + k: v for k, v in params.items()}


@pytest.fixture(scope="module")
def nets(fx, dev):
    s = fx["surf"]
    surface = S.BodySurface.from_arrays(s["vi"], s["vt"], s["vti"], n_verts=s["n_verts"], v2uv=s["v2uv"], uv_size=R.BODY_ENC["surface_uv"])
    sk = fx["skel"]
    skeleton = SK.BodySkeleton.from_arrays(sk["parents"], sk["pre_rotation"], sk["joint_offset"], sk["transform"], sk["transform_offsets"],
                                           16, 3, sk["rest_vertices"], sk["skin_indices"], sk["skin_weights"], template_verts=fx["template"],
                                           lbs_scale=fx["scales"][0], global_scaling=fx["global_scaling"])
    return {"face_dec": E.FaceDecoder.from_state_dict(prefixed(fx["face_dec"], "decoder_face."), fx["assets"]),
            "face_enc": E.FaceEncoder.from_state_dict(prefixed(fx["face_enc"], "encoder_face."), fx["assets"], uv_size=R.FACE_ENC["uv_size"]),
            "body_enc": E.BodyEncoder.from_state_dict(prefixed(fx["body_enc"], "encoder."), fx["assets"], surface, uv_size=R.BODY_ENC["uv_size"]),
            "surface": surface, "skeleton": skeleton}


@pytest.fixture(scope="module")
def ref(fx, nets, dev):
    """The float64 and float32 restatements of every stage on the fixture, computed once: {stage: (want, {output: e})}.  The UV
    images are the product surface's own (their parity is test_surface_hip.py's subject)."""
    a = fx["assets"]
    with torch.cuda.device(dev):
        nets["surface"]._images(dev)
    index_image, bary_image = nets["surface"].index_image.cpu().numpy(), nets["surface"].bary_image.cpu().numpy()
    face_mask = R.resize_corners(a["mugsy_face_mask"][..., 0], (R.FACE_ENC["uv_size"],) * 2)
    body_mask = (TR.resize(1.0 - a["face_mask"].astype(np.float64), (R.BODY_ENC["uv_size"],) * 2) != 0).astype(np.float64)
    out = {}

    def stage(name, fn):
        want, low = fn(np.float64), fn(np.float32)
        out[name] = (want, {k: R.nerr(low[k], want[k]) for k in want})

    stage("face_dec", lambda dt: R.face_decoder(fx["face_dec"], R.face_layers(R.FACE_DEC), a["face_frontal_view"], fx["codes"], dt))
    dec = out["face_dec"][0]
    geom32, raw32 = dec["face_geom"].astype(np.float32), dec["face_tex_raw"].astype(np.float32)
    out["face_enc_args"] = (face_mask, geom32, raw32)
    stage("face_enc", lambda dt: R.face_encoder(fx["face_enc"], R.face_blocks(R.FACE_ENC), face_mask, geom32, raw32, fx["face_dec"]["bias"], dtype=dt))
    stage("body_enc", lambda dt: R.body_encoder(fx["body_enc"], R.body_blocks(R.BODY_ENC), body_mask, index_image, bary_image,
                                               R.BODY_ENC["uv_size"], fx["displacement"], dtype=dt))
    sk, g = fx["skel"], fx["global_scaling"]
    posed32 = SR.pose_vertices(sk, fx["poses"], fx["scales"], fx["displacement"], fx["template"], g).astype(np.float32)
    out["posed32"] = posed32
    stage("unpose", lambda dt: {"verts_unposed": R.unpose(sk, fx["poses"], fx["scales"], posed32, fx["template"], g, dt)})
    low = R.unpose(sk, fx["poses"], fx["scales"], SR.pose_vertices(sk, fx["poses"], fx["scales"], fx["displacement"], fx["template"], g, np.float32),
                   fx["template"], g, np.float32)
    out["round_trip_e"] = R.nerr(low, fx["displacement"].astype(np.float64))
    return out


def test_face_decoder_on_the_fixture(dev, fx, nets, ref):
    want, e = ref["face_dec"]
    got = nets["face_dec"].forward(up(fx["codes"], dev), return_tex=True)
    assert set(got) == {"face_geom", "face_tex_raw", "face_tex"}
    for k in want:
        gate(f"enc_face_decoder_{k}", got[k], want[k], e[k])
    assert "face_tex" not in nets["face_dec"].forward(up(fx["codes"], dev))


def test_face_encoder_on_the_fixture(dev, fx, nets, ref):
    want, e = ref["face_enc"]
    _, geom32, raw32 = ref["face_enc_args"]
    got = nets["face_enc"].forward(up(geom32, dev), up(raw32, dev), nets["face_dec"].bias(dev))
    for k in want:
        gate(f"enc_face_encoder_{k}", got[k], want[k], e[k])
    assert torch.equal(got["face_embs"], got["face_embs_mu"]) and got["face_embs"].data_ptr() != got["face_embs_mu"].data_ptr()


def test_body_encoder_on_the_fixture(dev, fx, nets, ref):
    want, e = ref["body_enc"]
    got = nets["body_enc"].forward(up(fx["displacement"], dev))
    for k in want:
        gate(f"enc_body_encoder_{k}", got[k], want[k], e[k])


def test_unpose_vertices_on_the_fixture_and_round_trip(dev, fx, nets, ref):
    """Against the float64 LU inverse at 4 x the float32 LU's own error; and unpose_vertices(pose_vertices(x)) returns x within 4 x
    what the float32 restatement of the same round trip loses.  The fixture's blends are well conditioned: |det| in [0.5, 2]."""
    det = np.abs(R.blend_determinants(fx["skel"], fx["poses"], fx["scales"]))
    assert det.min() >= 0.5 and det.max() <= 2.0, (det.min(), det.max())
    want, e = ref["unpose"]
    sk, poses = nets["skeleton"], up(fx["poses"], dev)
    got = sk.unpose_vertices(poses, up(ref["posed32"], dev))
    gate("enc_unpose_vertices", got, want["verts_unposed"], e["verts_unposed"])
    x = up(fx["displacement"], dev)
    gate("enc_unpose_round_trip", sk.unpose_vertices(poses, sk.pose_vertices(poses, verts_unposed=x)), fx["displacement"].astype(np.float64),
         ref["round_trip_e"])


def test_miswired_restatements_break_a_gate(fx, ref):
    """The gates are not vacuous: each of these miswirings of the float64 restatement misses the allowance of at least one
    output that the correctly wired restatement defines."""
    mask, geom32, raw32 = ref["face_enc_args"]
    want, e = ref["face_enc"]
    for wiring in ("corners", "no_half", "no_mask", "swap", "resize_odd"):
        bad = R.face_encoder(fx["face_enc"], R.face_blocks(R.FACE_ENC), mask, geom32, raw32, fx["face_dec"]["bias"], wiring=wiring)
        broken = [k for k in want if R.nerr(bad[k], want[k]) > 4 * max(e[k], FLOOR)]
        assert broken, wiring
    want, e = ref["unpose"]
    bad = R.unpose(fx["skel"], fx["poses"], fx["scales"], ref["posed32"], fx["template"], fx["global_scaling"], subtract=False)
    assert R.nerr(bad, want["verts_unposed"]) > 4 * max(e["verts_unposed"], FLOOR)


# ------------------------------------------------------------------------------------------------ the reference's own modules
@pytest.fixture(scope="module")
def gold_ref():
    """The golden file of the reference's classes at their fixed sizes (face texture 1024, both encoders 512), the fixture it was
    made from and the float64 restatement of every stored output over every element, computed once (about 20 s on the CPU)."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "golden_encoder_v1.npz"))
    fx = {**R.make_reference_fixture(), "posed32": gold["posed32"]}
    return gold, fx, R.reference_forward(fx)


def test_networks_at_the_references_sizes_within_four_times_its_own_error(dev, gold_ref):
    """Every output of FaceDecoder, FaceEncoder, BodyEncoder and unpose_vertices, every element, against float64 at 4 max(e_ref,
    2^-24): e_ref is the error of the reference's own float32 modules on this fixture (tests/golden/make_golden_encoder.py)."""
    gold, fx, want = gold_ref
    a = fx["assets"]
    s, sk = fx["surf"], fx["skel"]
    surface = S.BodySurface.from_arrays(s["vi"], s["vt"], s["vti"], n_verts=s["n_verts"], v2uv=s["v2uv"],
                                        uv_size=R.REF_BODY_ENC["surface_uv"]).with_images(fx["index_image"], fx["bary_image"])
    skeleton = SK.BodySkeleton.from_arrays(sk["parents"], sk["pre_rotation"], sk["joint_offset"], sk["transform"], sk["transform_offsets"],
                                           104, 12, sk["rest_vertices"], sk["skin_indices"], sk["skin_weights"], template_verts=fx["template"],
                                           lbs_scale=fx["scales"][0], global_scaling=fx["global_scaling"])
    fdec = E.FaceDecoder.from_state_dict(prefixed(fx["face_dec"], "decoder_face."), a)
    fenc = E.FaceEncoder.from_state_dict(prefixed(fx["face_enc"], "encoder_face."), a)
    benc = E.BodyEncoder.from_state_dict(prefixed(fx["body_enc"], "encoder."), a, surface)
    assert (fdec.tex_size, len(fdec.layers), fenc.uv_size, len(fenc.blocks), benc.uv_size, len(benc.blocks)) == (1024, 8, 512, 7, 512, 7)
    e = lambda k: float(gold[f"e_ref/{k}"])
    with torch.cuda.device(dev):
        got = {f"face_dec/{k}": v for k, v in fdec.forward(up(fx["codes"], dev), return_tex=True).items()}
        geom32, raw32 = want["face_dec/face_geom"].astype(np.float32), want["face_dec/face_tex_raw"].astype(np.float32)
        got.update({f"face_enc/{k}": v for k, v in fenc.forward(up(geom32, dev), up(raw32, dev), fdec.bias(dev)).items()})
        got.update({f"body_enc/{k}": v for k, v in benc.forward(up(fx["displacement"], dev)).items()})
        got["unpose/verts_unposed"] = skeleton.unpose_vertices(up(fx["poses"], dev), up(fx["posed32"], dev))
    assert set(got) == set(want)
    for k in sorted(want):
        gate("enc_ref_" + k.replace("/", "_"), got[k], want[k], e(k))


# ------------------------------------------------------------------------------------------------ bit checks
def test_one_frame_and_three_frames_give_the_same_bits(dev, fx, nets):
    rs = np.random.RandomState(5)
    codes = up(rs.randn(3, R.FACE_DEC["n_latent"]), dev)
    dec = nets["face_dec"].forward(codes)
    one = nets["face_dec"].forward(codes[1:2])
    for k in dec:
        assert torch.equal(one[k], dec[k][1:2]), k
    bias = nets["face_dec"].bias(dev)
    enc = nets["face_enc"].forward(dec["face_geom"], dec["face_tex_raw"], bias)
    one = nets["face_enc"].forward(dec["face_geom"][1:2], dec["face_tex_raw"][1:2], bias)
    for k in enc:
        assert torch.equal(one[k], enc[k][1:2]), k
    verts = up(0.05 * rs.randn(3, nets["skeleton"].V, 3), dev)
    body = nets["body_enc"].forward(verts)
    one = nets["body_enc"].forward(verts[1:2])
    for k in body:
        assert torch.equal(one[k], body[k][1:2]), k
    poses = up(rs.randn(3, 16) * 0.3, dev)
    posed = nets["skeleton"].pose_vertices(poses, verts_unposed=verts)
    assert torch.equal(nets["skeleton"].unpose_vertices(poses[1:2], posed[1:2]), nets["skeleton"].unpose_vertices(poses, posed)[1:2])


def test_encode_motion_chunkings_agree_and_rest_is_recorded(dev, fx, nets):
    """[B, T, P] poses: two chunkings give the same bits; the hand-composed per-frame chain gives them too; body_embs="rest"
    differs from "per_frame" by what the encoder makes of unpose(pose(template)) - template: recorded, not gated (nobody has
    measured it)."""
    rs = np.random.RandomState(6)
    poses, codes = up(rs.randn(1, 3, 16) * 0.3, dev), up(rs.randn(1, 3, R.FACE_DEC["n_latent"]), dev)
    args = (nets["face_dec"], nets["face_enc"], nets["body_enc"], nets["skeleton"], poses, codes)
    whole = E.encode_motion(*args)
    assert whole["embs"].shape == (1, 3, R.BODY_ENC["n_embs"]) and whole["face_embs"].shape == (1, 3, R.FACE_ENC["n_embs"])
    single = E.encode_motion(*args, max_bytes=1)
    for k in whole:
        assert torch.equal(single[k], whole[k]), k
    sk = nets["skeleton"]
    face = nets["face_dec"].forward(codes[0])
    by_hand = nets["face_enc"].forward(face["face_geom"], face["face_tex_raw"], nets["face_dec"].bias(dev))["face_embs"]
    assert torch.equal(by_hand, whole["face_embs"][0])
    assert torch.equal(nets["body_enc"].forward(sk.unpose_vertices(poses[0], sk.pose_vertices(poses[0])))["embs"], whole["embs"][0])
    geom = sk.pose_vertices(poses[0], verts_unposed=up(0.05 * rs.randn(3, sk.V, 3), dev))
    with_geom = E.encode_motion(*args, geom=geom[None])
    assert torch.equal(with_geom["face_embs"], whole["face_embs"]) and not torch.equal(with_geom["embs"], whole["embs"])
    rest = E.encode_motion(*args, body_embs="rest")
    assert torch.equal(rest["face_embs"], whole["face_embs"])
    diff = float((rest["embs"] - whole["embs"]).abs().max())
    record("enc_body_embs_rest_vs_per_frame", max_abs_diff=diff, max_abs_value=float(whole["embs"].abs().max()))
    assert np.isfinite(diff)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals(dev, fx, nets):
    lib = _lib.load()
    x, w = torch.randn(2, 8, device=dev), torch.randn(8, 8, device=dev)
    stream = _lib.current_stream(dev)
    args = lambda out, scratch=None, n=0: (_lib.ptr(x), 8, _lib.ptr(w), None, 2, 8, 8, 0, 0.0, _lib.ptr(out), 8, _lib.ptr(scratch), n, stream)
    assert lib.a2p_linear_f32(*args(x)) == -1 and b"alias" in lib.a2p_last_error()                           # A2P_ERR_ARG
    assert lib.a2p_linear_f32(*args(w[1:3])) == -1 and b"weight" in lib.a2p_last_error()
    wide_x, wide_w = torch.randn(2, 300, device=dev), torch.randn(8, 300, device=dev)
    rc = lib.a2p_linear_f32(_lib.ptr(wide_x), 300, _lib.ptr(wide_w), None, 2, 300, 8, 0, 0.0, _lib.ptr(torch.empty(2, 8, device=dev)), 8, None, 0, stream)
    assert rc == -1 and b"scratch" in lib.a2p_last_error()                                                   # two slices need scratch
    assert lib.a2p_linear_f32(_lib.ptr(x), 8, _lib.ptr(w), None, 0, 8, 8, 0, 0.0, _lib.ptr(x), 8, None, 0, stream) == 0    # N = 0: no launch
    small = torch.zeros(4, device=dev)
    rc = lib.a2p_face_tex_cond(_lib.ptr(small), _lib.ptr(small), _lib.ptr(small), 1, _lib.CONV_MAX_CHANNELS + 1, 1, 1, 1, 1, _lib.ptr(x), stream)
    assert rc == -1 and b"C=" in lib.a2p_last_error()
    rc = lib.a2p_face_tex_cond(_lib.ptr(small), _lib.ptr(small), _lib.ptr(small), 1, 1, 2, 2, 1, 1, _lib.ptr(small), stream)
    assert rc == -1 and b"alias" in lib.a2p_last_error()
    d = _lib.A2PDown3Desc()
    t = torch.zeros(1, 1, 2, 2, device=dev)
    src = _lib.A2PConvSource(_lib.ptr(t), 4, 1, 2, 2, 0)
    d.h, d.x, d.w2, d.b2, d.wr, d.out, d.N, d.C_out = src, src, _lib.ptr(small), _lib.ptr(small), _lib.ptr(small), _lib.ptr(t), 1, 1
    assert lib.a2p_conv2d_down3_ub(ctypes.byref(d), stream) == -1 and b"alias" in lib.a2p_last_error()
    d.out, d.C_out = _lib.ptr(x), _lib.CONV_MAX_CHANNELS + 1
    assert lib.a2p_conv2d_down3_ub(ctypes.byref(d), stream) == -1 and b"C_out" in lib.a2p_last_error()
    sk = nets["skeleton"]
    v = torch.zeros(1, sk.V, 3, device=dev)
    mats = sk.transforms(up(fx["poses"][:1], dev))
    t_ = sk._tables(dev)
    rc = lib.a2p_unskin_vertices(_lib.ptr(mats), 1, sk.J, _lib.ptr(v), _lib.ptr(t_["base"]), _lib.ptr(t_["idx"]), _lib.ptr(t_["w"]), sk.V, sk.K,
                                 1.0, 1.0, 1.0, _lib.ptr(v), stream)
    assert rc == -1 and b"alias" in lib.a2p_last_error()

    with pytest.raises(A2PError, match="MI355X"):
        E.linear(torch.zeros(2, 8), w)
    with pytest.raises(A2PError, match="float32"):
        E.linear(x.double(), w)
    with pytest.raises(A2PError, match="weight"):
        E.linear(x, torch.randn(8, 7, device=dev))
    with pytest.raises(A2PError, match="face_codes"):
        nets["face_dec"].forward(torch.zeros(2, R.FACE_DEC["n_latent"] + 1, device=dev))
    with pytest.raises(A2PError, match="verts"):
        sk.unpose_vertices(up(fx["poses"], dev), torch.zeros(2, sk.V, 3, device=dev, dtype=torch.float64))
    with pytest.raises(A2PError, match="body_embs"):
        E.encode_motion(nets["face_dec"], nets["face_enc"], nets["body_enc"], sk, up(fx["poses"], dev), up(fx["codes"], dev), body_embs="mean")

    skel = dict(fx["skel"])
    weights = skel["skin_weights"].copy()
    weights[3] = 0                                                             # vertex 3 is bound to nothing: its blend is the zero matrix
    singular = SK.BodySkeleton.from_arrays(skel["parents"], skel["pre_rotation"], skel["joint_offset"], skel["transform"], skel["transform_offsets"],
                                           16, 3, skel["rest_vertices"], skel["skin_indices"], weights, lbs_scale=fx["scales"][0])
    with pytest.raises(A2PError, match="frame 0, vertex 3"):
        singular.unpose_vertices(up(fx["poses"], dev), torch.ones(2, sk.V, 3, device=dev))
