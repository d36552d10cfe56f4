"""CPU-side checks of the encode path (no GPU): the numpy restatement (tests/encoder_restatement.py) against torch's own layers in
float64, the float32 order-restatement of the linear kernel against float64, host folding and masks of audio2photoreal_amd/
encoder.py, the loaders' refusals, and header / struct / binding agreement."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import encoder_restatement as R
import skinning_restatement as SR
from audio2photoreal_amd import _lib
from audio2photoreal_amd import encoder as E
from audio2photoreal_amd import surface as S
from audio2photoreal_amd._lib import A2PError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy


@pytest.fixture(scope="module")
def fx():
    return R.make_fixture()


def prefixed(params, prefix):
    return {prefix + k: v for k, v in params.items()}


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("shape", [(2, 3, 5, (7, 9)), (1, 4, 2, (8, 8)), (3, 1, 1, (1, 1))], ids=["odd", "even", "one"])
def test_down3_against_torch_in_float64(shape):
    N, ci, co, (Hs, Ws) = shape
    rs = np.random.RandomState(ci)
    H, W = (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1
    h, x, w2, b2 = rs.randn(N, ci, Hs, Ws), rs.randn(N, ci, Hs, Ws), rs.randn(co, ci, 3, 3), rs.randn(co, H, W)
    wr, br = rs.randn(co, ci), rs.randn(co)
    want = F.leaky_relu(F.conv2d(T(h), T(w2), stride=2, padding=1) + T(b2)[None], 0.2) + F.conv2d(T(x), T(wr)[:, :, None, None], T(br), stride=2)
    assert np.abs(R.down3(h, x, w2, b2, wr, br) - want.numpy()).max() < 1e-12
    assert np.abs(R.down3(h, x, w2, b2, wr, br, resize_offset=1) - want.numpy()).max() > 1e-3 or min(Hs, Ws) == 1


@pytest.mark.parametrize("sizes", [((12, 10), (5, 7)), ((1024 // 64, 16), (8, 8)), ((5, 6), (11, 9))], ids=["mixed", "half", "up"])
def test_tex_cond_against_torch_in_float64(sizes):
    (Hs, Ws), (H, W) = sizes
    rs = np.random.RandomState(H)
    raw, bias, mask = rs.randn(2, 3, Hs, Ws), rs.randn(3, Hs, Ws), rs.rand(H, W)
    tex = 255 * (T(raw) + T(bias)[None] + 0.5)
    want = (F.interpolate(tex, (H, W), mode="bilinear", align_corners=False) / 255.0 - 0.5) * T(mask)
    assert np.abs(R.tex_cond(raw, bias, mask) - want.numpy()).max() < 1e-12
    for wiring in ("corners", "no_half", "no_mask"):
        assert np.abs(R.tex_cond(raw, bias, mask, wiring=wiring) - want.numpy()).max() > 1e-3, wiring


def test_unpose_inverts_pose_and_matches_torch_inverse(fx):
    """LBSModule.unpose restated: torch's 4 x 4 inverse of the blended matrix, as the reference calls it, gives the same vertices;
    and unpose(pose(x)) = x.  The fixture's blends are well conditioned (|det| in [0.5, 2] x scale^3 = 1)."""
    sk, g = fx["skel"], fx["global_scaling"]
    det = np.abs(R.blend_determinants(sk, fx["poses"], fx["scales"]))
    assert det.min() >= 0.5 and det.max() <= 2.0
    posed = SR.pose_vertices(sk, fx["poses"], fx["scales"], fx["displacement"], fx["template"], g)
    got = R.unpose(sk, fx["poses"], fx["scales"], posed, fx["template"], g)
    assert np.abs(got - fx["displacement"]).max() < 1e-12
    M = R.blended(sk, SR.transforms(sk, fx["poses"], fx["scales"]))
    M4 = np.concatenate([M, np.broadcast_to(np.array([0, 0, 0, 1.0]), M.shape[:2] + (1, 4))], 2)
    v4 = np.concatenate([posed / g, np.ones(posed.shape[:2] + (1,))], 2)
    want = torch.linalg.inv(T(M4)).matmul(T(v4)[..., None])[..., :3, 0].numpy() - fx["template"]
    assert np.abs(got - want).max() < 1e-12


def test_linear_rule_in_float32_is_close_to_float64_and_beats_one_chain():
    """The documented order (slices of 256 terms, then the slices in order) restated in float32: its error over 21918 terms stays
    near the rounding of the result, below a single serial chain's."""
    rs = np.random.RandomState(0)
    x, w, b = rs.randn(2, 21918).astype(np.float32), (rs.randn(6, 21918) / 148).astype(np.float32), rs.randn(6).astype(np.float32)
    want = R.linear(x, w, b, 0.2)
    e_rule = R.nerr(R.linear_rule32(x, w, b, 0.2), want)
    chain = np.zeros((2, 6), np.float32)
    for i in range(x.shape[1]):
        chain = R._fma32(x[:, i:i + 1], w[None, :, i], chain)
    e_chain = R.nerr(np.where(chain + b >= 0, chain + b, np.float32(0.2) * (chain + b)), want)
    assert e_rule < 2e-6 and e_rule <= e_chain, (e_rule, e_chain)
    assert E.linear_slices(21918) == 86 and E.linear_slices(256) == 1 and E.linear_slices(257) == 2 and E.linear_slices(1) == 1


def test_networks_against_torch_layers_in_float64(fx):
    """FaceDecoderFrontal, FaceEncoder and ConvDownBlock composed from torch's F.linear / conv2d / conv_transpose2d / interpolate
    in float64 give what the restatement gives."""
    p = {k: T(np.asarray(v, np.float64)) for k, v in fx["face_dec"].items()}
    fold = lambda q, n: q[f"{n}.weight_v"] * (q[f"{n}.weight_g"] / q[f"{n}.weight_v"].norm())
    codes = T(fx["codes"].astype(np.float64))
    enc = F.leaky_relu(F.linear(codes, fold(p, "encmod.0"), p["encmod.0.bias"]), 0.2)
    geom = F.linear(enc, fold(p, "geommod.0"), p["geommod.0.bias"])
    view = F.leaky_relu(F.linear(T(fx["assets"]["face_frontal_view"].astype(np.float64))[None].expand(2, -1), fold(p, "viewmod.0"), p["viewmod.0.bias"]), 0.2)
    y = F.leaky_relu(F.linear(torch.cat([enc, view], 1), fold(p, "texmod2.0"), p["texmod2.0.bias"]), 0.2).view(2, 6, 4, 4)
    layers = R.face_layers(R.FACE_DEC)
    for i, n in enumerate(layers):
        y = F.conv_transpose2d(y, fold(p, n), None, 2, 1) + p[f"{n}.bias"][None]
        if i + 1 < len(layers):
            y = F.leaky_relu(y, 0.2)
    got = R.face_decoder(fx["face_dec"], layers, fx["assets"]["face_frontal_view"], fx["codes"])
    assert np.abs(got["face_geom"].reshape(2, -1) - geom.numpy()).max() < 1e-11
    assert np.abs(got["face_tex_raw"] - y.numpy()).max() < 1e-11
    assert np.abs(got["face_tex"] - (255 * (y + p["bias"][None] + 0.5)).numpy()).max() < 1e-9

    q = {k: T(np.asarray(v, np.float64)) for k, v in fx["face_enc"].items()}
    mask = F.interpolate(T(fx["assets"]["mugsy_face_mask"][..., 0].astype(np.float64))[None, None], (16, 16), mode="bilinear", align_corners=True)
    x = (F.interpolate(255 * (y + p["bias"][None] + 0.5), (16, 16), mode="bilinear", align_corners=False) / 255.0 - 0.5) * mask
    for n in R.face_blocks(R.FACE_ENC):
        skip = F.conv2d(x, fold(q, f"{n}.conv_resize"), q[f"{n}.conv_resize.bias"], stride=2)
        h = F.leaky_relu(F.conv2d(x, fold(q, f"{n}.conv1"), padding=1) + q[f"{n}.conv1.bias"][None], 0.2)
        x = F.leaky_relu(F.conv2d(h, fold(q, f"{n}.conv2"), stride=2, padding=1) + q[f"{n}.conv2.bias"][None], 0.2) + skip
    g = F.leaky_relu(F.linear(geom, fold(q, "geommod.0"), q["geommod.0.bias"]), 0.2)
    j = F.leaky_relu(F.linear(torch.cat([x.reshape(2, -1), g], 1), fold(q, "jointmod.0"), q["jointmod.0.bias"]), 0.2)
    mu, logvar = F.linear(j, fold(q, "mu"), q["mu.bias"]), 0.1 * F.linear(j, fold(q, "logvar"), q["logvar.bias"])
    got = R.face_encoder(fx["face_enc"], R.face_blocks(R.FACE_ENC), mask[0, 0].numpy(), geom.numpy(), y.numpy(), fx["face_dec"]["bias"])
    assert np.abs(got["face_embs_mu"] - mu.numpy()).max() < 1e-10 and np.abs(got["face_embs_logvar"] - logvar.numpy()).max() < 1e-10


# ------------------------------------------------------------------------------------------------ host preparation
def test_folding_masks_and_ladders(fx):
    dec = E.FaceDecoder.from_state_dict(prefixed(fx["face_dec"], "decoder_face."), fx["assets"])
    assert (dec.n_latent, dec.n_hidden, dec.V, dec.n_view, dec.c0, dec.s0, dec.tex_channels, dec.tex_size) == (12, 10, 7, 3, 6, 4, 3, 32)
    assert [l[1:] for l in dec.layers] == [(6, 5, 4), (5, 4, 8), (4, 3, 16)]
    for name in ("encmod.0", "geommod.0", "texmod2.0", "texmod.2"):            # float64 fold, norm over the whole tensor, rounded once
        v, g = fx["face_dec"][f"{name}.weight_v"].astype(np.float64), fx["face_dec"][f"{name}.weight_g"].astype(np.float64)
        assert np.array_equal(dec.params[f"{name}.weight"], (v * (g / np.sqrt((v * v).sum()))).astype(np.float32)), name
    assert fx["face_dec"]["texmod.2.weight_g"].shape == (1, 4, 1, 1)           # the transposed layers carry g on axis 1
    fused = dict(fx["face_dec"])
    fused["encmod.0.weight"] = dec.params["encmod.0.weight"]
    del fused["encmod.0.weight_v"], fused["encmod.0.weight_g"]
    again = E.FaceDecoder.from_state_dict(prefixed(fused, "decoder_face."), fx["assets"])
    assert np.array_equal(again.params["encmod.0.weight"], dec.params["encmod.0.weight"])

    enc = E.FaceEncoder.from_state_dict(prefixed(fx["face_enc"], "encoder_face."), fx["assets"], uv_size=16)
    assert enc.blocks == [("conv_blocks.0", 3, 4, 16), ("conv_blocks.1", 4, 6, 8)]
    assert (enc.n_tex_enc, enc.n_geom_enc, enc.n_vert_in, enc.n_joint, enc.n_embs) == (96, 9, 21, 11, 5)
    assert enc.params["conv_blocks.0.conv_resize.weight"].shape == (4, 3)
    want = F.interpolate(T(fx["assets"]["mugsy_face_mask"][..., 0].astype(np.float64))[None, None], (16, 16), mode="bilinear", align_corners=True)
    assert np.array_equal(enc.params["tex_cond_mask"], want[0, 0].numpy().astype(np.float32))

    s = fx["surf"]
    surface = S.BodySurface.from_arrays(s["vi"], s["vt"], s["vti"], n_verts=s["n_verts"], v2uv=s["v2uv"], uv_size=24)
    body = E.BodyEncoder.from_state_dict(prefixed(fx["body_enc"], "encoder."), fx["assets"], surface, uv_size=16)
    assert body.blocks == [("verts_conv", 3, 8, 16), ("joint_conv_blocks.0", 8, 6, 8)] and (body.n_flat, body.n_embs) == (96, 7)
    want = F.interpolate(1 - T(fx["assets"]["face_mask"].astype(np.float64))[None, None], (16, 16), mode="bilinear") != 0
    assert np.array_equal(body.params["mask"], want[0, 0].numpy().astype(np.float32)) and 0 < body.params["mask"].mean() <= 1
    assert E.activation_bytes_per_frame(dec, enc, body, type("Sk", (), {"J": 6, "V": surface.V})) > 4 * 3 * 32 * 32


def test_loader_refusals(fx):
    sd = prefixed(fx["face_dec"], "decoder_face.")
    with pytest.raises(ValueError, match=r"`geommod.0.bias` has shape \[21\]; the configuration expects \[24\]"):
        E.FaceDecoder.from_state_dict({**sd, "decoder_face.geommod.0.weight_v": np.ones((24, 10), np.float32),
                                       "decoder_face.geommod.0.weight_g": np.ones((24, 1), np.float32)}, fx["assets"])
    with pytest.raises(ValueError, match="three per vertex"):
        E.FaceDecoder.from_state_dict({**sd, "decoder_face.geommod.0.weight_v": np.ones((22, 10), np.float32)}, fx["assets"])
    with pytest.raises(ValueError, match="texmod.2.bias"):
        E.FaceDecoder.from_state_dict({k: v for k, v in sd.items() if k != "decoder_face.texmod.2.bias"}, fx["assets"])
    with pytest.raises(ValueError, match="face_frontal_view"):
        E.FaceDecoder.from_state_dict(sd, {})
    with pytest.raises(ValueError, match="encmod.0"):
        E.FaceDecoder.from_state_dict({}, fx["assets"])
    se = prefixed(fx["face_enc"], "encoder_face.")
    with pytest.raises(ValueError, match=r"`conv_blocks.0.conv1.bias` has shape \[3, 16, 16\]; the configuration expects \[3, 32, 32\]"):
        E.FaceEncoder.from_state_dict(se, fx["assets"], uv_size=32)
    with pytest.raises(ValueError, match="uv_size=1 is outside"):
        E.FaceEncoder.from_state_dict(se, fx["assets"], uv_size=1)
    with pytest.raises(ValueError, match="jointmod.0.weight_v"):
        E.FaceEncoder.from_state_dict({**se, "encoder_face.jointmod.0.weight_v": np.ones((11, 104), np.float32)}, fx["assets"], uv_size=16)
    with pytest.raises(ValueError, match="mugsy_face_mask"):
        E.FaceEncoder.from_state_dict(se, {"mugsy_face_mask": np.zeros((4, 4), np.float32)}, uv_size=16)
    with pytest.raises(ValueError, match="not finite"):
        E.FaceEncoder.from_state_dict({**se, "encoder_face.mu.bias": np.full(5, np.nan, np.float32)}, fx["assets"], uv_size=16)
    with pytest.raises(TypeError, match="from_state_dict"):
        E.BodyEncoder()
    with pytest.raises(A2PError, match="MI355X"):
        E.linear(torch.zeros(2, 3), torch.zeros(4, 3))


# ------------------------------------------------------------------------------------------------ header and binding
def test_header_struct_and_binding_agree():
    header = open(os.path.join(ROOT, "include", "a2p_hip.h")).read()
    kernels = open(os.path.join(ROOT, "audio2photoreal_amd", "csrc", "kernels_encode.h")).read()
    assert re.search(r"#define A2P_LINEAR_KSLICE (\d+)", header).group(1) == str(_lib.LINEAR_KSLICE) == str(R.KSLICE)
    assert re.search(r"#define LIN_KSLICE (\d+)", kernels).group(1) == str(_lib.LINEAR_KSLICE)
    body = re.search(r"typedef struct a2p_down3_desc \{(.*?)\} a2p_down3_desc;", header, re.S).group(1)
    fields = [piece.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for piece in decl.split(",")]
    assert fields == [n for n, _ in _lib.A2PDown3Desc._fields_]
    new = {"a2p_linear_f32": 14, "a2p_conv2d_down3_ub": 2, "a2p_unskin_vertices": 14, "a2p_face_tex_cond": 11}
    assert set(new) <= set(_lib.EXPORTS)
    lib = _lib.load()
    for name, n_args in new.items():
        decl = re.search(rf"int {name}\((.*?)\);", header, re.S).group(1)
        assert len(decl.split(",")) == n_args == len(getattr(lib, name).argtypes), name
    tex = re.search(r"typedef struct a2p_tex_conv_desc \{(.*?)\} a2p_tex_conv_desc;", header, re.S).group(1)
    assert [p.split()[-1].lstrip("*") for d in tex.split(";") if d.strip() for p in d.split(",")] == [n for n, _ in _lib.A2PTexConvDesc._fields_]


# ------------------------------------------------------------------------------------------------ the command line
def test_command_line_argument_errors(tmp_path):
    base = ["--assets", "a.pt", "--checkpoint", "c.ckpt", "--out", str(tmp_path / "o.npy")]
    with pytest.raises(SystemExit):                                            # one source of cameras
        E.main(["--results", "r.npy", *base, "--eye", "0", "0", "1", "--defaults", "d.pth"])
    with pytest.raises(SystemExit):
        E.main(base)                                                           # --results is required
    with pytest.raises(A2PError, match="--target goes with --eye"):
        E.main(["--results", "r.npy", *base, "--defaults", "d.pth", "--target", "0", "0", "0"])
    np.save(tmp_path / "r.npy", {"pose": np.zeros((1, 4, 104), np.float32)})
    with pytest.raises(A2PError, match="holds no `face`"):
        E.main(["--results", str(tmp_path / "r.npy"), *base])
    np.save(tmp_path / "r2.npy", {"pose": np.zeros((1, 4, 104), np.float32), "face": np.zeros((1, 5, 256), np.float32)})
    with pytest.raises(A2PError, match="same R and T"):
        E.main(["--results", str(tmp_path / "r2.npy"), *base])


# ------------------------------------------------------------------------------------------------ the reference's own modules
@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_encoder_v1.npz"))


@pytest.fixture(scope="module")
def ref_fx():
    return R.make_reference_fixture()


def test_the_generated_fixture_is_the_one_the_reference_ran_on(gold, ref_fx):
    for net in ("face_dec", "face_enc", "body_enc"):
        stored = {k.split("/", 2)[2]: float(gold[k]) for k in gold.files if k.startswith(f"fingerprint/{net}/")}
        assert R.fingerprint(ref_fx[net]) == stored, net
    for k in gold.files:
        if k.startswith("input/"):
            assert float(np.asarray(ref_fx[k[6:]], np.float64).sum()) == float(gold[k]), k
    for k in ("codes", "poses", "scales"):
        assert np.array_equal(gold[k], ref_fx[k]), k
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_encoder_v1.npz")) < 1 << 20


def test_restatement_reproduces_the_reference(gold, ref_fx):
    """float64 restatement against the reference's float32 FaceDecoderFrontal, FaceEncoder, Encoder and LBSModule.unpose (at their
    fixed sizes, 1024 and 512): on the stored elements the difference, normalised by the output's largest value, stays inside
    e_ref, which was measured over every element."""
    rows = slice(int(gold["rows_start"]), None, int(gold["rows_step"]))
    want = R.reference_forward({**ref_fx, "posed32": gold["posed32"]})
    assert {k[4:] for k in gold.files if k.startswith("ref/")} == set(want)
    for name, w in want.items():
        ref, e_ref = gold[f"ref/{name}"], float(gold[f"e_ref/{name}"])
        sub = w[..., rows, :] if w.ndim == 4 and w.shape[-2] >= 128 else w
        assert 0 < e_ref < 1e-4, name                                          # a float32 rounding error, not a formula error
        assert ref.shape == sub.shape and ref.dtype == np.float32, name
        err = float(np.abs(ref.astype(np.float64) - sub).max() / np.abs(w).max())
        assert err <= e_ref, (name, err, e_ref)
    assert np.array_equal(want["face_enc/face_embs"], want["face_enc/face_embs_mu"])        # eval mode
    posed = SR.pose_vertices(ref_fx["skel"], ref_fx["poses"], ref_fx["scales"], ref_fx["displacement"], ref_fx["template"], ref_fx["global_scaling"])
    assert R.nerr(gold["posed32"], posed) < 1e-5                               # the stored vertices are the posed displacement
