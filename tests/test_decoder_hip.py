"""Decoder layers on the MI355X (csrc/kernels_conv.h, audio2photoreal_amd/decoder.py) against the float64 restatement
(tests/decoder_restatement.py).

Gate: the normalised error of every output (max |difference| / max |value|, every element) is at most 4 x the float32 error of the
same formulas on the same inputs: for the fixture decoder the reference's own error stored in tests/golden/golden_decoder_v1.npz
(e_ref), for every other shape the restatement run in float32 against itself in float64.  The factor 4 pays for fused multiply-adds
and the kernel's order of summation (input channel, then tap).  No number is hard-coded; every measured value goes to record(...)
beside its allowance (dec_* entries).  Copies, masks' zeros and the refusals are compared exactly."""
import ctypes
import os

import numpy as np
import pytest
import torch

import decoder_restatement as R
import skinning_restatement as SR
from audio2photoreal_amd import _lib
from audio2photoreal_amd import decoder as D
from audio2photoreal_amd import skinning as SK
from audio2photoreal_amd import surface as S
from conftest import record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_decoder_v1.npz"))


@pytest.fixture(scope="module")
def fx():
    """The fixture as data, with the restatement's float64 forward (outputs and block-level intermediates) computed once."""
    f = R.make_fixture()
    f["keep"] = {}
    f["want"] = R.decoder_forward(f["params"], f["cfg"], f["assets"], f["surf"], f["motion"], f["embs"], f["face_embs"], keep=f["keep"])
    return f


@pytest.fixture(scope="module")
def decoder(fx):
    s = fx["surf"]
    surface = S.BodySurface.from_arrays(s["vi"], s["vt"], s["vti"], n_verts=s["n_verts"], v2uv=s["v2uv"], uv_size=48)
    return D.BodyDecoder.from_state_dict({"decoder." + k: v for k, v in fx["params"].items()}, fx["assets"], surface, **fx["cfg"])


def gate(name, got, want, allowance):
    """Record and assert one output: got (device tensor) against want (float64) within `allowance` (normalised), every element."""
    assert tuple(got.shape) == want.shape, (name, tuple(got.shape), want.shape)
    err = R.nerr(got.cpu().numpy(), want)
    record(name, err=err, allowance=float(allowance))
    assert np.isfinite(err) and err <= allowance, (name, err, allowance)


def own(fn):
    """(float64 result, 4 x the float32 restatement's error against it): the allowance of a shape outside the fixture."""
    want = fn(np.float64)
    return want, 4 * R.nerr(fn(np.float32), want)


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


# ------------------------------------------------------------------------------------------------ the layer
# name: (N, C_in, C_out, groups, k, source size, output size or None, bias, slope, skip, skip channels, skip size or None, mask)
LAYER_CASES = {
    "k3_3to5_24x40_untied_lrelu": (1, 3, 5, 1, 3, (24, 40), None, "untied", 0.2, None, 0, None, False),
    "k1_g2_17x33_tied_skip_tensor_mask": (3, 6, 10, 2, 1, (17, 33), None, "tied", None, "tensor", 0, None, True),
    "k3_g3_17x33_nobias_skip_conv": (3, 9, 15, 3, 3, (17, 33), None, None, 0.2, "conv", 6, None, False),
    "k3_cap_128to128_8x8": (1, 128, 128, 1, 3, (8, 8), None, "untied", 0.2, "conv", 128, None, False),
    "k3_g2_up_8to16_first_launch": (3, 8, 8, 2, 3, (8, 8), (16, 16), "untied", 0.2, None, 0, None, False),
    "k3_g2_16_skip_up_8to16_second_launch": (3, 8, 4, 2, 3, (16, 16), None, "untied", 0.2, "conv", 8, (8, 8), True),
    "k3_up_5x7_to_12x9_tied": (1, 3, 5, 1, 3, (5, 7), (12, 9), "tied", None, "conv", 2, (5, 7), False),
    "k1_up_5x7_to_12x9_skip_tensor_mask": (3, 4, 3, 1, 1, (5, 7), (12, 9), "untied", 0.1, "tensor", 0, None, True),
    "k1_1x1_plane_linear": (3, 16, 9, 1, 1, (1, 1), None, "tied", 0.2, None, 0, None, False),
    "k3_g2_1x1_plane_mask": (1, 2, 2, 2, 3, (1, 1), None, None, None, None, 0, None, True),
    "k3_1to1_up_1x1_to_9x33": (1, 1, 1, 1, 3, (1, 1), (9, 33), "untied", None, None, 0, None, False),
}


@pytest.mark.parametrize("name", list(LAYER_CASES))
def test_layer(dev, name):
    N, C_in, C_out, groups, k, src, size, bias, slope, skip, C_s, skip_size, mask = LAYER_CASES[name]
    rs = np.random.RandomState(sum(map(ord, name)))
    H, W = size or src
    a = {"x": rs.randn(N, C_in, *src), "w": rs.randn(C_out, C_in // groups, k, k) / np.sqrt(C_in // groups * k * k)}
    if bias:
        a["bias"] = rs.randn(*((C_out,) if bias == "tied" else (C_out, H, W)))
    if skip == "tensor":
        a["skip"] = rs.randn(N, C_out, H, W)
    if skip == "conv":
        a.update(skip_src=rs.randn(N, C_s, *(skip_size or (H, W))), skip_w=rs.randn(C_out, C_s // groups) / np.sqrt(C_s // groups), skip_b=rs.randn(C_out))
    if mask:
        a["mask"] = (rs.rand(H, W) < 0.7).astype(np.float32)
        a["mask"][0, 0] = 1                                                   # a 1 x 1 plane keeps a value to normalise by
    a = {key: v.astype(np.float32) for key, v in a.items()}
    want, allow = own(lambda dt: R.layer(a["x"], a["w"], a.get("bias"), groups, size, slope, a.get("skip"), a.get("skip_src"),
                                         a.get("skip_w"), a.get("skip_b"), a.get("mask"), dt))
    t = {key: up(v, dev) for key, v in a.items()}
    got = D.conv2d_ub(t["x"], t["w"], t.get("bias"), groups=groups, size=size, slope=slope, skip=t.get("skip"), skip_src=t.get("skip_src"),
                      skip_weight=t.get("skip_w"), skip_bias=t.get("skip_b"), mask=t.get("mask"))
    assert got.shape == (N, C_out, H, W) and got.dtype == torch.float32
    gate(f"dec_layer_{name}", got, want, allow)
    if mask:
        assert bool((got[:, :, t["mask"] == 0] == 0).all())
    if N > 1:                                                                 # a frame alone gives the bits it has inside the batch
        one = lambda v: v[1:2] if v is not None else None
        alone = D.conv2d_ub(t["x"][1:2], t["w"], t.get("bias"), groups=groups, size=size, slope=slope, skip=one(t.get("skip")),
                            skip_src=one(t.get("skip_src")), skip_weight=t.get("skip_w"), skip_bias=t.get("skip_b"), mask=t.get("mask"))
        assert torch.equal(alone[0], got[1])


def test_channel_window_source_and_offsets_past_2_31(dev):
    rs = np.random.RandomState(5)
    x, w, b = rs.randn(2, 7, 9, 40).astype(np.float32), (rs.randn(3, 4, 3, 3) / 6).astype(np.float32), rs.randn(3, 9, 40).astype(np.float32)
    tx = up(x, dev)
    want, allow = own(lambda dt: R.layer(x[:, 2:6], w, b, dtype=dt))
    gate("dec_layer_channel_window", D.conv2d_ub(tx[:, 2:6], up(w, dev), up(b, dev)), want, allow)
    # 9 planes of 16384 x 16384: the output holds 2.4e9 elements, so the last planes lie past 2^31; k = 1 from one channel
    # without a bias is a single product per element, which has one correct float32 value
    side = _lib.CONV_MAX_SIZE
    big = torch.randn(1, 1, side, side, device=dev)
    wk = torch.linspace(-2.0, 2.0, 9, device=dev).reshape(9, 1, 1, 1).contiguous()
    out = D.conv2d_ub(big, wk)
    assert out.numel() > 2 ** 31
    for c in (0, 7, 8):
        assert torch.equal(out[0, c], big[0, 0] * wk[c, 0, 0, 0]), c


# ------------------------------------------------------------------------------------------------ blocks of the fixture decoder
BLOCK_INPUTS = {"embs_conv_block.3": lambda k, w: k["embs_conv_block.2"], "face_embs_conv_block.2": lambda k, w: k["face_embs_conv_block.1"],
                "joint_conv_block": lambda k, w: np.concatenate([w["pose_conv"], w["embs_conv"]], 1),
                "conv_blocks.0": lambda k, w: np.concatenate([k["joint_conv_block"]] * 2, 1), "conv_blocks.1": lambda k, w: k["conv_blocks.0"]}


@pytest.mark.parametrize("name", list(BLOCK_INPUTS))
def test_blocks_against_the_fixture_intermediates(dev, gold, fx, decoder, name):
    """ConvBlock (joint_conv_block) and UpConvBlockDeep, plain and grouped, from the float64 input of the restatement's forward."""
    spec = {s[0]: s for s in [*decoder.embs_blocks, *decoder.face_blocks, decoder.joint_block, *decoder.up_blocks]}[name]
    x = BLOCK_INPUTS[name](fx["keep"], fx["want"])
    got = decoder._block(decoder._tables(dev), up(x, dev), spec)
    gate(f"dec_block_{name}", got, fx["keep"][name], 4 * float(gold[f"e_ref/block/{name}"]))


# ------------------------------------------------------------------------------------------------ seams
def test_seam_impaint_chain_and_duplicates(dev):
    rs = np.random.RandomState(7)
    H, W = 20, 37
    flat = rs.choice(H * W, size=120, replace=False)
    dst, src = flat[:60].copy(), flat[60:].copy()
    src[40:] = dst[:20]                                                       # chains: these read texels that earlier pairs write
    dst[30:36] = dst[:6]                                                      # duplicates: the later pair wins
    ij = lambda f: np.stack([f // W, f % W], 1)
    value = rs.randn(3, 5, H, W).astype(np.float32)
    seam = D.SeamSampler({"dst_ij": ij(dst), "src_ij": ij(src), "uvs": np.zeros((H, W, 2), np.float32), "weights": np.zeros((H, W), np.float32)})
    assert seam.P == 54
    t = up(value, dev)
    got = seam.impaint(t)
    assert got.data_ptr() == t.data_ptr()                                     # in place, like the reference
    want = R.impaint(value, ij(dst), ij(src))
    assert np.array_equal(got.cpu().numpy(), want)
    fv = value.reshape(3, 5, -1)
    assert np.array_equal(want.reshape(3, 5, -1)[:, :, dst[45]], fv[:, :, dst[5]])           # the original value of a written texel
    assert np.array_equal(want.reshape(3, 5, -1)[:, :, dst[2]], fv[:, :, src[32]])           # the last pair of a repeated destination
    assert seam.impaint(t[:0]).shape == (0, 5, H, W)


def test_seam_resample_with_uvs_beyond_the_border(dev):
    rs = np.random.RandomState(8)
    H, W = 19, 45
    seam = R.random_seams(rs, H, W, pairs=10, chains=2)
    seam["uvs"][::3, ::4] += rs.uniform(-0.7, 0.7, seam["uvs"][::3, ::4].shape).astype(np.float32)    # far outside [0, 1]
    seam["uvs"][0, 0], seam["uvs"][1, 1], seam["uvs"][2, 2] = (0.0, 0.0), (1.0, 1.0), (-3.0, 4.0)
    seam["weights"] = seam["weights"][:, :, None]                             # [H, W, 1] is accepted too
    assert (seam["uvs"] < 0).any() and (seam["uvs"] > 1).any()
    tex = rs.randn(11, 1, H, W).astype(np.float32)                            # 11 planes: one full group of 8 and a group of 3
    sampler = D.SeamSampler(seam)
    want, allow = own(lambda dt: R.resample(tex, seam["uvs"], seam["weights"], dt))
    t = up(tex, dev)
    got = sampler.resample(t)
    assert got.data_ptr() != t.data_ptr() and torch.equal(t.cpu(), torch.from_numpy(tex))
    gate("dec_seam_resample", got, want, allow)
    assert torch.equal(sampler.resample(t[9:10])[0], got[9])
    both, both_allow = own(lambda dt: R.resample(R.impaint(tex, seam["dst_ij"], seam["src_ij"]), seam["uvs"], seam["weights"], dt))
    gate("dec_seam_call", sampler(up(tex, dev)), both, both_allow)
    assert sampler.resample(t[:0]).shape == (0, 1, H, W)


# ------------------------------------------------------------------------------------------------ the decoder
def run(decoder, fx, dev, frames=slice(None)):
    return decoder.forward(up(fx["motion"][frames], dev), up(fx["embs"][frames], dev), up(fx["face_embs"][frames], dev))


def test_decoder_forward_on_the_fixture(dev, gold, fx, decoder):
    got = run(decoder, fx, dev)
    assert set(got) == {"geom_delta_rec", "geom_uv_delta_rec", "tex_mean_rec", "embs_conv", "pose_conv"}
    for k, v in got.items():
        gate(f"dec_forward_{k}", v, fx["want"][k], 4 * float(gold[f"e_ref/{k}"]))
    non_head = torch.from_numpy(decoder.non_head_mask).to(dev)
    assert bool((got["pose_conv"][:, :, non_head == 0] == 0).all())
    # a given embs_conv skips the embedding branch and is left as it was
    given = got["embs_conv"].clone()
    before = given.clone()
    again = decoder.forward(up(fx["motion"], dev), up(fx["embs"], dev), up(fx["face_embs"], dev), embs_conv=given)
    assert torch.equal(given, before) and again["embs_conv"].data_ptr() != given.data_ptr()
    want = R.decoder_forward(fx["params"], fx["cfg"], fx["assets"], fx["surf"], fx["motion"], fx["embs"], fx["face_embs"],
                             embs_conv=before.cpu().numpy())
    for k in ("embs_conv", "tex_mean_rec"):
        gate(f"dec_forward_given_embs_conv_{k}", again[k], want[k], 4 * float(gold[f"e_ref/{k}"]))
    with pytest.raises(D.A2PError, match=r"motion must be float32 \[N, 16\]"):
        decoder.forward(up(fx["motion"][:, :-1], dev), up(fx["embs"], dev), up(fx["face_embs"], dev))
    with pytest.raises(D.A2PError, match="must live on the MI355X"):
        decoder.forward(torch.from_numpy(fx["motion"]), up(fx["embs"], dev), up(fx["face_embs"], dev))


def test_two_runs_and_a_frame_alone_give_the_same_bits(dev, fx, decoder):
    rs = np.random.RandomState(9)
    three = {"motion": rs.randn(3, 16).astype(np.float32), "embs": rs.randn(3, 16).astype(np.float32), "face_embs": rs.randn(3, 8).astype(np.float32)}
    full, again = run(decoder, three, dev), run(decoder, three, dev)
    alone = run(decoder, three, dev, slice(1, 2))
    for k in full:
        assert torch.equal(full[k], again[k]), f"two identical runs differ in {k}"
        assert alone[k].shape[0] == 1 and torch.equal(alone[k][0], full[k][1]), f"frame 1 of {k} depends on the batch"
    empty = run(decoder, three, dev, slice(0, 0))
    assert empty["tex_mean_rec"].shape == (0, 3, 256, 256) and empty["geom_delta_rec"].shape == (0, 437, 3)


@pytest.fixture(scope="module")
def skeleton(fx):
    """A random skeleton over the fixture mesh's 437 vertices, driven by the decoder's 6 + 10 pose parameters."""
    skel = SR.make_skeleton(12, 6, 437, 4, P_pos=16, P_scale=3)
    sk = SK.BodySkeleton.from_arrays(skel["parents"], skel["pre_rotation"], skel["joint_offset"], skel["transform"], skel["transform_offsets"],
                                     16, 3, skel["rest_vertices"], skel["skin_indices"], skel["skin_weights"],
                                     template_verts=fx["surf"]["rest"], lbs_scale=np.zeros(3, np.float32), global_scaling=np.float32(10.0))
    return skel, sk


def test_decode_motion_in_chunks_of_one_frame(dev, fx, decoder, skeleton):
    _, sk = skeleton
    rs = np.random.RandomState(10)
    poses, embs, face = rs.randn(1, 3, 16) * 0.5, rs.randn(1, 3, 16), rs.randn(1, 3, 8)
    with torch.cuda.device(dev):
        whole = D.decode_motion(decoder, sk, poses, embs, face)
        assert decoder.activation_bytes_per_frame() > 1
        calls = []
        forward = decoder.forward
        decoder.forward = lambda *a, **k: (calls.append(a[0].shape[0]), forward(*a, **k))[1]
        try:
            chunked = D.decode_motion(decoder, sk, poses, embs, face, max_bytes=1)
        finally:
            del decoder.forward
    assert calls == [1, 1, 1]
    assert {k: tuple(v.shape) for k, v in whole.items()} == {"vertices": (1, 3, 437, 3), "tex_mean": (1, 3, 3, 256, 256), "geom_delta": (1, 3, 437, 3)}
    for k in whole:
        assert torch.equal(whole[k], chunked[k]), k
    frames = up(poses.reshape(3, 16), dev)
    preds = decoder.forward(frames, up(embs.reshape(3, 16), dev), up(face.reshape(3, 8), dev))
    assert torch.equal(whole["geom_delta"][0], preds["geom_delta_rec"]) and torch.equal(whole["tex_mean"][0], preds["tex_mean_rec"])
    assert torch.equal(whole["vertices"][0], sk.pose_vertices(frames, verts_unposed=preds["geom_delta_rec"]))
    with pytest.raises(D.A2PError, match=r"embs must be \[1, 3, 16\]"):
        D.decode_motion(decoder, sk, poses, embs[:, :2], face)


def test_command_line_matches_the_direct_call(dev, fx, decoder, skeleton, tmp_path):
    skel, sk = skeleton
    model, cfg = SR.as_model_dicts(skel)
    s, t = fx["surf"], torch.from_numpy
    assets = {"lbs_model_json": model, "lbs_config_dict": cfg, "lbs_template_verts": t(s["rest"]), "lbs_scale": torch.zeros(3),
              "global_scaling": torch.tensor(10.0), "topology": {"vi": t(s["vi"]), "vt": t(s["vt"]), "vti": t(s["vti"]), "v2uv": t(s["v2uv"])},
              **{k: fx["assets"][k] for k in D.ASSET_KEYS}}
    torch.save(assets, tmp_path / "static_assets.pt")
    torch.save({"decoder." + k: t(v) for k, v in fx["params"].items()}, tmp_path / "body_dec.ckpt")
    rs = np.random.RandomState(13)
    motions, embs, face = rs.randn(1, 16, 1, 4) * 0.5, rs.randn(1, 4, 16).astype(np.float32), rs.randn(1, 4, 8).astype(np.float32)
    np.save(tmp_path / "results.npy", {"motions": motions})
    np.savez(tmp_path / "embs.npz", embs=embs, face_embs=face)
    argv = ["--results", str(tmp_path / "results.npy"), "--embeddings", str(tmp_path / "embs.npz"), "--assets", str(tmp_path / "static_assets.pt"),
            "--checkpoint", str(tmp_path / "body_dec.ckpt"), "--out", str(tmp_path / "decoded.npy"), "--frames", "1:3"]
    for key, value in fx["cfg"].items():
        argv += ["--" + key.replace("_", "-"), str(value)]
    with torch.cuda.device(dev):
        assert D.main(argv) == 0
        want = D.decode_motion(decoder, sk, motions[:, :, 0, 1:3].transpose(0, 2, 1), embs[:, 1:3], face[:, 1:3])
    got = np.load(tmp_path / "decoded.npy", allow_pickle=True).item()
    assert set(got) == set(want) == {"vertices", "tex_mean", "geom_delta"}
    for k in want:
        assert got[k].dtype == np.float32 and got[k].shape[:2] == (1, 2) and np.array_equal(got[k], want[k].cpu().numpy()), k


# ------------------------------------------------------------------------------------------------ refusals of the C ABI, N = 0
def test_c_abi_refusals_and_empty_batches(dev):
    x, w = torch.randn(2, 4, 6, 6, device=dev), torch.randn(4, 4, 3, 3, device=dev)
    out = torch.zeros(2, 4, 6, 6, device=dev)

    def desc(**over):
        d = _lib.A2PConv2dDesc()
        d.x = _lib.A2PConvSource(_lib.ptr(x), 4 * 36, 4, 6, 6, 0)
        d.weight, d.out, d.N, d.C_out, d.H, d.W, d.k, d.groups = _lib.ptr(w), _lib.ptr(out), 2, 4, 6, 6, 3, 1
        for k, v in over.items():
            setattr(d, k, v)
        return d

    def call(d):
        with torch.cuda.device(dev):
            return _lib.check(_lib.load().a2p_conv2d_ub(ctypes.byref(d), _lib.current_stream(dev)), "a2p_conv2d_ub")

    assert call(desc()) == 0
    with pytest.raises(D.A2PError, match="out must not alias an input .it overlaps x."):
        call(desc(out=_lib.ptr(x)))
    with pytest.raises(D.A2PError, match="out must not alias an input .it overlaps x."):
        call(desc(out=x[1:].data_ptr()))                                      # a partial overlap, not only the same pointer
    with pytest.raises(D.A2PError, match="out must not alias an input .it overlaps weight."):
        call(desc(out=_lib.ptr(w)))
    with pytest.raises(D.A2PError, match="k=5, need 1 or 3"):
        call(desc(k=5))
    with pytest.raises(D.A2PError, match=f"C_out={_lib.CONV_MAX_CHANNELS + 1} with groups=1: need a multiple of groups with at most {_lib.CONV_MAX_CHANNELS}"):
        call(desc(C_out=_lib.CONV_MAX_CHANNELS + 1))
    with pytest.raises(D.A2PError, match=f"x.C={2 * _lib.CONV_MAX_CHANNELS + 2} with groups=2"):
        call(desc(x=_lib.A2PConvSource(_lib.ptr(x), 1 << 40, 2 * _lib.CONV_MAX_CHANNELS + 2, 6, 6, 0), groups=2))
    with pytest.raises(D.A2PError, match="bias_mode=2 needs a bias"):
        call(desc(bias_mode=_lib.CONV_BIAS_UNTIED))
    with pytest.raises(D.A2PError, match="x.frame_stride=100 is below C H W = 144"):
        call(desc(x=_lib.A2PConvSource(_lib.ptr(x), 100, 4, 6, 6, 0)))
    # N = 0 returns without a launch, through the C ABI and through the layer
    before = out.clone()
    assert call(desc(N=0)) == 0 and torch.equal(out, before)
    assert D.conv2d_ub(x[:0], w).shape == (0, 4, 6, 6)
    with pytest.raises(D.A2PError, match="weight .4, 4, 3, 3. does not fit C_in=4, groups=2"):
        D.conv2d_ub(x, w, groups=2)
    with pytest.raises(D.A2PError, match="must live on the MI355X"):
        D.conv2d_ub(x.cpu(), w)
