"""Texture layers on the MI355X (csrc/kernels_texture.h, audio2photoreal_amd/texture.py) against the float64 restatement
(tests/texture_restatement.py).

Gate: the normalised error of every output (max |difference| / max |value|, every element) is at most 4 x max(e, 2^-24).  e is, for
the fixture networks, the reference's own float32 error stored in tests/golden/golden_texture_v1.npz (e_ref); for every other shape
the restatement run in float32 against itself in float64.  The factor 4 pays for fused multiply-adds and the kernel's order of
summation; the floor 2^-24 is one float32 rounding of an output of magnitude 1, without which a saturated sigmoid or a clamped
display value could make e vanish by luck.  No other tolerance is written down; every measured value goes to record("tex_...")
beside its allowance.  The tap tables, copies and refusals are compared exactly."""
import ctypes
import os

import numpy as np
import pytest
import torch

import decoder_restatement as DR
import skinning_restatement as SR
import texture_restatement as R
from audio2photoreal_amd import _lib
from audio2photoreal_amd import decoder as D
from audio2photoreal_amd import render as RD
from audio2photoreal_amd import skinning as SK
from audio2photoreal_amd import surface as S
from audio2photoreal_amd import texture as T
from conftest import record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLOOR = 2.0 ** -24


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_texture_v1.npz"))


@pytest.fixture(scope="module")
def fx():
    return R.make_fixture()


def gate(name, got, want, e):
    """Record and assert one output: got (device tensor) against want (float64) within 4 max(e, 2^-24), every element."""
    assert tuple(got.shape) == want.shape, (name, tuple(got.shape), want.shape)
    err, allowance = R.nerr(got.cpu().numpy(), want), 4 * max(float(e), FLOOR)
    record(name, err=err, allowance=allowance)
    assert np.isfinite(err) and err <= allowance, (name, err, allowance)


def own(fn):
    """(float64 result, the float32 restatement's error against it): e of a shape outside the fixture."""
    want = fn(np.float64)
    return want, R.nerr(fn(np.float32), want)


def up(a, dev):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


# ------------------------------------------------------------------------------------------------ the tap tables, exactly
def test_down_layer_tap_table(dev):
    """One channel, no bias, a single non-zero input element at each of the 16 positions of a 4 x 4 input (16 frames): every
    element of the 2 x 2 output is w[ky][kx] x with ky = i - 2 y + 1, kx = j - 2 x + 1, or 0 when that tap does not exist."""
    rs = np.random.RandomState(1)
    w = rs.randn(1, 1, 4, 4).astype(np.float32)
    x, want = np.zeros((16, 1, 4, 4), np.float32), np.zeros((16, 1, 2, 2), np.float32)
    for n in range(16):
        i, j = divmod(n, 4)
        x[n, 0, i, j] = np.float32(1.5 + n)
        for y in range(2):
            for xx in range(2):
                ky, kx = i - 2 * y + 1, j - 2 * xx + 1
                if 0 <= ky < 4 and 0 <= kx < 4:
                    want[n, 0, y, xx] = w[0, 0, ky, kx] * x[n, 0, i, j]
    assert torch.equal(T.conv2d_down_ub(up(x, dev), up(w, dev)).cpu(), torch.from_numpy(want))


def test_transposed_layer_tap_table(dev):
    """Likewise for every position of a 2 x 2 input: out[Y][X] = w[Y + 1 - 2 i][X + 1 - 2 j] x where that tap exists, else 0; and a
    1 x 1 input gives out[Y][X] = w[1 + Y][1 + X] x."""
    rs = np.random.RandomState(2)
    w = rs.randn(1, 1, 4, 4).astype(np.float32)
    x, want = np.zeros((4, 1, 2, 2), np.float32), np.zeros((4, 1, 4, 4), np.float32)
    for n in range(4):
        i, j = divmod(n, 2)
        x[n, 0, i, j] = np.float32(0.75 + n)
        for Y in range(4):
            for X in range(4):
                ky, kx = Y + 1 - 2 * i, X + 1 - 2 * j
                if 0 <= ky < 4 and 0 <= kx < 4:
                    want[n, 0, Y, X] = w[0, 0, ky, kx] * x[n, 0, i, j]
    assert torch.equal(T.conv_transpose2d_ub(up(x, dev), up(w, dev)).cpu(), torch.from_numpy(want))
    one = np.full((1, 1, 1, 1), 1.25, np.float32)
    assert torch.equal(T.conv_transpose2d_ub(up(one, dev), up(w, dev)).cpu()[0, 0], torch.from_numpy(w[0, 0, 1:3, 1:3] * np.float32(1.25)))


# ------------------------------------------------------------------------------------------------ the strided layers
# name: (N, C_in, C_out, source size, bias, slope).  Planes whose OUTPUT is at most 16 x 16 take the 8 x 8 tile, larger ones 8 x 32.
DOWN_CASES = {
    "3to5_6x10_untied_lrelu": (1, 3, 5, (6, 10), "untied", 0.2),
    "odd_5x7_source_tied": (3, 2, 3, (5, 7), "tied", None),
    "13to9_4x4_staging_remainder": (1, 13, 9, (4, 4), "untied", 0.2),
    "128to16_4x4_nobias": (1, 128, 16, (4, 4), None, 0.2),
    "2to3_18x70_crosses_tiles": (3, 2, 3, (18, 70), "untied", 0.2),
    "3to9_20x72_eight_per_thread": (1, 3, 9, (20, 72), "tied", None),
    "2to3_24x30_small_tiles_cross": (3, 2, 3, (24, 30), None, None),
    "9to33_10x12_two_chunks_small": (1, 9, 33, (10, 12), "untied", 0.2),
    "2to2_32x32_last_small": (1, 2, 2, (32, 32), None, None),
    "2to2_34x32_first_large": (1, 2, 2, (34, 32), None, None),
    "2to2_2x2_smallest": (3, 2, 2, (2, 2), "tied", 0.2),
}


def strided_inputs(name, N, C_in, C_out, src, out_size, bias, transposed, skip=False):
    rs = np.random.RandomState(sum(map(ord, name)))
    a = {"x": rs.randn(N, C_in, *src), "w": rs.randn(*((C_in, C_out) if transposed else (C_out, C_in)), 4, 4) / np.sqrt(C_in * (4 if transposed else 16))}
    if bias:
        a["bias"] = rs.randn(*((C_out,) if bias == "tied" else (C_out, *out_size)))
    if skip:
        a["skip"] = rs.randn(N, C_out, *out_size)
    return {k: v.astype(np.float32) for k, v in a.items()}


@pytest.mark.parametrize("name", list(DOWN_CASES))
def test_down_layer(dev, name):
    N, C_in, C_out, src, bias, slope = DOWN_CASES[name]
    size = ((src[0] - 2) // 2 + 1, (src[1] - 2) // 2 + 1)
    a = strided_inputs(name, N, C_in, C_out, src, size, bias, False)
    want, e = own(lambda dt: R.down_layer(a["x"], a["w"], a.get("bias"), slope, dt))
    t = {k: up(v, dev) for k, v in a.items()}
    got = T.conv2d_down_ub(t["x"], t["w"], t.get("bias"), slope=slope)
    assert got.shape == (N, C_out, *size) and got.dtype == torch.float32
    gate(f"tex_down_{name}", got, want, e)
    if N > 1:                                                                 # a frame alone gives the bits it has inside the batch
        assert torch.equal(T.conv2d_down_ub(t["x"][1:2], t["w"], t.get("bias"), slope=slope)[0], got[1])


def test_down_layer_channel_window_source(dev):
    rs = np.random.RandomState(5)
    x, w, b = rs.randn(2, 7, 9, 40).astype(np.float32), (rs.randn(3, 4, 4, 4) / 8).astype(np.float32), rs.randn(3, 4, 20).astype(np.float32)
    want, e = own(lambda dt: R.down_layer(x[:, 2:6], w, b, dtype=dt))
    tx = up(x, dev)
    got = T.conv2d_down_ub(tx[:, 2:6], up(w, dev), up(b, dev))
    gate("tex_down_channel_window", got, want, e)
    assert torch.equal(T.conv2d_down_ub(tx[1:2, 2:6], up(w, dev), up(b, dev))[0], got[1])


# name: (N, C_in, C_out, source size, bias, slope, sigmoid_beta, skip).  SOURCE planes up to 16 x 16 take the 8 x 8 tile.
UP_CASES = {
    "3to5_3x5_untied_lrelu": (1, 3, 5, (3, 5), "untied", 0.2, None, False),
    "13to6_9x33_crosses_tiles": (3, 13, 6, (9, 33), "tied", None, None, True),
    "256to7_4x4_skip_lrelu": (1, 256, 7, (4, 4), "untied", 0.2, None, True),
    "64to1_8x8_sigmoid": (3, 64, 1, (8, 8), "untied", None, 1.0, False),
    "4to3_10x40_four_per_thread": (1, 4, 3, (10, 40), None, 0.2, None, False),
    "5to3_12x11_small_tiles_cross": (3, 5, 3, (12, 11), None, None, None, True),
    "17to35_5x6_two_chunks_small": (1, 17, 35, (5, 6), "untied", 0.2, None, False),
    "2to2_16x16_last_small": (1, 2, 2, (16, 16), None, None, None, False),
    "2to2_17x16_first_large": (1, 2, 2, (17, 16), None, None, None, False),
    "3to2_1x1_smallest_sigmoid": (3, 3, 2, (1, 1), "tied", None, -0.5, True),
}


@pytest.mark.parametrize("name", list(UP_CASES))
def test_transposed_layer(dev, name):
    N, C_in, C_out, src, bias, slope, beta, skip = UP_CASES[name]
    size = (2 * src[0], 2 * src[1])
    a = strided_inputs(name, N, C_in, C_out, src, size, bias, True, skip)
    want, e = own(lambda dt: R.up_layer(a["x"], a["w"], a.get("bias"), slope, beta, a.get("skip"), dt))
    t = {k: up(v, dev) for k, v in a.items()}
    got = T.conv_transpose2d_ub(t["x"], t["w"], t.get("bias"), slope=slope, sigmoid_beta=beta, skip=t.get("skip"))
    assert got.shape == (N, C_out, *size) and got.dtype == torch.float32
    gate(f"tex_up_{name}", got, want, e)
    if N > 1:
        alone = T.conv_transpose2d_ub(t["x"][1:2], t["w"], t.get("bias"), slope=slope, sigmoid_beta=beta, skip=t["skip"][1:2] if skip else None)
        assert torch.equal(alone[0], got[1])


# ------------------------------------------------------------------------------------------------ resize and compose
@pytest.mark.parametrize("src,size", [((5, 7), (10, 14)), ((3, 3), (48, 48)), ((1, 1), (4, 4)), ((7, 5), (9, 11)), ((12, 12), (5, 7))])
def test_resize(dev, src, size):
    x = np.random.RandomState(sum(src) + sum(size)).randn(3, 2, *src).astype(np.float32)
    want, e = own(lambda dt: R.resize(x, size, dt))
    t = up(x, dev)
    got = T.resize_bilinear(t, size)
    gate(f"tex_resize_{src[0]}x{src[1]}_to_{size[0]}x{size[1]}", got, want, e)
    assert torch.equal(T.resize_bilinear(t[1:2], size)[0], got[1])
    same = T.resize_bilinear(t, src)                                          # the same size returns equal bits in a new tensor
    assert same.data_ptr() != t.data_ptr() and torch.equal(same, t)
    assert T.resize_bilinear(t[:0], size).shape == (0, 2, *size)


@pytest.mark.parametrize("shadow", [None, "per_frame", "shared"])
def test_compose(dev, shadow):
    rs = np.random.RandomState(11)
    a = {"t": rs.randn(2, 3, 5, 7), "u": rs.randn(2, 12, 5, 7), "mean": 100 + 40 * rs.randn(3, 10, 14)}
    if shadow:
        a["shadow"] = rs.rand(2 if shadow == "per_frame" else 1, 1, 10, 14)
    a = {k: v.astype(np.float32) for k, v in a.items()}
    want, e = own(lambda dt: R.compose(a["t"], a["u"], a["mean"], 48.0, a.get("shadow"), dt))
    t = {k: up(v, dev) for k, v in a.items()}
    before = {k: v.clone() for k, v in t.items()}
    got = T.compose_texture(t["t"], t["u"], t["mean"], 48.0, t.get("shadow"))
    gate(f"tex_compose_{shadow}", got, want, e)
    assert all(torch.equal(t[k], before[k]) for k in t)                       # nothing is written except out
    sh = t.get("shadow")
    alone = T.compose_texture(t["t"][1:2], t["u"][1:2], t["mean"][None], 48.0, None if sh is None else sh[1:2] if shadow == "per_frame" else sh)
    assert torch.equal(alone[0], got[1])
    assert T.compose_texture(t["t"][:0], t["u"][:0], t["mean"], 48.0).shape == (0, 3, 10, 14)


def test_compose_is_the_pixel_shuffle_of_u_exactly(dev):
    u = torch.randn(2, 12, 5, 7, device=dev)
    got = T.compose_texture(torch.zeros(2, 3, 5, 7, device=dev), u, torch.zeros(3, 10, 14, device=dev), 1.0, torch.ones(1, 1, 10, 14, device=dev))
    assert torch.equal(got, torch.nn.functional.pixel_shuffle(u, 2))


# ------------------------------------------------------------------------------------------------ the fixture networks
def test_view_unet_on_the_fixture(dev, gold, fx):
    net = T.ViewUNet(fx["unet"], **fx["unet_cfg"])
    keep_w, keep = {}, {}
    want = R.unet_forward(fx["unet"], fx["unet_x"], keep=keep_w)
    x = up(fx["unet_x"], dev)
    got = net(x, keep=keep)
    gate("tex_unet_out", got, want, gold["e_ref/unet/out"])
    gate("tex_unet_down5", keep["down5"], keep_w["down5"], gold["e_ref/unet/down5"])
    gate("tex_unet_up1", keep["up1"], keep_w["up1"], gold["e_ref/unet/up1"])
    assert torch.equal(net(x[1:2])[0], got[1])
    with pytest.raises(T.A2PError, match=r"x must be float32 \[N, 4, 64, 64\]"):
        net(x[:, :3])


def test_pose_shadow_on_the_fixture(dev, gold, fx):
    net = T.PoseShadow(fx["shadow"], **fx["shadow_cfg"])
    keep_w, keep = {}, {}
    want = R.pose_shadow_forward(fx["shadow"], fx["shadow_motion"], fx["shadow_cfg"]["uv_size"], keep=keep_w)
    m = up(fx["shadow_motion"], dev)
    got = net(m, keep=keep)
    gate("tex_shadow_map", got, want, gold["e_ref/shadow/shadow_map"])
    gate("tex_shadow_map_lowres", keep["shadow_map_lowres"], keep_w["shadow_map_lowres"], gold["e_ref/shadow/shadow_map_lowres"])
    assert torch.equal(net(m[1:2])[0], got[1])


@pytest.fixture(scope="module")
def full_frame(dev, fx):
    """The one full-size frame (1024 -> 2048) of forward_tex: the float64 restatement and the GPU result, computed once."""
    want = R.fixture_forward_tex(fx)
    net = T.UpscaleNet(fx["upscale"], **fx["upscale_cfg"])
    inputs = {k: up(fx[k], dev) for k in ("tex_mean_rec", "tex_view_rec", "shadow_map")}
    before = {k: v.clone() for k, v in inputs.items()}
    got = T.forward_tex(net, D.SeamSampler(fx["seam_data_1024"]), D.SeamSampler(fx["seam_data_2048"]), up(fx["tex_mean"][0], dev), fx["tex_std"],
                        **inputs)
    assert all(torch.equal(inputs[k], before[k]) for k in inputs)             # the inputs are left as they were
    u = net(torch.cat([inputs["tex_mean_rec"], inputs["tex_view_rec"]], 1))
    return {"want": want, "got": got, "u": u}


def test_forward_tex_on_the_full_size_frame(gold, fx, full_frame):
    gate("tex_forward_tex", full_frame["got"], full_frame["want"], gold["e_ref/forward_tex/tex_rec"])
    want_u = R.upscale_forward(fx["upscale"], np.concatenate([fx["tex_mean_rec"], fx["tex_view_rec"]], 1))
    gate("tex_upscale", full_frame["u"], want_u, gold["e_ref/forward_tex/upscale"])


def test_linear_to_display(dev, gold, fx):
    gate("tex_display", T.linear_to_display(up(fx["display_rgb"], dev)), R.display(fx["display_rgb"]), gold["e_ref/display"])
    got = T.linear_to_display(up(fx["display_rgb"], dev))
    assert float(got.min()) == 0.0 and float(got.max()) == 255.0              # the fixture reaches both clamps


# ------------------------------------------------------------------------------------------------ the whole texture, frames
@pytest.fixture(scope="module")
def body(dev):
    """The decoder fixture (uv 256, 437 vertices, 6 + 10 pose parameters) with a small BodyTexture, a skeleton and a 48 x 64 camera.
    This scene is for bit-equality only: the random skeleton and the unscaled deltas fold the sheet and the camera is far away,
    so no value can be gated on it.  tests/test_body_chain_hip.py gates the values, on a scene made for that."""
    f = DR.make_fixture()
    s = f["surf"]
    small = S.BodySurface.from_arrays(s["vi"], s["vt"], s["vti"], n_verts=s["n_verts"], v2uv=s["v2uv"], uv_size=48)
    surface = S.BodySurface.from_arrays(s["vi"], s["vt"], s["vti"], n_verts=s["n_verts"], v2uv=s["v2uv"], uv_size=256)
    decoder = D.BodyDecoder.from_state_dict({"decoder." + k: v for k, v in f["params"].items()}, f["assets"], small, **f["cfg"])
    sd, assets = R.texture_state(41, 256)
    cfg = dict(uv_size=256, n_init_ftrs=2, upscale_n_ftrs=3, pose_to_shadow_dims=16)
    texture = T.BodyTexture.from_state_dict(sd, assets, surface, **cfg)
    plain = T.BodyTexture.from_state_dict({k: v for k, v in sd.items() if not k.startswith("pose_to_shadow.")}, assets, surface, **cfg)
    skel = SR.make_skeleton(12, 6, 437, 4, P_pos=16, P_scale=3)
    sk = SK.BodySkeleton.from_arrays(skel["parents"], skel["pre_rotation"], skel["joint_offset"], skel["transform"], skel["transform_offsets"],
                                     16, 3, skel["rest_vertices"], skel["skin_indices"], skel["skin_weights"],
                                     template_verts=s["rest"], lbs_scale=np.zeros(3, np.float32), global_scaling=np.float32(10.0))
    rs = np.random.RandomState(12)
    poses, embs, face = rs.randn(1, 3, 16) * 0.5, rs.randn(1, 3, 16), rs.randn(1, 3, 8)
    frames = up(poses.reshape(3, 16), dev)
    preds = decoder.forward(frames, up(embs.reshape(3, 16), dev), up(face.reshape(3, 8), dev))
    verts = sk.pose_vertices(frames, verts_unposed=preds["geom_delta_rec"])
    lo, hi = verts.reshape(-1, 3).min(0).values.cpu().numpy(), verts.reshape(-1, 3).max(0).values.cpu().numpy()
    centre = (lo + hi) / 2
    K, Rt = RD.look_at(centre + np.array([0.0, 0.0, 2.5 * float((hi - lo).max())]), centre, (0.0, 1.0, 0.0), 48, 64, 40.0)
    return {"decoder": decoder, "texture": texture, "plain": plain, "surface": surface, "skeleton": sk, "rasterizer": RD.BodyRasterizer(surface, 48, 64),
            "poses": poses, "embs": embs, "face": face, "frames": frames, "preds": preds, "verts": verts, "K": K[None].to(dev), "Rt": Rt[None].to(dev)}


def test_body_texture_forward(dev, body):
    tex, surface, verts, mean = body["texture"], body["surface"], body["verts"], body["preds"]["tex_mean_rec"]
    cam = RD.camera_centre(body["Rt"])
    out = tex.forward(verts, mean, cam, motion=body["frames"])
    assert set(out) == {"tex_rec", "tex_view_rec", "cond_view", "shadow_map"}
    assert out["tex_rec"].shape == (3, 3, 512, 512) and out["shadow_map"].shape == (3, 1, 512, 512) and bool(torch.isfinite(out["tex_rec"]).all())
    assert torch.equal(out["cond_view"], torch.cat([surface.to_uv(surface.view_cos(verts, cam)[..., None]), mean], 1))
    # the pieces by hand, bit for bit
    assert torch.equal(out["tex_view_rec"], tex.view_net(out["cond_view"]))
    assert torch.equal(out["shadow_map"], tex.pose_shadow(body["frames"]))
    assert torch.equal(out["tex_rec"], tex.forward_tex(mean, out["tex_view_rec"], out["shadow_map"]))
    alone = tex.forward(verts[1:2], mean[1:2], cam, motion=body["frames"][1:2])
    for k in out:
        assert torch.equal(alone[k][0], out[k][1]), f"frame 1 of {k} depends on the batch"
    # a caller's shadow map; neither (the shadow is 1); both is refused
    given = tex.forward(verts, mean, cam, shadow_map=out["shadow_map"][:1])
    assert torch.equal(given["shadow_map"], out["shadow_map"][:1]) and torch.equal(given["tex_rec"][0], out["tex_rec"][0])
    none = body["plain"].forward(verts, mean, cam)
    assert none["shadow_map"] is None and torch.equal(none["tex_view_rec"], out["tex_view_rec"])
    with pytest.raises(T.A2PError, match="pass motion .for PoseToShadow. or shadow_map, not both"):
        tex.forward(verts, mean, cam, motion=body["frames"], shadow_map=out["shadow_map"])
    with pytest.raises(T.A2PError, match="no pose_to_shadow"):
        body["plain"].forward(verts, mean, cam, motion=body["frames"])


def test_render_rgb_motion_in_chunks_of_one_frame(dev, body):
    b = body
    args = (b["decoder"], b["texture"], b["skeleton"], b["rasterizer"], b["poses"], b["embs"], b["face"], b["K"], b["Rt"])
    with torch.cuda.device(dev):
        whole = T.render_rgb_motion(*args)
        calls = []
        forward = b["texture"].forward
        b["texture"].forward = lambda *a, **k: (calls.append(a[0].shape[0]), forward(*a, **k))[1]
        try:
            chunked = T.render_rgb_motion(*args, max_bytes=1)
        finally:
            del b["texture"].forward
    assert calls == [1, 1, 1] and whole.shape == (1, 3, 3, 48, 64) and whole.dtype == torch.float32
    assert torch.equal(whole, chunked)
    tex = b["texture"].forward(b["verts"], b["preds"]["tex_mean_rec"], RD.camera_centre(b["Rt"]), motion=b["frames"])
    image = b["rasterizer"].render(b["verts"], tex["tex_rec"], b["K"], b["Rt"])["render"]
    assert torch.equal(whole[0], T.linear_to_display(image))
    assert float(whole.max()) > 0 and float(whole.min()) >= 0 and float(whole.max()) <= 255
    with pytest.raises(T.A2PError, match=r"embs must be \[1, 3, 16\]"):
        T.render_rgb_motion(b["decoder"], b["texture"], b["skeleton"], b["rasterizer"], b["poses"], b["embs"][:, :2], b["face"], b["K"], b["Rt"])


# ------------------------------------------------------------------------------------------------ refusals, N = 0
def test_refusals_and_empty_batches(dev):
    x, w = torch.randn(2, 4, 6, 6, device=dev), torch.randn(4, 4, 4, 4, device=dev)
    lib = _lib.load()

    def call(entry, out, **over):
        d = _lib.A2PTexConvDesc()
        d.x = _lib.A2PConvSource(_lib.ptr(x), 4 * 36, 4, 6, 6, 0)
        d.weight, d.out, d.N, d.C_out = _lib.ptr(w), out, 2, 4
        for k, v in over.items():
            setattr(d, k, v)
        with torch.cuda.device(dev):
            return _lib.check(getattr(lib, entry)(ctypes.byref(d), _lib.current_stream(dev)), entry)

    down, upo = torch.zeros(2, 4, 3, 3, device=dev), torch.zeros(2, 4, 12, 12, device=dev)
    assert call("a2p_conv2d_down_ub", _lib.ptr(down)) == 0 and call("a2p_conv_transpose2d_ub", _lib.ptr(upo)) == 0
    assert torch.equal(down, T.conv2d_down_ub(x, w)) and torch.equal(upo, T.conv_transpose2d_ub(x, w))
    for entry, name in (("a2p_conv2d_down_ub", "conv2d_down_ub"), ("a2p_conv_transpose2d_ub", "conv_transpose2d_ub")):
        with pytest.raises(T.A2PError, match=f"{name}: out must not alias an input .it overlaps x."):
            call(entry, x[1:].data_ptr())                                     # a partial overlap, not only the same pointer
        with pytest.raises(T.A2PError, match=f"{name}: out must not alias an input .it overlaps weight."):
            call(entry, _lib.ptr(w))
        with pytest.raises(T.A2PError, match=f"{name}: C_out={_lib.CONV_MAX_CHANNELS + 1}, outside"):
            call(entry, _lib.ptr(upo), C_out=_lib.CONV_MAX_CHANNELS + 1)
        with pytest.raises(T.A2PError, match=f"{name}: bias_mode=2 needs a bias"):
            call(entry, _lib.ptr(upo), bias_mode=_lib.CONV_BIAS_UNTIED)
        with pytest.raises(T.A2PError, match=f"{name}: null x.data, weight or out"):
            call(entry, None)
        before = upo.clone()
        assert call(entry, _lib.ptr(upo), N=0) == 0 and torch.equal(upo, before)
    with pytest.raises(T.A2PError, match="conv2d_down_ub: x is 1 x 6, outside .2, 16384."):
        call("a2p_conv2d_down_ub", _lib.ptr(down), x=_lib.A2PConvSource(_lib.ptr(x), 4 * 36, 4, 1, 6, 0))
    with pytest.raises(T.A2PError, match="conv2d_down_ub: act=2 outside .0, 1."):
        call("a2p_conv2d_down_ub", _lib.ptr(down), act=_lib.TEX_ACT_SIGMOID)
    with pytest.raises(T.A2PError, match="conv_transpose2d_ub: out must not alias an input .it overlaps skip."):
        call("a2p_conv_transpose2d_ub", _lib.ptr(upo), skip=_lib.ptr(upo))
    with torch.cuda.device(dev):
        with pytest.raises(T.A2PError, match="resize_bilinear: out must not alias x"):
            _lib.check(lib.a2p_resize_bilinear(_lib.ptr(x), 8, 6, 6, 6, 6, _lib.ptr(x), _lib.current_stream(dev)), "a2p_resize_bilinear")
        with pytest.raises(T.A2PError, match="resize_bilinear: the output is 0 x 6"):
            _lib.check(lib.a2p_resize_bilinear(_lib.ptr(x), 8, 6, 6, 0, 6, _lib.ptr(upo), _lib.current_stream(dev)), "a2p_resize_bilinear")
        with pytest.raises(T.A2PError, match="texture_compose: out must not alias an input .it overlaps u."):
            _lib.check(lib.a2p_texture_compose(_lib.ptr(down), _lib.ptr(upo), _lib.ptr(x), 1.0, None, 0, 1, 1, 3, 3, _lib.ptr(upo),
                                               _lib.current_stream(dev)), "a2p_texture_compose")
        with pytest.raises(T.A2PError, match="texture_compose: shadow holds 3 frames, need 1 or N=2"):
            _lib.check(lib.a2p_texture_compose(_lib.ptr(down), _lib.ptr(upo), _lib.ptr(x), 1.0, _lib.ptr(w), 3, 2, 1, 3, 3, _lib.ptr(upo),
                                               _lib.current_stream(dev)), "a2p_texture_compose")
    # the wrappers: shapes, devices, dtypes, N = 0
    with pytest.raises(T.A2PError, match="x is 1 x 6: the 4 x 4 stride-2 convolution needs at least 2 x 2"):
        T.conv2d_down_ub(x[:, :, :1], w)
    with pytest.raises(T.A2PError, match=r"skip must be float32 \[2, 4, 12, 12\]"):
        T.conv_transpose2d_ub(x, w, skip=torch.zeros(2, 4, 12, 11, device=dev))
    with pytest.raises(T.A2PError, match="pass slope .LeakyReLU. or sigmoid_beta, not both"):
        T.conv_transpose2d_ub(x, w, slope=0.2, sigmoid_beta=1.0)
    with pytest.raises(T.A2PError, match=r"weight must be float32 \[C_out, C_in, 4, 4\]"):
        T.conv2d_down_ub(x, w[:, :3])
    for fn in (T.conv2d_down_ub, T.conv_transpose2d_ub):
        with pytest.raises(T.A2PError, match="must live on the MI355X"):
            fn(x.cpu(), w)
        with pytest.raises(T.A2PError, match="x must be float32"):
            fn(x.double(), w)
        with pytest.raises(T.A2PError, match="weight must be float32"):
            fn(x, w.half())
    with pytest.raises(T.A2PError, match="must live on the MI355X"):
        T.resize_bilinear(x.cpu(), (3, 3))
    with pytest.raises(T.A2PError, match="x must be float32"):
        T.resize_bilinear(x.double(), (3, 3))
    with pytest.raises(T.A2PError, match=r"u must be float32 \[2, 16, 6, 6\]"):
        T.compose_texture(x, x, torch.zeros(4, 12, 12, device=dev), 1.0)
    with pytest.raises(T.A2PError, match="must live on the MI355X"):
        T.compose_texture(x.cpu(), torch.zeros(2, 16, 6, 6), torch.zeros(4, 12, 12), 1.0)
    assert T.conv2d_down_ub(x[:0], w).shape == (0, 4, 3, 3) and T.conv_transpose2d_ub(x[:0], w).shape == (0, 4, 12, 12)
