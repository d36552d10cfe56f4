"""Host side of the texture layers (audio2photoreal_amd/texture.py) and their numpy restatement (tests/texture_restatement.py)
against PyTorch's own strided convolutions, interpolation and pixel shuffle in float64, and against the reference's UNetWB,
PoseToShadow, forward_tex and linear2displayBatch stored in tests/golden/golden_texture_v1.npz.  No GPU."""
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import texture_restatement as R
from audio2photoreal_amd import _lib
from audio2photoreal_amd import surface as S
from audio2photoreal_amd import texture as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_texture_v1.npz"))


@pytest.fixture(scope="module")
def fx():
    return R.make_fixture()


@pytest.fixture(scope="module")
def surface():
    from surface_restatement import make_surface
    s = make_surface()
    return S.BodySurface.from_arrays(s["vi"], s["vt"], s["vti"], n_verts=s["n_verts"], uv_size=32)


@pytest.mark.parametrize("shape", [(2, 3, 5, 6, 10), (1, 2, 3, 5, 7), (1, 4, 2, 2, 2), (1, 1, 1, 9, 3)])
def test_strided_layers_against_torch_in_float64(shape):
    N, C_in, C_out, Hs, Ws = shape
    rs = np.random.RandomState(sum(shape))
    x = rs.randn(N, C_in, Hs, Ws)
    w = rs.randn(C_out, C_in, 4, 4)
    want = F.conv2d(t64(x), t64(w), stride=2, padding=1).numpy()
    got = R.conv_down(x, w)
    assert got.shape == want.shape == (N, C_out, (Hs - 2) // 2 + 1, (Ws - 2) // 2 + 1)
    assert np.abs(got - want).max() < 1e-12
    wt = rs.randn(C_in, C_out, 4, 4)                                          # 16 independent taps per channel pair
    want = F.conv_transpose2d(t64(x), t64(wt), stride=2, padding=1).numpy()
    got = R.conv_transpose(x, wt)
    assert got.shape == want.shape == (N, C_out, 2 * Hs, 2 * Ws)
    assert np.abs(got - want).max() < 1e-12


@pytest.mark.parametrize("src,size", [((5, 7), (10, 14)), ((3, 3), (48, 48)), ((1, 1), (4, 4)), ((7, 5), (9, 11)), ((12, 12), (5, 7)),
                                      ((128, 128), (320, 320)), ((6, 6), (6, 6))])
def test_resize_against_torch(src, size):
    x = np.random.RandomState(3).randn(2, 3, *src)
    want = F.interpolate(t64(x), size, mode="bilinear", align_corners=False).numpy()
    assert np.abs(R.resize(x, size) - want).max() < 1e-12


def test_pixel_shuffle_and_compose_against_torch():
    rs = np.random.RandomState(4)
    t, u = rs.randn(2, 3, 5, 7), rs.randn(2, 12, 5, 7)
    mean, shadow = rs.randn(3, 10, 14), rs.rand(2, 1, 10, 14)
    assert np.array_equal(R.pixel_shuffle(u), F.pixel_shuffle(t64(u), 2).numpy())
    want = ((F.interpolate(t64(t), (10, 14), mode="bilinear", align_corners=False) + F.pixel_shuffle(t64(u), 2)) * 48.0 + t64(mean)) * t64(shadow)
    assert np.abs(R.compose(t, u, mean, 48.0, shadow) - want.numpy()).max() < 1e-11
    assert np.abs(R.compose(t, u, mean, 48.0, shadow[:1]) - (want / t64(shadow) * t64(shadow[:1])).numpy()).max() < 1e-11


def test_the_generated_fixture_is_the_one_the_reference_ran_on(gold, fx):
    for net in ("unet", "shadow", "upscale"):
        stored = {k.split("/", 2)[2]: float(gold[k]) for k in gold.files if k.startswith(f"fingerprint/{net}/")}
        assert R.fingerprint(fx[net]) == stored, net
    for k in gold.files:
        if k.startswith("input/"):
            assert float(np.asarray(fx[k[6:]], np.float64).sum()) == float(gold[k]), k


def test_restatement_reproduces_the_reference(gold, fx):
    """float64 restatement against the reference's float32 modules: on the stored elements the difference, normalised by the
    output's largest value, stays inside e_ref, which was measured over every element."""
    rows = slice(int(gold["rows_start"]), None, int(gold["rows_step"]))
    rows2k = slice(int(gold["rows2k_start"]), None, int(gold["rows2k_step"]))
    keep_u, keep_s = {}, {}
    unet = R.unet_forward(fx["unet"], fx["unet_x"], keep=keep_u)
    shadow = R.pose_shadow_forward(fx["shadow"], fx["shadow_motion"], fx["shadow_cfg"]["uv_size"], keep=keep_s)
    x6 = np.concatenate([fx["tex_mean_rec"], fx["tex_view_rec"]], 1)
    whole = {"unet/out": (unet, None), "unet/down5": (keep_u["down5"], None), "unet/up1": (keep_u["up1"], None),
             "shadow/shadow_map": (shadow, rows), "shadow/shadow_map_lowres": (keep_s["shadow_map_lowres"], None),
             "forward_tex/tex_rec": (R.fixture_forward_tex(fx), rows2k),
             "forward_tex/upscale": (R.pixel_shuffle(R.upscale_forward(fx["upscale"], x6)), rows2k), "display": (R.display(fx["display_rgb"]), None)}
    assert {k[4:] for k in gold.files if k.startswith("ref/")} == set(whole)
    for name, (want, r) in whole.items():
        ref, e_ref = gold[f"ref/{name}"], float(gold[f"e_ref/{name}"])
        sub = want[..., r, :] if r is not None else want
        assert 0 < e_ref < 1e-4, name                                         # a float32 rounding error, not a formula error
        assert ref.shape == sub.shape and ref.dtype == np.float32, name
        err = float(np.abs(ref.astype(np.float64) - sub).max() / np.abs(want).max())
        assert err <= e_ref, (name, err, e_ref)


def test_transposed_fold_has_g_on_axis_1_and_the_norm_over_the_whole_tensor():
    rs = np.random.RandomState(5)
    v, g = rs.randn(6, 5, 4, 4).astype(np.float32), (rs.rand(1, 5, 1, 1) + 0.5).astype(np.float32)
    w = T.folded_weight_transposed({"up.weight_v": v, "up.weight_g": g}, "up", (6, 5, 4, 4))
    want = v.astype(np.float64) * g.astype(np.float64) / np.linalg.norm(v.astype(np.float64))
    assert w.dtype == np.float32 and w.shape == (6, 5, 4, 4) and np.array_equal(w, want.astype(np.float32))
    assert np.array_equal(w, R.weight_of({"up.weight_v": v, "up.weight_g": g}, "up").astype(np.float32))
    fused = T.folded_weight_transposed({"up.weight": w}, "up", (6, 5, 4, 4))                                  # a fused key is taken as it is
    assert np.array_equal(fused, w)
    with pytest.raises(ValueError, match=r"`up\.weight_g` has shape \[5, 1, 1, 1\]; the configuration expects \[1, 5, 1, 1\]"):
        T.folded_weight_transposed({"up.weight_v": v, "up.weight_g": g.reshape(5, 1, 1, 1)}, "up", (6, 5, 4, 4))


def test_view_unet_folds_out_scale_in_float64(fx):
    net = T.ViewUNet(fx["unet"], **fx["unet_cfg"])
    F_ = fx["unet_cfg"]["n_init_ftrs"]
    w = R.weight_of(fx["unet"], "out") * 0.1
    assert np.array_equal(net.params["out.weight_x"], w[:, :F_].astype(np.float32))
    assert np.array_equal(net.params["out.weight_x1"], w[:, F_:, 0, 0].astype(np.float32))
    assert np.array_equal(net.params["out.bias"], (fx["unet"]["out.bias"].astype(np.float64) * 0.1).astype(np.float32))
    assert np.array_equal(net.params["up3.0.weight"], R.weight_of(fx["unet"], "up3.0").astype(np.float32))
    assert all(v.dtype == np.float32 for v in net.params.values())


def test_prepare_tex_mean_against_torch_in_float64():
    rs = np.random.RandomState(6)
    x = rs.rand(3, 23, 31) * 255
    k1 = torch.exp(-0.5 * (torch.linspace(-5, 5, 11, dtype=torch.float64) / 2.0) ** 2)
    k1 = k1 / k1.sum()
    kernel = (k1[:, None] * k1[None, :]).expand(3, 1, 11, 11)
    blurred = F.conv2d(F.pad(t64(x)[None], (5, 5, 5, 5), mode="reflect"), kernel, groups=3)
    assert np.abs(T.gaussian_blur(x) - blurred[0].numpy()).max() < 1e-10
    assert np.abs(R.blur(x) - blurred[0].numpy()).max() < 1e-10
    want = F.interpolate(blurred, (64, 64), mode="bilinear", align_corners=False).numpy()
    got = T.prepare_tex_mean(x, 64)
    assert got.dtype == np.float32 and got.shape == (1, 3, 64, 64) and np.array_equal(got, want.astype(np.float32))
    with pytest.raises(ValueError, match=r"tex_mean must be \[C, H, W\]"):
        T.prepare_tex_mean(x[0], 64)


def test_loader_refusals_and_optional_parts(surface):
    sd, assets = R.texture_state(31, 32)
    cfg = dict(uv_size=32, n_init_ftrs=2, upscale_n_ftrs=3, pose_to_shadow_dims=16)
    tex = T.BodyTexture.from_state_dict(sd, assets, surface, **cfg)
    assert tex.tex_std == 48.0 and tex.tex_mean.shape == (3, 64, 64) and tex.pose_shadow.uv_size == 64
    assert np.array_equal(tex.tex_mean, T.prepare_tex_mean(assets["tex_mean"], 64)[0]) and tex.activation_bytes_per_frame() > 4 * 3 * 64 * 64
    # the checkpoint's own tex_mean buffer takes precedence; without pose_to_shadow.* there is no shadow network; tex_var defaults
    buffer = np.random.RandomState(1).rand(1, 3, 64, 64).astype(np.float32)
    no_shadow = {k: v for k, v in sd.items() if not k.startswith("pose_to_shadow.")}
    lean = T.BodyTexture.from_state_dict({"m." + k: v for k, v in dict(no_shadow, tex_mean=buffer).items()},
                                         {k: v for k, v in assets.items() if k not in ("tex_var", "tex_mean")}, surface, prefix="m.", **cfg)
    assert lean.pose_shadow is None and lean.tex_std == 64.0 and np.array_equal(lean.tex_mean, buffer[0])

    def refuse(match, sd=sd, assets=assets, **over):
        with pytest.raises(ValueError, match=match):
            T.BodyTexture.from_state_dict(sd, assets, surface, **dict(cfg, **over))

    p = dict(sd)
    del p["decoder_view.unet.up2.0.weight_g"]
    refuse(r"no `up2\.0\.weight_g` \(expected shape \[1, 8, 1, 1\]\)", sd=p)
    p = dict(sd)
    p["upscale_net.out_block.bias"] = np.zeros((12, 32, 31), np.float32)
    refuse(r"`out_block\.bias` has shape \[12, 32, 31\]; the configuration expects \[12, 32, 32\]", sd=p)
    refuse(r"`conv_block\.0\.weight_v` has shape \[3, 6, 3, 3\]; the configuration expects \[5, 6, 3, 3\]", upscale_n_ftrs=5)
    refuse(r"`fc_block\.0\.weight_v` has shape \[4096, 16\]; the configuration expects \[4096, 104\]", pose_to_shadow_dims=104)
    p = dict(sd)
    p["pose_to_shadow.conv_block.4.bias"] = p["pose_to_shadow.conv_block.4.bias"].copy()
    p["pose_to_shadow.conv_block.4.bias"][3, 2, 1] = np.nan
    refuse(r"`conv_block\.4\.bias`\[3, 2, 1\] is not finite", sd=p)
    refuse(r"assets `seam_data_2048` is for 32 x 32 maps; the configuration expects 64 x 64", assets=dict(assets, seam_data_2048=assets["seam_data_1024"]))
    refuse("the assets hold no `seam_data_1024`", assets={k: v for k, v in assets.items() if k != "seam_data_1024"})
    refuse(r"assets `tex_var` has shape \[2\]; the configuration expects a scalar", assets=dict(assets, tex_var=np.array([48.0, 48.0], np.float32)))
    refuse("assets `tex_var` is not finite", assets=dict(assets, tex_var=np.float32(np.inf)))
    refuse("the assets hold no `tex_mean`", assets={k: v for k, v in assets.items() if k != "tex_mean"})
    refuse(r"`tex_mean` has shape \[1, 3, 32, 32\]; the configuration expects \[1, 3, 64, 64\]", sd=dict(sd, tex_mean=buffer[:, :, :32, :32]))
    refuse("the surface maps to 32 texels; uv_size=64", uv_size=64)
    with pytest.raises(ValueError, match="size=48: need a multiple of 32"):
        T.ViewUNet({}, size=48)


def test_header_and_binding_constants_agree():
    header = open(os.path.join(ROOT, "include", "a2p_hip.h")).read()
    enum = dict(re.findall(r"(A2P_TEX_ACT_\w+) = (\d+)", header))
    assert enum == {"A2P_TEX_ACT_NONE": str(_lib.TEX_ACT_NONE), "A2P_TEX_ACT_LRELU": str(_lib.TEX_ACT_LRELU), "A2P_TEX_ACT_SIGMOID": str(_lib.TEX_ACT_SIGMOID)}
    kernels = open(os.path.join(ROOT, "audio2photoreal_amd", "csrc", "kernels_texture.h")).read()
    assert dict(re.findall(r"#define (TEX_ACT_\w+) (\d+)", kernels)) == {k[4:]: v for k, v in enum.items()}
    body = re.search(r"typedef struct a2p_tex_conv_desc \{(.*?)\} a2p_tex_conv_desc;", header, re.S).group(1)
    fields = [piece.split()[-1].lstrip("*") for decl in body.split(";") if decl.strip() for piece in decl.split(",")]
    assert fields == [n for n, _ in _lib.A2PTexConvDesc._fields_]
    assert {"a2p_conv2d_down_ub", "a2p_conv_transpose2d_ub", "a2p_resize_bilinear", "a2p_texture_compose"} <= set(_lib.EXPORTS)
    lib = _lib.load()
    assert len(lib.a2p_texture_compose.argtypes) == 12 and len(lib.a2p_resize_bilinear.argtypes) == 8
