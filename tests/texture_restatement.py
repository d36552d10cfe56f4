"""A numpy restatement of the texture layers (audio2photoreal_amd/texture.py; the reference's visualize/ca_body/nn/unet.py UNetWB,
nn/shadow.py PoseToShadow, UpscaleNet and AutoEncoder.forward_tex of models/mesh_vae_drivable.py, linear2displayBatch of
utils/image.py and torchvision's gaussian_blur), written from the mathematics.  Test infrastructure: the yardstick of
tests/test_texture_hip.py and tests/test_texture_cpu.py, and what tests/golden/make_golden_texture.py measures the reference's own
float32 error against.

As in decoder_restatement.py every numeric function takes `dtype` (float64 by default): all inputs are cast to it and every
operation runs in it; the float32 run against the float64 run is the allowance of the GPU tests for shapes outside the fixture.
Parameters are dicts under the reference's key names without the module prefix (down1.0.weight_v, conv_block.8.bias, ...)."""
import numpy as np

from decoder_restatement import conv2d, fold, impaint, layer, lrelu, nerr, random_seams, resample  # noqa: F401

SLOPE = 0.2


# ------------------------------------------------------------------------------------------------ the layers
def weight_of(params, name, dtype=np.float64):
    """The weight of layer `name`: the fused `name.weight` when present, else v (g / ||v||) with the norm over the whole tensor;
    g broadcasts, so [C_out, 1, 1, 1] (g_dim = 0) and the transposed layers' [1, C_out, 1, 1] (g_dim = 1) both work."""
    if f"{name}.weight" in params:
        return np.asarray(params[f"{name}.weight"], dtype)
    return fold(params[f"{name}.weight_v"], params[f"{name}.weight_g"], dtype)


def conv_down(x, w, dtype=np.float64):
    """4 x 4, stride 2, zero padding 1.  x [N, C_in, Hs, Ws], w [C_out, C_in, 4, 4] -> [N, C_out, (Hs - 2) // 2 + 1, (Ws - 2) // 2 + 1]."""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    N, C_in, Hs, Ws = x.shape
    assert w.shape[1:] == (C_in, 4, 4) and min(Hs, Ws) >= 2
    H, W = (Hs - 2) // 2 + 1, (Ws - 2) // 2 + 1
    xp = np.zeros((N, C_in, Hs + 2, Ws + 2), dtype)
    xp[:, :, 1:1 + Hs, 1:1 + Ws] = x
    out = np.zeros((N, w.shape[0], H, W), dtype)
    for ky in range(4):
        for kx in range(4):
            out = out + np.einsum("oc,nchw->nohw", w[:, :, ky, kx], xp[:, :, ky:ky + 2 * H:2, kx:kx + 2 * W:2]).astype(dtype)
    return out


# output parity -> ((k, source offset), (k, source offset)): Y + 1 - k = 2 (Y // 2 + offset)
TAPS = {0: ((1, 0), (3, -1)), 1: ((0, 1), (2, 0))}


def conv_transpose(x, w, dtype=np.float64):
    """4 x 4, stride 2, padding 1, transposed.  x [N, C_in, Hs, Ws], w [C_in, C_out, 4, 4] -> [N, C_out, 2 Hs, 2 Ws]."""
    x, w = np.asarray(x, dtype), np.asarray(w, dtype)
    N, C_in, Hs, Ws = x.shape
    assert w.shape[0] == C_in and w.shape[2:] == (4, 4)
    xp = np.zeros((N, C_in, Hs + 2, Ws + 2), dtype)
    xp[:, :, 1:1 + Hs, 1:1 + Ws] = x
    out = np.zeros((N, w.shape[1], 2 * Hs, 2 * Ws), dtype)
    for py in (0, 1):
        for px in (0, 1):
            acc = np.zeros((N, w.shape[1], Hs, Ws), dtype)
            for ky, oy in TAPS[py]:
                for kx, ox in TAPS[px]:
                    acc = acc + np.einsum("co,nchw->nohw", w[:, :, ky, kx], xp[:, :, 1 + oy:1 + oy + Hs, 1 + ox:1 + ox + Ws]).astype(dtype)
            out[:, :, py::2, px::2] = acc
    return out


def _bias(v, bias, dtype):
    if bias is None:
        return v
    b = np.asarray(bias, dtype)
    return v + (b[None, :, None, None] if b.ndim == 1 else b[None])


def sigmoid(x, dtype=np.float64):
    x = np.asarray(x, dtype)
    return dtype(1) / (dtype(1) + np.exp(-x))


def down_layer(x, w, bias=None, slope=None, dtype=np.float64):
    """texture.conv2d_down_ub: lrelu(conv_down(x, w) + bias, slope)."""
    v = _bias(conv_down(x, w, dtype), bias, dtype)
    return v if slope is None else lrelu(v, slope, dtype)


def up_layer(x, w, bias=None, slope=None, sigmoid_beta=None, skip=None, dtype=np.float64):
    """texture.conv_transpose2d_ub: act(conv_transpose(x, w) + bias) + skip with act LeakyReLU, sigmoid(. + beta) or none."""
    v = _bias(conv_transpose(x, w, dtype), bias, dtype)
    if slope is not None:
        v = lrelu(v, slope, dtype)
    if sigmoid_beta is not None:
        v = sigmoid(v + dtype(sigmoid_beta), dtype)
    return v if skip is None else v + np.asarray(skip, dtype)


def resize_axis(n_in, n_out, dtype=np.float64):
    """(i0, i1, l0, l1) of F.interpolate(mode="bilinear", align_corners=False) along one axis."""
    scale = dtype(n_in) / dtype(n_out)
    src = np.maximum((np.arange(n_out, dtype=dtype) + dtype(0.5)) * scale - dtype(0.5), dtype(0))
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = src - i0.astype(dtype)
    return i0, i1, dtype(1) - l1, l1


def resize(x, size, dtype=np.float64):
    """F.interpolate(x, size, mode="bilinear", align_corners=False).  x [.., Hs, Ws] -> [.., H, W]."""
    x = np.asarray(x, dtype)
    y0, y1, l0y, l1y = resize_axis(x.shape[-2], size[0], dtype)
    x0, x1, l0x, l1x = resize_axis(x.shape[-1], size[1], dtype)
    top = l0x * x[..., y0, :][..., x0] + l1x * x[..., y0, :][..., x1]
    bot = l0x * x[..., y1, :][..., x0] + l1x * x[..., y1, :][..., x1]
    return l0y[:, None] * top + l1y[:, None] * bot


def pixel_shuffle(u):
    """nn.PixelShuffle(2): [N, 4 C, H, W] -> [N, C, 2 H, 2 W] with out[n][c][Y][X] = u[n][4 c + 2 (Y % 2) + X % 2][Y // 2][X // 2]."""
    u = np.asarray(u)
    N, C4, H, W = u.shape
    return u.reshape(N, C4 // 4, 2, 2, H, W).transpose(0, 1, 4, 2, 5, 3).reshape(N, C4 // 4, 2 * H, 2 * W)


def compose(t, u, tex_mean, tex_std, shadow=None, dtype=np.float64):
    """texture.compose_texture: ((resize(t, 2x) + pixel_shuffle(u)) tex_std + tex_mean) shadow."""
    t = np.asarray(t, dtype)
    v = resize(t, (2 * t.shape[2], 2 * t.shape[3]), dtype) + pixel_shuffle(np.asarray(u, dtype))
    v = v * dtype(tex_std) + np.asarray(tex_mean, dtype).reshape((1,) + v.shape[1:])
    return v if shadow is None else v * np.asarray(shadow, dtype)


# ------------------------------------------------------------------------------------------------ the networks
def unet_forward(params, x, out_scale=0.1, dtype=np.float64, keep=None):
    """UNetWB.forward.  `keep` receives down1 .. down5 and up1 .. up5 (up1 .. up4 with their skip added)."""
    keep = {} if keep is None else keep
    xs = [np.asarray(x, dtype)]
    for i in range(1, 6):
        xs.append(down_layer(xs[-1], weight_of(params, f"down{i}.0", dtype), params[f"down{i}.0.bias"], SLOPE, dtype))
        keep[f"down{i}"] = xs[-1]
    h = xs[5]
    for i in range(1, 6):
        h = up_layer(h, weight_of(params, f"up{i}.0", dtype), params[f"up{i}.0.bias"], SLOPE, skip=xs[5 - i] if i < 5 else None, dtype=dtype)
        keep[f"up{i}"] = h
    return layer(np.concatenate([h, xs[0]], 1), weight_of(params, "out", dtype), params["out.bias"], dtype=dtype) * dtype(out_scale)


SHADOW_LAYERS = ((0, 256, 256, 8), (2, 256, 128, 16), (4, 128, 128, 32), (6, 128, 64, 64), (8, 64, 1, 128))


def pose_shadow_forward(params, motion, uv_size, beta=1.0, dtype=np.float64, keep=None):
    """PoseToShadow.forward: shadow_map [N, 1, uv_size, uv_size]; `keep` receives shadow_map_lowres."""
    motion = np.asarray(motion, dtype)
    x = lrelu(motion @ weight_of(params, "fc_block.0", dtype).T + np.asarray(params["fc_block.0.bias"], dtype), SLOPE, dtype)
    x = x.reshape(-1, 256, 4, 4)
    for i, _, _, _ in SHADOW_LAYERS:
        last = i == 8
        x = up_layer(x, weight_of(params, f"conv_block.{i}", dtype), params[f"conv_block.{i}.bias"], None if last else SLOPE,
                     beta if last else None, dtype=dtype)
    if keep is not None:
        keep["shadow_map_lowres"] = x
    return resize(x, (uv_size, uv_size), dtype)


def upscale_forward(params, x, dtype=np.float64):
    """UpscaleNet's two layers WITHOUT the pixel shuffle: [N, 4 C, S, S]."""
    h = layer(x, weight_of(params, "conv_block.0", dtype), params["conv_block.0.bias"], slope=SLOPE, dtype=dtype)
    return layer(h, weight_of(params, "out_block", dtype), params["out_block.bias"], dtype=dtype)


def seam_steps(x, seam, resamples, dtype):
    x = impaint(x, seam["dst_ij"], seam["src_ij"])
    for _ in range(resamples):
        x = resample(x, seam["uvs"], seam["weights"], dtype)
    return x


def forward_tex(upscale_params, seam, seam_2k, tex_mean, tex_std, tex_mean_rec, tex_view_rec, shadow_map=None, dtype=np.float64):
    """AutoEncoder.forward_tex."""
    a, b = np.asarray(tex_mean_rec, dtype), np.asarray(tex_view_rec, dtype)
    t = seam_steps(a + b, seam, 1, dtype)
    u = upscale_forward(upscale_params, np.concatenate([a, b], 1), dtype)
    if shadow_map is not None:
        shadow_map = seam_steps(np.asarray(shadow_map, dtype), seam_2k, 2, dtype)
    return seam_steps(compose(t, u, tex_mean, tex_std, shadow_map, dtype), seam_2k, 2, dtype)


# ------------------------------------------------------------------------------------------------ host preparation, display
def blur(x, kernel_size=11, dtype=np.float64):
    """torchvision's gaussian_blur with its default sigma, as two 1-D passes over the reflect-padded map."""
    x = np.asarray(x, dtype)
    k, r = kernel_size, kernel_size // 2
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    k1 = np.exp(-0.5 * (np.linspace(-(k - 1) * 0.5, (k - 1) * 0.5, k) / sigma) ** 2)
    k1 = (k1 / k1.sum()).astype(dtype)
    xp = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(r, r), (r, r)], mode="reflect")
    H, W = x.shape[-2:]
    rows = sum(k1[i] * xp[..., i:i + H, :] for i in range(k))
    return sum(k1[j] * rows[..., :, j:j + W] for j in range(k))


def display(rgb, dtype=np.float64):
    """linear2displayBatch(rgb, gamma=1.5, wbscale=[1.05, 0.95, 1.45], black=5 / 255, mode="srgb") on [.., 3, H, W]."""
    wb = np.asarray([1.05, 0.95, 1.45], np.float32).astype(dtype)[:, None, None]
    v = np.asarray(rgb, dtype) / dtype(255) * wb - dtype(5.0 / 255.0)
    curve = dtype(1.055) * np.maximum(v, dtype(0.0031308)) ** dtype(1 / 1.5) - dtype(0.055)
    return np.clip(np.where(v <= dtype(0.0031308), v * dtype(12.92), curve), 0, 1).astype(dtype) * dtype(255)


# ------------------------------------------------------------------------------------------------ the fixture, as data built here
UNET_CFG = dict(in_channels=4, out_channels=3, size=64, n_init_ftrs=4)
SHADOW_CFG = dict(n_pose_dims=10, uv_size=320)
UPSCALE_CFG = dict(in_channels=6, out_channels=3, n_ftrs=4, size=1024)
TEX_STD = 64.0
N_FRAMES = 2


def random_layer(rs, params, name, shape, bias_shape, g_axis=0):
    """weight_v ~ N(0, 1) (so the 16 taps of a transposed layer are independent: the reference's glorot makes the four parities
    equal, which would hide a swapped tap), weight_g on axis g_axis ~ sqrt(C_out) U(0.7, 1.6), bias ~ 0.3 N."""
    g_shape = tuple(s if a == g_axis else 1 for a, s in enumerate(shape))
    params[f"{name}.weight_v"] = rs.randn(*shape).astype(np.float32)
    params[f"{name}.weight_g"] = (np.sqrt(shape[g_axis]) * rs.uniform(0.7, 1.6, g_shape)).astype(np.float32)
    params[f"{name}.bias"] = (0.3 * rs.randn(*bias_shape)).astype(np.float32)


def unet_params(cfg, seed):
    rs, p = np.random.RandomState(seed), {}
    F, s, cin = cfg["n_init_ftrs"], cfg["size"], cfg["in_channels"]
    ch = [cin, F, 2 * F, 4 * F, 8 * F, 16 * F]
    for i in range(1, 6):
        random_layer(rs, p, f"down{i}.0", (ch[i], ch[i - 1], 4, 4), (ch[i], s >> i, s >> i))
    up = [16 * F, 8 * F, 4 * F, 2 * F, F, F]
    for i in range(1, 6):
        random_layer(rs, p, f"up{i}.0", (up[i - 1], up[i], 4, 4), (up[i], s >> (5 - i), s >> (5 - i)), g_axis=1)
    random_layer(rs, p, "out", (cfg["out_channels"], F + cin, 1, 1), (cfg["out_channels"], s, s))
    return p


def shadow_params(cfg, seed):
    rs, p = np.random.RandomState(seed), {}
    random_layer(rs, p, "fc_block.0", (256 * 4 * 4, cfg["n_pose_dims"]), (256 * 4 * 4,))
    for i, cin, cout, s in SHADOW_LAYERS:
        random_layer(rs, p, f"conv_block.{i}", (cin, cout, 4, 4), (cout, s, s), g_axis=1)
    return p


def smooth(rs, shape, coarse=16, scale=1.0):
    """A smooth random map: N(0, scale) on a coarse grid, resized bilinearly, as float32."""
    return (scale * resize(rs.randn(*shape[:-2], coarse, coarse), shape[-2:])).astype(np.float32)


def upscale_params(cfg, seed):
    """UpscaleNet's state dict; the two untied biases (16 M values at 1024 x 1024) are smooth maps."""
    rs, p = np.random.RandomState(seed), {}
    s = cfg["size"]
    random_layer(rs, p, "conv_block.0", (cfg["n_ftrs"], cfg["in_channels"], 3, 3), (1,))
    random_layer(rs, p, "out_block", (4 * cfg["out_channels"], cfg["n_ftrs"], 1, 1), (1,))
    p["conv_block.0.bias"] = smooth(rs, (cfg["n_ftrs"], s, s), scale=0.3)
    p["out_block.bias"] = smooth(rs, (4 * cfg["out_channels"], s, s), scale=0.3)
    return p


def make_fixture(seed=21):
    """Everything the fixture-level tests and the golden maker run, as data: a UNetWB(4, 3, 64, 4) with 2 input frames; a
    PoseToShadow(10, 320) with 2 poses (128 -> 320 is a non-integer ratio); and ONE frame of forward_tex at 1024 -> 2048 (the
    reference hard-codes 2048) with an UpscaleNet(6, 3, 4, 1024), two synthetic seam tables, tex_mean, tex_std and smooth inputs."""
    rs = np.random.RandomState(seed)
    s, S = UNET_CFG["size"], UPSCALE_CFG["size"]
    return {"unet_cfg": dict(UNET_CFG), "unet": unet_params(UNET_CFG, seed + 1), "unet_x": rs.randn(N_FRAMES, 4, s, s).astype(np.float32),
            "shadow_cfg": dict(SHADOW_CFG), "shadow": shadow_params(SHADOW_CFG, seed + 2),
            "shadow_motion": rs.randn(N_FRAMES, SHADOW_CFG["n_pose_dims"]).astype(np.float32),
            "upscale_cfg": dict(UPSCALE_CFG), "upscale": upscale_params(UPSCALE_CFG, seed + 3),
            "seam_data_1024": random_seams(rs, S, S), "seam_data_2048": random_seams(rs, 2 * S, 2 * S),
            "tex_mean": smooth(rs, (1, 3, 2 * S, 2 * S), scale=40.0) + np.float32(100.0), "tex_std": TEX_STD,
            "tex_mean_rec": smooth(rs, (1, 3, S, S)), "tex_view_rec": smooth(rs, (1, 3, S, S), scale=0.1),
            "shadow_map": (0.2 + 0.8 * sigmoid(smooth(rs, (1, 1, 2 * S, 2 * S)))).astype(np.float32),
            "display_rgb": (rs.rand(2, 3, 12, 16) * 300 - 20).astype(np.float32)}


def fixture_forward_tex(fx, dtype=np.float64):
    return forward_tex(fx["upscale"], fx["seam_data_1024"], fx["seam_data_2048"], fx["tex_mean"], fx["tex_std"], fx["tex_mean_rec"],
                       fx["tex_view_rec"], fx["shadow_map"], dtype)


def fingerprint(params):
    """{key: float64 sum of the array}: what the golden file stores of the generated state dicts."""
    return {k: float(np.asarray(v, np.float64).sum()) for k, v in params.items()}


def texture_state(seed, uv_size, n_init_ftrs=2, upscale_n_ftrs=3, pose_dims=16, with_shadow=True):
    """(state dict, assets) of a small BodyTexture under the reference's key names: decoder_view.unet.*, upscale_net.*,
    pose_to_shadow.* and the assets seam_data_1024 / seam_data_2048 (at uv_size and 2 uv_size), tex_mean [3, 40, 40], tex_var."""
    rs = np.random.RandomState(seed)
    sd = {"decoder_view.unet." + k: v for k, v in unet_params(dict(in_channels=4, out_channels=3, size=uv_size, n_init_ftrs=n_init_ftrs), seed + 1).items()}
    up = {}
    random_layer(rs, up, "conv_block.0", (upscale_n_ftrs, 6, 3, 3), (upscale_n_ftrs, uv_size, uv_size))
    random_layer(rs, up, "out_block", (12, upscale_n_ftrs, 1, 1), (12, uv_size, uv_size))
    sd.update({"upscale_net." + k: v for k, v in up.items()})
    if with_shadow:
        sd.update({"pose_to_shadow." + k: v for k, v in shadow_params(dict(n_pose_dims=pose_dims), seed + 2).items()})
    assets = {"seam_data_1024": random_seams(rs, uv_size, uv_size, pairs=40, chains=5),
              "seam_data_2048": random_seams(rs, 2 * uv_size, 2 * uv_size, pairs=40, chains=5),
              "tex_mean": (100 + 40 * rs.randn(3, 40, 40)).astype(np.float32), "tex_var": np.float32(48.0)}
    return sd, assets
