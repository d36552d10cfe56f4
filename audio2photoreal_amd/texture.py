"""The final body texture and RGB frames on the MI355X: what the reference's AutoEncoder.forward (visualize/ca_body/models/
mesh_vae_drivable.py) runs after ConvDecoder -- UNetViewDecoder (nn/unet.py UNetWB), PoseToShadow (nn/shadow.py), UpscaleNet and
forward_tex -- as HIP launches for all frames (csrc/kernels_texture.h), and linear2displayBatch of utils/image.py.

    python -m audio2photoreal_amd.texture --results results.npy --embeddings embs.npz --assets static_assets.pt
                                          --checkpoint body_dec.ckpt --out frames.npy [--size H W]
                                          [--camera-json FILE | --eye X Y Z --target X Y Z --fov D] [--frames A:B] [--png-dir DIR]
                                          [--uv-size S --n-init-ftrs F --upscale-n-ftrs F --pose-to-shadow-dims P --n-embs E ...]

`conv2d_down_ub`, `conv_transpose2d_ub`, `resize_bilinear` and `compose_texture` are one launch each of the four exports of the
"texture layers" of include/a2p_hip.h.  `ViewUNet`, `PoseShadow` and `UpscaleNet` are the reference's networks built from its state
dict; `BodyTexture` is the texture half of AutoEncoder.forward; `render_rgb_motion` chains decoder, skinning, texture, rasteriser
and display curve frame chunk by frame chunk.  Everything takes float32 tensors that live on the GPU and runs on the caller's
current stream; there is no CPU path.

Differences from the reference, on purpose:
  * the weight normalisation is folded once at construction, in float64, and rounded to float32 once, as in decoder.py; for the
    transposed layers (la.ConvTranspose2dWNUB, g_dim = 1) weight_g is [1, C_out, 1, 1] and the norm runs over the whole weight_v;
  * UNetWB's out_scale is folded into its last layer's weight and bias in the same float64 step (the reference multiplies the
    layer's output), and that layer reads cat([x, x1]) as two sources of one launch: the concatenation is never written;
  * the pixel shuffle of UpscaleNet happens inside `compose_texture`;
  * `prepare_tex_mean` restates torchvision's gaussian_blur (kernel 11, sigma 2.0, reflect padding) in float64 numpy; it has
    never been run against torchvision itself, and a checkpoint's own `tex_mean` buffer takes precedence."""
from __future__ import annotations

import argparse
import ctypes
import sys

import numpy as np
import torch

from . import _lib, avatar
from ._lib import A2PError
from .avatar import HostNet, as_numpy, asset, checked, f32, gpu_f32, operand, resize_axis_half64, source
from .decoder import LRELU_SLOPE, SeamSampler, conv2d_ub

WB_SCALE = (1.05, 0.95, 1.45)          # linear2displayBatch's white balance
DISPLAY_GAMMA, DISPLAY_BLACK = 1.5, 5.0 / 255.0


# ------------------------------------------------------------------------------------------------ host preparation
def fold_weight_norm64(weight_v, weight_g) -> np.ndarray:
    """float64 w = weight_v * (weight_g / ||weight_v||) with the norm over the WHOLE weight_v; weight_g broadcasts against weight_v,
    so it serves g_dim = 0 ([C_out, 1, ...]) and the transposed layers' g_dim = 1 ([1, C_out, 1, 1]) alike."""
    v, g = as_numpy(weight_v).astype(np.float64), as_numpy(weight_g).astype(np.float64)
    return v * (g / np.sqrt((v * v).sum()))


def folded_weight64(state_dict, name: str, shape, g_axis: int = 0) -> np.ndarray:
    """The float64 weight of layer `name`: `name.weight` when the state dict holds the fused tensor, else the fold of `name.weight_g`
    (1 everywhere but shape[g_axis] on axis g_axis) and `name.weight_v`.  A missing key or a wrong shape is a ValueError naming it."""
    shape = tuple(int(s) for s in shape)
    if f"{name}.weight" in state_dict:
        return checked(state_dict, f"{name}.weight", shape).astype(np.float64)
    g_shape = tuple(s if a == g_axis else 1 for a, s in enumerate(shape))
    return fold_weight_norm64(checked(state_dict, f"{name}.weight_v", shape), checked(state_dict, f"{name}.weight_g", g_shape))


def folded_weight_transposed(state_dict, name: str, shape) -> np.ndarray:
    """float32 weight [C_in, C_out, 4, 4] of a la.ConvTranspose2dWNUB: weight_g is [1, C_out, 1, 1] (g_dim = 1)."""
    return np.ascontiguousarray(folded_weight64(state_dict, name, shape, g_axis=1), np.float32)


def gaussian_blur(x, kernel_size: int = 11) -> np.ndarray:
    """float64 [.., H, W]: torchvision's gaussian_blur with its default sigma 0.3 ((k - 1) / 2 - 1) + 0.8, restated: the 1-D kernel
    exp(-x^2 / 2 sigma^2) at x = -(k - 1) / 2 .. (k - 1) / 2, normalised; its outer product; reflect padding."""
    x = as_numpy(x).astype(np.float64)
    k, r = int(kernel_size), int(kernel_size) // 2
    if k % 2 != 1 or min(x.shape[-2:]) <= r:
        raise ValueError(f"gaussian_blur: kernel_size={k} must be odd and the map ({list(x.shape[-2:])}) larger than {r} (reflect padding)")
    sigma = 0.3 * ((k - 1) * 0.5 - 1) + 0.8
    k1 = np.exp(-0.5 * (np.linspace(-(k - 1) * 0.5, (k - 1) * 0.5, k) / sigma) ** 2)
    k1 /= k1.sum()
    k2 = np.outer(k1, k1)
    xp = np.pad(x, [(0, 0)] * (x.ndim - 2) + [(r, r), (r, r)], mode="reflect")
    H, W = x.shape[-2:]
    out = np.zeros_like(x)
    for ky in range(k):
        for kx in range(k):
            out += k2[ky, kx] * xp[..., ky:ky + H, kx:kx + W]
    return out


def prepare_tex_mean(tex_mean, size: int) -> np.ndarray:
    """float32 [1, 3, size, size]: AutoEncoder.__init__'s F.interpolate(gaussian_blur(tex_mean[None], kernel_size=11), (size, size),
    mode="bilinear") in float64 numpy, rounded to float32 once.  tex_mean is the assets' [C, H, W]."""
    a = as_numpy(tex_mean)
    if a.ndim != 3:
        raise ValueError(f"tex_mean must be [C, H, W] (got {list(a.shape)})")
    if not np.isfinite(a).all():
        raise ValueError("tex_mean holds non-finite values")
    b = gaussian_blur(a[None], 11)
    (y0, y1, ly), (x0, x1, lx) = resize_axis_half64(b.shape[2], int(size)), resize_axis_half64(b.shape[3], int(size))
    top = (1 - lx) * b[:, :, y0][:, :, :, x0] + lx * b[:, :, y0][:, :, :, x1]
    bot = (1 - lx) * b[:, :, y1][:, :, :, x0] + lx * b[:, :, y1][:, :, :, x1]
    return f32((1 - ly)[:, None] * top + ly[:, None] * bot)


# ------------------------------------------------------------------------------------------------ the four launches
def _strided(entry: str, x, weight, bias, slope, sigmoid_beta, skip, transposed: bool):
    x, xs = source(x, "x")
    N, C_in, Hs, Ws = x.shape
    dev = x.device
    if not transposed and min(Hs, Ws) < 2:
        raise A2PError(f"x is {Hs} x {Ws}: the 4 x 4 stride-2 convolution needs at least 2 x 2")
    if transposed and max(Hs, Ws) > _lib.CONV_MAX_SIZE // 2:
        raise A2PError(f"x is {Hs} x {Ws}: the output side may not exceed {_lib.CONV_MAX_SIZE}")
    H, W = (2 * Hs, 2 * Ws) if transposed else ((Hs - 2) // 2 + 1, (Ws - 2) // 2 + 1)
    w_text = "[C_in, C_out, 4, 4]" if transposed else "[C_out, C_in, 4, 4]"
    weight = operand(weight, "weight", w_text, lambda s: len(s) == 4 and s[2:] == (4, 4) and s[0 if transposed else 1] == C_in, dev)
    C_out = weight.shape[1 if transposed else 0]
    d = _lib.A2PTexConvDesc()
    d.x, d.weight, d.N, d.C_out = xs, _lib.ptr(weight), N, C_out
    keep = [x, weight]
    if bias is not None:
        bias = operand(bias, "bias", f"[{C_out}] or [{C_out}, {H}, {W}]", lambda s: s in ((C_out,), (C_out, H, W)), dev)
        keep.append(bias)
        d.bias, d.bias_mode = _lib.ptr(bias), _lib.CONV_BIAS_TIED if bias.dim() == 1 else _lib.CONV_BIAS_UNTIED
    if slope is not None and sigmoid_beta is not None:
        raise A2PError("pass slope (LeakyReLU) or sigmoid_beta, not both")
    if slope is not None:
        d.act, d.slope = _lib.TEX_ACT_LRELU, float(slope)
    if sigmoid_beta is not None:
        d.act, d.beta = _lib.TEX_ACT_SIGMOID, float(sigmoid_beta)
    if skip is not None:
        skip = operand(skip, "skip", f"[{N}, {C_out}, {H}, {W}]", lambda s: s == (N, C_out, H, W), dev)
        keep.append(skip)
        d.skip = _lib.ptr(skip)
    out = torch.empty(N, C_out, H, W, dtype=torch.float32, device=dev)
    d.out = _lib.ptr(out)
    if N == 0:
        return out
    with _lib.on_device_of(x):
        _lib.check(getattr(_lib.load(), entry)(ctypes.byref(d), _lib.current_stream(dev)), entry)
    return out


def conv2d_down_ub(x, weight, bias=None, *, slope=None):
    """One launch of a2p_conv2d_down_ub: la.Conv2dWNUB(C_in, C_out, H, W, 4, 2, 1) and an optional LeakyReLU(slope).  x [N, C_in, Hs,
    Ws] with Hs, Ws >= 2 (a channel window of a contiguous tensor is passed as it is); weight [C_out, C_in, 4, 4], already folded;
    bias [C_out], [C_out, H, W] or None.  Returns [N, C_out, (Hs - 2) // 2 + 1, (Ws - 2) // 2 + 1]."""
    return _strided("a2p_conv2d_down_ub", x, weight, bias, slope, None, None, False)


def conv_transpose2d_ub(x, weight, bias=None, *, slope=None, sigmoid_beta=None, skip=None):
    """One launch of a2p_conv_transpose2d_ub: la.ConvTranspose2dWNUB(C_in, C_out, 2 Hs, 2 Ws, 4, 2, 1), then + bias, then
    LeakyReLU(slope) or sigmoid(. + sigmoid_beta), then + skip [N, C_out, 2 Hs, 2 Ws].  weight [C_in, C_out, 4, 4] (PyTorch's
    transposed layout), already folded.  Returns [N, C_out, 2 Hs, 2 Ws]."""
    return _strided("a2p_conv_transpose2d_ub", x, weight, bias, slope, sigmoid_beta, skip, True)


def resize_bilinear(x, size):
    """F.interpolate(x, size, mode="bilinear", align_corners=False) of x [N, C, Hs, Ws], any ratio up or down: a new tensor."""
    x = gpu_f32(x, "x", "[N, C, Hs, Ws] with Hs, Ws >= 1", lambda s: len(s) == 4 and min(s[2:]) >= 1).contiguous()
    H, W = int(size[0]), int(size[1])
    if not (1 <= H <= _lib.CONV_MAX_SIZE and 1 <= W <= _lib.CONV_MAX_SIZE):
        raise A2PError(f"size {H} x {W} is outside [1, {_lib.CONV_MAX_SIZE}]")
    N, C, Hs, Ws = x.shape
    out = torch.empty(N, C, H, W, dtype=torch.float32, device=x.device)
    if N * C == 0:
        return out
    with _lib.on_device_of(x):
        _lib.check(_lib.load().a2p_resize_bilinear(_lib.ptr(x), N * C, Hs, Ws, H, W, _lib.ptr(out), _lib.current_stream(x.device)),
                   "a2p_resize_bilinear")
    return out


def compose_texture(t, u, tex_mean, tex_std, shadow=None):
    """One launch of a2p_texture_compose: ((resize_bilinear(t, 2x) + pixel_shuffle(u, 2)) * tex_std + tex_mean) * shadow.  t [N, C,
    Sh, Sw]; u [N, 4 C, Sh, Sw]; tex_mean [C, 2 Sh, 2 Sw] (or [1, C, ..]); tex_std a number; shadow [N or 1, 1, 2 Sh, 2 Sw] or None."""
    t = gpu_f32(t, "t", "[N, C, Sh, Sw]", lambda s: len(s) == 4 and min(s[1:]) >= 1).contiguous()
    N, C, Sh, Sw = t.shape
    dev = t.device
    u = operand(u, "u", f"[{N}, {4 * C}, {Sh}, {Sw}]", lambda s: s == (N, 4 * C, Sh, Sw), dev)
    tex_mean = operand(tex_mean, "tex_mean", f"[{C}, {2 * Sh}, {2 * Sw}]", lambda s: s in ((C, 2 * Sh, 2 * Sw), (1, C, 2 * Sh, 2 * Sw)), dev)
    frames = 0
    if shadow is not None:
        shadow = operand(shadow, "shadow", f"[{N} or 1, 1, {2 * Sh}, {2 * Sw}]",
                          lambda s: len(s) == 4 and s[0] in (1, N) and s[1:] == (1, 2 * Sh, 2 * Sw), dev)
        frames = shadow.shape[0]
    out = torch.empty(N, C, 2 * Sh, 2 * Sw, dtype=torch.float32, device=dev)
    if N == 0:
        return out
    with _lib.on_device_of(t):
        _lib.check(_lib.load().a2p_texture_compose(_lib.ptr(t), _lib.ptr(u), _lib.ptr(tex_mean), float(tex_std), _lib.ptr(shadow), frames,
                                                   N, C, Sh, Sw, _lib.ptr(out), _lib.current_stream(dev)), "a2p_texture_compose")
    return out


# ------------------------------------------------------------------------------------------------ the networks
def _positive(**values):
    for name, v in values.items():
        if not 1 <= int(v) <= _lib.CONV_MAX_CHANNELS:
            raise ValueError(f"{name}={v} is outside [1, {_lib.CONV_MAX_CHANNELS}]")


class ViewUNet(HostNet):
    """UNetWB(in_channels, out_channels, size, n_init_ftrs, out_scale) of nn/unet.py from the keys down1.0.weight_v / weight_g /
    bias ... down5.0.*, up1.0.* ... up5.0.*, out.* (a fused `weight` is accepted in place of a pair): five down launches, five
    transposed launches (up1 .. up4 add their skip inside the launch) and one conv2d_ub launch for `out` over cat([x, x1])."""

    def __init__(self, state_dict, in_channels: int = 4, out_channels: int = 3, size: int = 1024, n_init_ftrs: int = 8,
                 out_scale: float = 0.1, prefix: str = ""):
        _positive(in_channels=in_channels, out_channels=out_channels, n_init_ftrs=16 * int(n_init_ftrs))
        size, F = int(size), int(n_init_ftrs)
        if size < 32 or size % 32 or size > _lib.CONV_MAX_SIZE:
            raise ValueError(f"size={size}: need a multiple of 32 in [32, {_lib.CONV_MAX_SIZE}] (five halvings)")
        self.in_channels, self.out_channels, self.size, self.F, self.out_scale = int(in_channels), int(out_channels), size, F, float(out_scale)
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        ch = [self.in_channels, F, 2 * F, 4 * F, 8 * F, 16 * F]
        p = {}
        for i in range(1, 6):
            s = size >> i
            p[f"down{i}.0.weight"] = f32(folded_weight64(sd, f"down{i}.0", (ch[i], ch[i - 1], 4, 4)))
            p[f"down{i}.0.bias"] = checked(sd, f"down{i}.0.bias", (ch[i], s, s))
        up = [16 * F, 8 * F, 4 * F, 2 * F, F, F]
        for i in range(1, 6):
            s = size >> (5 - i)
            p[f"up{i}.0.weight"] = folded_weight_transposed(sd, f"up{i}.0", (up[i - 1], up[i], 4, 4))
            p[f"up{i}.0.bias"] = checked(sd, f"up{i}.0.bias", (up[i], s, s))
        w = folded_weight64(sd, "out", (self.out_channels, F + self.in_channels, 1, 1)) * self.out_scale
        p["out.weight_x"], p["out.weight_x1"] = f32(w[:, :F]), f32(w[:, F:, 0, 0])
        p["out.bias"] = f32(checked(sd, "out.bias", (self.out_channels, size, size)).astype(np.float64) * self.out_scale)
        self.params, self._dev = p, {}

    def activation_floats_per_frame(self) -> int:
        F, s = self.F, self.size
        n = sum(2 * (F << (i - 1)) * (s >> i) ** 2 for i in range(1, 6))      # x2 .. x6 and the four sums at the same sizes
        return n + (F + self.out_channels) * s * s

    def forward(self, x, keep=None):
        """x [N, in_channels, size, size] -> [N, out_channels, size, size]; `keep` (a dict) receives the intermediates down1 .. down5
        and up1 .. up5."""
        s = self.size
        x1 = gpu_f32(x, "x", f"[N, {self.in_channels}, {s}, {s}]", lambda sh: len(sh) == 4 and sh[1:] == (self.in_channels, s, s))
        t = self._tables(x1.device)
        downs = [x1]
        for i in range(1, 6):
            downs.append(conv2d_down_ub(downs[-1], t[f"down{i}.0.weight"], t[f"down{i}.0.bias"], slope=LRELU_SLOPE))
        h = downs[5]
        ups = []
        for i in range(1, 6):
            h = conv_transpose2d_ub(h, t[f"up{i}.0.weight"], t[f"up{i}.0.bias"], slope=LRELU_SLOPE, skip=downs[5 - i] if i < 5 else None)
            ups.append(h)
        if keep is not None:
            keep.update({f"down{i}": downs[i] for i in range(1, 6)})
            keep.update({f"up{i}": ups[i - 1] for i in range(1, 6)})
        return conv2d_ub(h, t["out.weight_x"], t["out.bias"], skip_src=x1, skip_weight=t["out.weight_x1"])

    __call__ = forward


class PoseShadow(HostNet):
    """PoseToShadow(n_pose_dims, uv_size, beta) of nn/shadow.py from fc_block.0.* and conv_block.0/2/4/6/8.*: the linear layer
    through conv2d_ub on a 1 x 1 plane, five transposed launches at 8 .. 128 (the last with the sigmoid), resize_bilinear."""
    LAYERS = ((0, 256, 256, 8), (2, 256, 128, 16), (4, 128, 128, 32), (6, 128, 64, 64), (8, 64, 1, 128))

    def __init__(self, state_dict, n_pose_dims: int, uv_size: int, beta: float = 1.0, prefix: str = ""):
        _positive(n_pose_dims=n_pose_dims)
        if not 1 <= int(uv_size) <= _lib.CONV_MAX_SIZE:
            raise ValueError(f"uv_size={uv_size} is outside [1, {_lib.CONV_MAX_SIZE}]")
        self.n_pose_dims, self.uv_size, self.beta = int(n_pose_dims), int(uv_size), float(beta)
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        p = {"fc_block.0.weight": f32(folded_weight64(sd, "fc_block.0", (256 * 4 * 4, self.n_pose_dims)))[:, :, None, None],
             "fc_block.0.bias": checked(sd, "fc_block.0.bias", (256 * 4 * 4,))}
        for i, cin, cout, s in self.LAYERS:
            p[f"conv_block.{i}.weight"] = folded_weight_transposed(sd, f"conv_block.{i}", (cin, cout, 4, 4))
            p[f"conv_block.{i}.bias"] = checked(sd, f"conv_block.{i}.bias", (cout, s, s))
        self.params, self._dev = p, {}

    def activation_floats_per_frame(self) -> int:
        return self.n_pose_dims + 4096 + sum(cout * s * s for _, _, cout, s in self.LAYERS) + self.uv_size ** 2

    def forward(self, motion, keep=None):
        """motion [N, n_pose_dims] -> shadow_map [N, 1, uv_size, uv_size]; `keep` receives shadow_map_lowres [N, 1, 128, 128]."""
        motion = gpu_f32(motion, "motion", f"[N, {self.n_pose_dims}]", lambda s: len(s) == 2 and s[1] == self.n_pose_dims).contiguous()
        t = self._tables(motion.device)
        x = conv2d_ub(motion[:, :, None, None], t["fc_block.0.weight"], t["fc_block.0.bias"], slope=LRELU_SLOPE)
        x = x.reshape(motion.shape[0], 256, 4, 4)
        for i, _, _, _ in self.LAYERS:
            last = i == 8
            x = conv_transpose2d_ub(x, t[f"conv_block.{i}.weight"], t[f"conv_block.{i}.bias"], slope=None if last else LRELU_SLOPE,
                                    sigmoid_beta=self.beta if last else None)
        if keep is not None:
            keep["shadow_map_lowres"] = x
        return resize_bilinear(x, (self.uv_size, self.uv_size))

    __call__ = forward


class UpscaleNet(HostNet):
    """UpscaleNet(in_channels, out_channels, n_ftrs, size, upscale_factor=2) of mesh_vae_drivable.py without its pixel shuffle
    (compose_texture applies it): conv_block.0 (k = 3, LeakyReLU) and out_block (k = 1), two conv2d_ub launches."""

    def __init__(self, state_dict, in_channels: int = 6, out_channels: int = 3, n_ftrs: int = 8, size: int = 1024, prefix: str = ""):
        _positive(in_channels=in_channels, out_channels=4 * int(out_channels), n_ftrs=n_ftrs)
        self.in_channels, self.out_channels, self.n_ftrs, self.size = int(in_channels), int(out_channels), int(n_ftrs), int(size)
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        s = self.size
        self.params = {"conv_block.0.weight": f32(folded_weight64(sd, "conv_block.0", (self.n_ftrs, self.in_channels, 3, 3))),
                       "conv_block.0.bias": checked(sd, "conv_block.0.bias", (self.n_ftrs, s, s)),
                       "out_block.weight": f32(folded_weight64(sd, "out_block", (4 * self.out_channels, self.n_ftrs, 1, 1))),
                       "out_block.bias": checked(sd, "out_block.bias", (4 * self.out_channels, s, s))}
        self._dev = {}

    def activation_floats_per_frame(self) -> int:
        return (self.in_channels + self.n_ftrs + 4 * self.out_channels) * self.size ** 2

    def forward(self, x):
        """x [N, in_channels, size, size] -> out_block's output [N, 4 out_channels, size, size], BEFORE the pixel shuffle."""
        t = self._tables(x.device)
        h = conv2d_ub(x, t["conv_block.0.weight"], t["conv_block.0.bias"], slope=LRELU_SLOPE)
        return conv2d_ub(h, t["out_block.weight"], t["out_block.bias"])

    __call__ = forward


# ------------------------------------------------------------------------------------------------ the texture
def forward_tex(upscale_net: UpscaleNet, seam_sampler: SeamSampler, seam_sampler_2k: SeamSampler, tex_mean, tex_std: float, tex_mean_rec,
                tex_view_rec, shadow_map=None):
    """AutoEncoder.forward_tex in the reference's order: t = tex_mean_rec + tex_view_rec (a torch add), impaint and resample at S;
    the two UpscaleNet launches on cat([tex_mean_rec, tex_view_rec]); impaint and two resamples of the shadow map at 2 S; one
    compose_texture; impaint and two resamples of the result.  tex_mean_rec, tex_view_rec [N, C, S, S]; tex_mean [C, 2 S, 2 S] on the
    GPU; shadow_map [N or 1, 1, 2 S, 2 S] or None (no shadow).  No input is modified.  Returns [N, C, 2 S, 2 S]."""
    S = seam_sampler.H
    tex_mean_rec = gpu_f32(tex_mean_rec, "tex_mean_rec", f"[N, C, {S}, {S}]", lambda s: len(s) == 4 and s[2:] == (S, S))
    N, C = tex_mean_rec.shape[:2]
    tex_view_rec = gpu_f32(tex_view_rec, "tex_view_rec", f"[{N}, {C}, {S}, {S}]", lambda s: s == (N, C, S, S))
    k = seam_sampler_2k
    with _lib.on_device_of(tex_mean_rec):
        t = seam_sampler.resample(seam_sampler.impaint(tex_mean_rec + tex_view_rec))
        u = upscale_net(torch.cat([tex_mean_rec, tex_view_rec], dim=1))
        if shadow_map is not None:
            shadow_map = gpu_f32(shadow_map, "shadow_map", f"[{N} or 1, 1, {2 * S}, {2 * S}]",
                                  lambda s: len(s) == 4 and s[0] in (1, N) and s[1:] == (1, 2 * S, 2 * S))
            shadow_map = k.resample(k.resample(k.impaint(shadow_map.clone())))
        tex = compose_texture(t, u, tex_mean, tex_std, shadow_map)
        return k.resample(k.resample(k.impaint(tex)))


class BodyTexture(HostNet):
    """The texture half of AutoEncoder.forward: UNetViewDecoder, PoseToShadow, UpscaleNet and forward_tex."""

    @classmethod
    def from_state_dict(cls, state_dict, assets, surface, *, uv_size: int = 1024, n_init_ftrs: int = 8, upscale_n_ftrs: int = 8,
                        pose_to_shadow_dims: int = 104, shadow_beta: float = 1.0, prefix: str = "") -> "BodyTexture":
        """state_dict: the reference's keys under `prefix`: decoder_view.unet.*, upscale_net.*, pose_to_shadow.* (optional: without
        them the shadow is the caller's shadow_map, or 1) and the buffer tex_mean [1, 3, 2 uv_size, 2 uv_size] (optional: without it
        prepare_tex_mean(assets["tex_mean"], 2 uv_size)).  assets: seam_data_1024 and seam_data_2048 (the seam tables at uv_size and
        2 uv_size, whatever their names say), tex_var (optional, default 64.0; the reference's tex_std) and tex_mean.  surface: the
        surface.BodySurface (uv_size texels) whose view_cos and to_uv condition the view network.  The reference's configuration of
        upscale_n_ftrs and pose_to_shadow_dims is not part of its tree: pass the checkpoint's own."""
        self = object.__new__(cls)
        S = int(uv_size)
        if surface.uv_size != S:
            raise ValueError(f"the surface maps to {surface.uv_size} texels; uv_size={S}")
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        self.uv_size, self.surface = S, surface
        self.view_net = ViewUNet(sd, 4, 3, S, n_init_ftrs, 0.1, prefix="decoder_view.unet.")
        self.upscale_net = UpscaleNet(sd, 6, 3, upscale_n_ftrs, S, prefix="upscale_net.")
        self.pose_shadow = None
        if any(k.startswith("pose_to_shadow.") for k in sd):
            self.pose_shadow = PoseShadow(sd, pose_to_shadow_dims, 2 * S, shadow_beta, prefix="pose_to_shadow.")
        if "tex_mean" in sd:
            self.tex_mean = checked(sd, "tex_mean", (1, 3, 2 * S, 2 * S))[0]
        else:
            self.tex_mean = prepare_tex_mean(asset(assets, "tex_mean"), 2 * S)[0]
            if self.tex_mean.shape[0] != 3:
                raise ValueError(f"assets `tex_mean` has {self.tex_mean.shape[0]} channels; the texture has 3")
        self.tex_std = 64.0
        if (hasattr(assets, "keys") and "tex_var" in assets) or (not hasattr(assets, "keys") and hasattr(assets, "tex_var")):
            var = as_numpy(asset(assets, "tex_var"))
            if var.size != 1:
                raise ValueError(f"assets `tex_var` has shape {list(var.shape)}; the configuration expects a scalar")
            self.tex_std = float(var.reshape(()))
        if not np.isfinite(self.tex_std):
            raise ValueError(f"assets `tex_var` is not finite ({self.tex_std})")
        self.seam_sampler, self.seam_sampler_2k = SeamSampler(asset(assets, "seam_data_1024")), SeamSampler(asset(assets, "seam_data_2048"))
        for key, seam, side in (("seam_data_1024", self.seam_sampler, S), ("seam_data_2048", self.seam_sampler_2k, 2 * S)):
            if (seam.H, seam.W) != (side, side):
                raise ValueError(f"assets `{key}` is for {seam.H} x {seam.W} maps; the configuration expects {side} x {side}")
        self.params, self._dev = {"tex_mean": self.tex_mean}, {}
        return self

    def _tex_mean(self, device):
        return self._tables(device)["tex_mean"]

    def activation_bytes_per_frame(self) -> int:
        """An upper bound of the bytes one frame's forward allocates (every intermediate counted as if none were freed)."""
        S = self.uv_size
        n = self.surface.V + 5 * S * S + self.view_net.activation_floats_per_frame()       # view cosine, its map, cond_view
        n += 3 * 3 * S * S + self.upscale_net.activation_floats_per_frame()                 # the sum and its two seam steps
        n += (self.pose_shadow.activation_floats_per_frame() if self.pose_shadow else 0) + 2 * 4 * S * S    # shadow and its resamples
        return 4 * (n + 3 * 3 * 4 * S * S)                                                  # compose and two resamples at 2 S

    def forward_tex(self, tex_mean_rec, tex_view_rec, shadow_map=None):
        """forward_tex (below) with this object's networks, seam tables, tex_mean and tex_std."""
        S = self.uv_size
        tex_mean_rec = gpu_f32(tex_mean_rec, "tex_mean_rec", f"[N, 3, {S}, {S}]", lambda s: len(s) == 4 and s[1:] == (3, S, S))
        return forward_tex(self.upscale_net, self.seam_sampler, self.seam_sampler_2k, self._tex_mean(tex_mean_rec.device), self.tex_std,
                           tex_mean_rec, tex_view_rec, shadow_map)

    def forward(self, geom, tex_mean_rec, camera_pos, motion=None, shadow_map=None) -> dict:
        """geom [N, V, 3] (posed vertices), tex_mean_rec [N, 3, S, S], camera_pos [N or 1, 3]; the shadow map comes from
        PoseShadow(motion [N, pose_to_shadow_dims]) or is the caller's shadow_map [N or 1, 1, 2 S, 2 S], or neither (then it is 1
        and the returned shadow_map None).  Returns tex_rec [N, 3, 2 S, 2 S], tex_view_rec, cond_view [N, 4, S, S] and shadow_map
        (as used, before its seam steps)."""
        if motion is not None and shadow_map is not None:
            raise A2PError("pass motion (for PoseToShadow) or shadow_map, not both")
        if motion is not None and self.pose_shadow is None:
            raise A2PError("motion was given but the state dict held no pose_to_shadow.* weights")
        S = self.uv_size
        tex_mean_rec = gpu_f32(tex_mean_rec, "tex_mean_rec", f"[N, 3, {S}, {S}]", lambda s: len(s) == 4 and s[1:] == (3, S, S))
        with _lib.on_device_of(tex_mean_rec):
            view_cos_uv = self.surface.to_uv(self.surface.view_cos(geom, camera_pos)[..., None])
            cond_view = torch.cat([view_cos_uv, tex_mean_rec], dim=1)
            tex_view_rec = self.view_net(cond_view)
            if motion is not None:
                shadow_map = self.pose_shadow(motion)
            tex_rec = self.forward_tex(tex_mean_rec, tex_view_rec, shadow_map)
        return {"tex_rec": tex_rec, "tex_view_rec": tex_view_rec, "cond_view": cond_view, "shadow_map": shadow_map}

    __call__ = forward


# ------------------------------------------------------------------------------------------------ frames
def linear_to_display(rgb):
    """linear2displayBatch(rgb, mode="srgb") of utils/image.py on [.., 3, H, W]: white balance [1.05, 0.95, 1.45] on rgb / 255,
    minus black 5 / 255, the sRGB curve with gamma 1.5, clamped to [0, 1], times 255.  Torch ops on the rendered image: one pass
    over H x W pixels, not a hot path."""
    if not torch.is_tensor(rgb) or rgb.dim() < 3 or rgb.shape[-3] != 3:
        raise A2PError("rgb must be a tensor [.., 3, H, W]")
    wb = torch.tensor(WB_SCALE, dtype=torch.float32, device=rgb.device)[:, None, None]
    v = rgb.float() / 255.0 * wb - DISPLAY_BLACK
    curve = 1.055 * torch.pow(torch.clamp(v, min=0.0031308), 1.0 / DISPLAY_GAMMA) - 0.055
    return torch.clamp(torch.where(v <= 0.0031308, v * 12.92, curve), 0, 1) * 255.0


def display_to_linear(rgb):
    """The inverse of linear_to_display on display values in [0, 255], [.., 3, H, W]: the inverse of the sRGB-type curve with gamma
    1.5 (its linear piece below 12.92 x 0.0031308), plus black, divided by the white balance, times 255.  linear_to_display of
    the result gives rgb back to float32 rounding.  Torch ops, not a hot path: a background is converted once."""
    if not torch.is_tensor(rgb) or rgb.dim() < 3 or rgb.shape[-3] != 3:
        raise A2PError("rgb must be a tensor [.., 3, H, W]")
    wb = torch.tensor(WB_SCALE, dtype=torch.float32, device=rgb.device)[:, None, None]
    y = rgb.float() / 255.0
    curve = torch.pow((torch.clamp(y, min=0.0) + 0.055) / 1.055, DISPLAY_GAMMA)
    v = torch.where(y <= 12.92 * 0.0031308, y / 12.92, curve)
    return (v + DISPLAY_BLACK) / wb * 255.0


def display_background(background, height: int, width: int, device=None):
    """A display-space background -- three numbers, [3, H, W] or [H, W, 3], in [0, 255] -- as (display [3, 1, 1] or [3, H, W],
    linear [3] or [1, 3, H, W]) float32 tensors on `device`: the second is display_to_linear of the first, what
    BodyRasterizer.render_antialiased composites under the linear image.  None gives (None, None)."""
    if background is None:
        return None, None
    try:
        x = torch.as_tensor(np.asarray(background.detach().cpu() if torch.is_tensor(background) else background, np.float32))
    except (TypeError, ValueError):
        raise ValueError(f"background must be three numbers or an image in [0, 255] (got {type(background).__name__})") from None
    H, W = int(height), int(width)
    if tuple(x.shape) == (3,):
        x = x.reshape(3, 1, 1)
    elif tuple(x.shape) == (H, W, 3) and tuple(x.shape) != (3, H, W):
        x = x.permute(2, 0, 1)
    elif tuple(x.shape) != (3, H, W):
        raise ValueError(f"background must be three numbers, [3, {H}, {W}] or [{H}, {W}, 3] (got {list(x.shape)})")
    if not bool(((x >= 0) & (x <= 255)).all()):
        raise ValueError("background must hold display values in [0, 255]")
    x = x.contiguous().to(device or "cpu")
    linear = display_to_linear(x)
    return x, (linear.reshape(3) if x.shape[1:] == (1, 1) else linear[None].contiguous())


def display_frames(rasterizer, verts, tex, K, Rt, supersample: int = 1, background=(None, None)):
    """Display RGB [N, 3, H, W] of one camera: rasterizer.render and linear_to_display; with supersample > 1 or a background (the
    pair display_background returns) render_antialiased, composited in linear light, then linear_to_display, and finally every
    pixel no sample covers is set to the given display value itself."""
    shown, linear = background
    if supersample == 1 and shown is None:
        return linear_to_display(rasterizer.render(verts, tex, K, Rt)["render"])
    got = rasterizer.render_antialiased(verts, tex, K, Rt, supersample, linear)
    image = linear_to_display(got["render"])
    return image if shown is None else torch.where(got["alpha"] == 0, shown, image)


def render_rgb_motion(decoder, texture: BodyTexture, skeleton, rasterizer, poses, embs, face_embs, K, Rt, camera_pos=None,
                      max_bytes: int = 1 << 30, supersample: int = 1, background=None):
    """Display RGB frames [B, T, 3, H, W] (or [N, 3, H, W] for flat frames; float32 in [0, 255] on the GPU) of un-normalised body
    motion in the layouts decoder.decode_motion takes, with embs and face_embs on the same leading axes: per chunk of frames
    BodyDecoder.forward, skeleton.pose_vertices, BodyTexture.forward (motion = the chunk's poses when the texture has PoseToShadow
    weights), rasterizer.render and linear_to_display.  K / Rt are [N or 1, 3, .]; camera_pos [N or 1, 3] defaults to
    render.camera_centre(Rt).  Only the images are kept (a 2048 x 2048 texture is 50 MB a frame); a chunk's activations
    (activation_bytes_per_frame of decoder and texture) stay under max_bytes, at least one frame; a frame's result does not depend
    on the chunking.

    supersample = s > 1 anti-aliases with s x s samples per pixel (rasterizer.render_antialiased).  background: a display-space
    colour (three numbers) or image ([H, W, 3] or [3, H, W]) in [0, 255]; it is converted once by display_to_linear, composited
    under the avatar in linear light, where coverage is a fraction of light, and passed through linear_to_display with it; a
    pixel no sample covers holds the given value itself.  With the defaults the calls are those made without the two keywords."""
    from .render import camera_centre
    supersample = rasterizer._supersample(supersample)
    background = display_background(background, rasterizer.height, rasterizer.width)
    avatar.check_pose_width(skeleton, decoder)
    frames, lead = avatar.clip_frames("render_rgb_motion", poses, skeleton.P_pos)
    N, dev = frames.shape[0], frames.device
    embs = avatar.per_frame(embs, "embs", lead, (decoder.n_embs,), dev)
    face_embs = avatar.per_frame(face_embs, "face_embs", lead, (decoder.n_face_embs,), dev)
    K, k_per = rasterizer._camera(K, "K", 3, N, dev)
    Rt, rt_per = rasterizer._camera(Rt, "Rt", 4, N, dev)
    camera_pos = camera_centre(Rt) if camera_pos is None else torch.as_tensor(camera_pos).to(device=dev, dtype=torch.float32).reshape(-1, 3)
    if camera_pos.shape[0] not in (1, N):
        raise A2PError(f"camera_pos must be [{N} or 1, 3] (got {list(camera_pos.shape)})")
    cam_per = camera_pos.shape[0] == N and N != 1
    H, W = rasterizer.height, rasterizer.width
    background = tuple(None if x is None else x.to(dev) for x in background)
    out = torch.empty(N, 3, H, W, dtype=torch.float32, device=dev)
    for a, b in avatar.frame_chunks(N, max_bytes, decoder.activation_bytes_per_frame() + texture.activation_bytes_per_frame()):
        part = lambda x, per: x[a:b] if per else x
        preds, verts = avatar.decode_and_pose(decoder, skeleton, frames[a:b], embs[a:b], face_embs[a:b])
        tex = texture.forward(verts, preds["tex_mean_rec"], part(camera_pos, cam_per),
                              motion=frames[a:b] if texture.pose_shadow is not None else None)
        out[a:b] = display_frames(rasterizer, verts, tex["tex_rec"], part(K, k_per), part(Rt, rt_per), supersample, background)
    return out.reshape(*lead, 3, H, W)


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m audio2photoreal_amd.texture", description="Display RGB frames of the motions of a results.npy.")
    ap.add_argument("--results", required=True, help="results.npy of sample.generate (key `motions` [B, P, 1, T], un-normalised)")
    ap.add_argument("--embeddings", required=True, help=".npz with `embs` [B, T, n_embs] and `face_embs` [B, T, n_face_embs]")
    ap.add_argument("--assets", required=True, help="static_assets.pt: topology, the skinning model, the decoder's masks, tex_mean, both seam tables")
    ap.add_argument("--checkpoint", required=True, help="the body model's state dict (decoder.*, decoder_view.*, upscale_net.*, ...)")
    ap.add_argument("--out", required=True, help="frames.npy: a float32 array [B, T, 3, H, W] in [0, 255]")
    avatar.add_camera_arguments(ap)
    avatar.add_render_arguments(ap, png="rgb")
    avatar.add_network_arguments(ap)
    return ap


def main(argv=None) -> int:
    from . import render as R
    args = parser().parse_args(argv)
    motions, embs, face_embs = avatar.load_motion_clip(args.results, args.embeddings, args.frames)
    avatar.require_gpu("the frames are rendered")
    person = avatar.load_avatar(args.assets, args.checkpoint, args)
    H, W = args.size
    poses = torch.from_numpy(motions).to("cuda")
    rest = person.skeleton.pose_vertices(poses.reshape(-1, poses.shape[-1])[:1]).cpu().numpy()  # frames the default camera
    K, Rt = R._camera_from_args(args, rest, H, W)
    rgb = render_rgb_motion(person.decoder, person.texture, person.skeleton, R.BodyRasterizer(person.surface, H, W), poses, embs, face_embs,
                            K.to("cuda"), Rt.to("cuda"), max_bytes=args.max_bytes, supersample=args.supersample,
                            background=args.background).cpu().numpy()
    np.save(args.out, rgb)
    print(f"{args.out}: rgb {list(rgb.shape)}")
    if args.png_dir is not None:                                              # rounded here: write_pngs writes a uint8 image as it is
        count = R.write_pngs({"rgb": np.clip(np.rint(rgb), 0, 255).astype(np.uint8)}, args.png_dir)
        print(f"{args.png_dir}: {count} png files")
    return 0


if __name__ == "__main__":
    sys.exit(main())
