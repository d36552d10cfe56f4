"""Decoded body geometry and mean texture on the MI355X: the reference's ConvDecoder (visualize/ca_body/models/mesh_vae_drivable.py)
and the layer family it is made of -- the weight-normalised convolution with an untied bias, la.Conv2dWNUB, inside the residual
blocks ConvBlock and UpConvBlockDeep of nn/blocks.py, and the SeamSampler of utils/seams.py -- as HIP launches for all frames
(csrc/kernels_conv.h).

    python -m audio2photoreal_amd.decoder --results results.npy --embeddings embs.npz --assets static_assets.pt
                                          --checkpoint body_dec.ckpt --out decoded.npy [--frames A:B] [--max-bytes B]

`conv2d_ub` is one launch of the layer: convolution (k = 1 or 3, groups) of a source that may be read through bilinear upsampling,
bias (tied or untied), LeakyReLU, a skip operand (a tensor, or the 1 x 1 convolution of a second source) and a per-pixel mask.  A
ConvBlock and an UpConvBlockDeep are two launches each; neither the upsampled input nor the skip branch is written to memory.
`SeamSampler` is the reference's; `BodyDecoder` is ConvDecoder, built once from the reference's state dict; `decode_motion` feeds
its geometry to skinning.BodySkeleton.  Everything takes float32 tensors that live on the GPU and runs on the caller's current
stream; there is no CPU path.

Differences from the reference, on purpose:
  * the weight normalisation w = v g / ||v|| is folded once at construction, in float64, and rounded to float32 once (the
    reference recomputes it in float32 in every forward);
  * `SeamSampler.impaint` reads every source from the tensor as it was before the call, and of several pairs with the same
    destination the last in the list wins (the reference's indexed assignment leaves both to the backend);
  * `BodyDecoder.forward` does not modify a passed `embs_conv`: the merged map it returns is a new tensor."""
from __future__ import annotations

import argparse
import ctypes
import sys

import numpy as np
import torch

from . import _lib, avatar
from ._lib import A2PError
from .avatar import HostNet, as_numpy, asset, checked, gpu_f32, source

LRELU_SLOPE = 0.2
ASSET_KEYS = ("pose_cond_mask", "head_cond_mask", "face_cond_mask", "body_cond_mask", "seam_data_1024")


# ------------------------------------------------------------------------------------------------ host preparation
def fold_weight_norm(weight_v, weight_g) -> np.ndarray:
    """float32 w = weight_v * (weight_g / ||weight_v||): weight_norm_wrapper(..., g_dim=0, v_dim=None), whose norm runs over the
    WHOLE weight_v tensor; weight_g is [C_out, 1, ...].  Computed in float64 and rounded once."""
    v, g = as_numpy(weight_v).astype(np.float64), as_numpy(weight_g).astype(np.float64)
    return np.ascontiguousarray(v * (g / np.sqrt((v * v).sum())), np.float32)


def folded_weight(state_dict, name: str, shape) -> np.ndarray:
    """The float32 weight of layer `name` ("...conv1"): `name.weight` when the state dict holds the fused tensor, else the fold of
    `name.weight_g` / `name.weight_v`.  A missing key or a shape other than `shape` is a ValueError naming it."""
    shape = tuple(int(s) for s in shape)
    g_shape = (shape[0],) + (1,) * (len(shape) - 1)
    if f"{name}.weight" in state_dict:
        return checked(state_dict, f"{name}.weight", shape)
    v, g = checked(state_dict, f"{name}.weight_v", shape), checked(state_dict, f"{name}.weight_g", g_shape)
    return fold_weight_norm(v, g)


def resolve_seam_pairs(dst_ij, src_ij, H: int, W: int):
    """(dst, src) int64 flat texel indices i W + j of the pairs impaint applies: every (row, column) checked against [0, H) x
    [0, W), and of several pairs with the same destination only the last in the list kept (in its place in the list).  Sources
    are read before any destination is written, so a chain a -> b, b -> c gives c the original b."""
    flat = []
    for name, a in (("dst_ij", dst_ij), ("src_ij", src_ij)):
        a = as_numpy(a)
        if a.ndim != 2 or a.shape[1] != 2 or not (np.issubdtype(a.dtype, np.integer) or a.size == 0):
            raise ValueError(f"{name} must be an integer array [P, 2] (got {a.dtype} {list(a.shape)})")
        a = a.astype(np.int64)
        bad = np.argwhere((a < 0) | (a >= np.array([H, W])))
        if bad.size:
            p, k = map(int, bad[0])
            raise ValueError(f"{name}[{p}, {k}] = {int(a[p, k])} is outside [0, {'HW'[k]}={(H, W)[k]})")
        flat.append(a[:, 0] * W + a[:, 1])
    dst, src = flat
    if dst.shape != src.shape:
        raise ValueError(f"dst_ij holds {dst.size} pairs and src_ij {src.size}")
    _, first_from_end = np.unique(dst[::-1], return_index=True)               # the last occurrence of every destination
    keep = np.sort(dst.size - 1 - first_from_end)
    return dst[keep], src[keep]


# ------------------------------------------------------------------------------------------------ the seam sampler
class SeamSampler(HostNet):
    """SeamSampler(seam_data) of utils/seams.py: seam_data holds dst_ij / src_ij [P, 2] (row, column), uvs [H, W, 2] and weights
    [H, W] or [H, W, 1].  The pair list is resolved on the host here (resolve_seam_pairs); device copies are made on first use."""

    def __init__(self, seam_data):
        uvs, weights = as_numpy(seam_data["uvs"]), as_numpy(seam_data["weights"])
        if uvs.ndim != 3 or uvs.shape[2] != 2 or min(uvs.shape[:2]) < 1:
            raise ValueError(f"uvs must be [H, W, 2] (got {list(uvs.shape)})")
        self.H, self.W = int(uvs.shape[0]), int(uvs.shape[1])
        if max(self.H, self.W) > _lib.CONV_MAX_SIZE:
            raise ValueError(f"uvs is {self.H} x {self.W}; a side is at most {_lib.CONV_MAX_SIZE}")
        if tuple(weights.shape) not in ((self.H, self.W), (self.H, self.W, 1)):
            raise ValueError(f"weights must be [{self.H}, {self.W}] or [{self.H}, {self.W}, 1] (got {list(weights.shape)})")
        for name, a in (("uvs", uvs), ("weights", weights)):
            bad = np.argwhere(~np.isfinite(a))
            if bad.size:
                raise ValueError(f"{name}{list(map(int, bad[0]))} is not finite ({a[tuple(bad[0])]})")
        self.uvs = np.ascontiguousarray(uvs, np.float32)
        self.weights = np.ascontiguousarray(weights.reshape(self.H, self.W), np.float32)
        self.dst, self.src = resolve_seam_pairs(seam_data["dst_ij"], seam_data["src_ij"], self.H, self.W)
        self.P = int(self.dst.size)
        self.params = {"dst": self.dst.astype(np.int32), "src": self.src.astype(np.int32), "uvs": self.uvs, "weights": self.weights}
        self._dev = {}

    def _value(self, value, name):
        return gpu_f32(value, name, f"[N, C, {self.H}, {self.W}]", lambda s: len(s) == 4 and s[2:] == (self.H, self.W))

    def impaint(self, value):
        """value[:, :, dst] = (value before the call)[:, :, src], IN PLACE like the reference (value must be contiguous); returns
        value."""
        value = self._value(value, "value")
        if not value.is_contiguous():
            raise A2PError("impaint writes in place: value must be contiguous")
        planes = value.shape[0] * value.shape[1]
        if planes == 0 or self.P == 0:
            return value
        t = self._tables(value.device)
        scratch = torch.empty(planes * self.P, dtype=torch.float32, device=value.device)
        with _lib.on_device_of(value):
            _lib.check(_lib.load().a2p_seam_impaint(_lib.ptr(value), planes, self.H, self.W, _lib.ptr(t["dst"]), _lib.ptr(t["src"]),
                                                    self.P, _lib.ptr(scratch), _lib.current_stream(value.device)), "a2p_seam_impaint")
        return value

    def resample(self, tex):
        """(1 - w) tex + w grid_sample(tex, 2 (uvs - 0.5), bilinear, align_corners=False, padding_mode="border"): a new tensor."""
        tex = self._value(tex, "tex").contiguous()
        out = torch.empty_like(tex)
        planes = tex.shape[0] * tex.shape[1]
        if planes == 0:
            return out
        t = self._tables(tex.device)
        with _lib.on_device_of(tex):
            _lib.check(_lib.load().a2p_seam_resample(_lib.ptr(tex), planes, self.H, self.W, _lib.ptr(t["uvs"]), _lib.ptr(t["weights"]),
                                                     _lib.ptr(out), _lib.current_stream(tex.device)), "a2p_seam_resample")
        return out

    def __call__(self, tex):
        """SeamSampler.forward: impaint (in place), then resample."""
        return self.resample(self.impaint(tex))


# ------------------------------------------------------------------------------------------------ the layer
def conv2d_ub(x, weight, bias=None, *, groups: int = 1, size=None, slope=None, skip=None, skip_src=None, skip_weight=None,
              skip_bias=None, mask=None):
    """One launch of the decoder layer (a2p_conv2d_ub): out [N, C_out, H, W] =
        (lrelu(conv(up(x), weight) + bias, slope) + skip) * mask
    x [N, C_in, Hs, Ws]; size = (H, W) reads x through nn.UpsamplingBilinear2d(size) (default: x's own size, read directly);
    weight [C_out, C_in / groups, k, k] with k = 1 or 3 (stride 1, zero padding k // 2), already folded; bias [C_out] (tied),
    [C_out, H, W] (untied) or None; slope None = no activation; skip [N, C_out, H, W], or skip_src [N, C_s, Hs', Ws'] with
    skip_weight [C_out, C_s / groups] (or [.., 1, 1]) and skip_bias [C_out] or None -- the 1 x 1 convolution, with the same
    groups, of a second source that is upsampled the same way; mask [H, W] or None.  At most 4096 channels per group."""
    keep = []
    x, xs = source(x, "x")
    N, C_in, Hs, Ws = x.shape
    dev = x.device
    H, W = (Hs, Ws) if size is None else (int(size[0]), int(size[1]))

    def operand(t, name, shape_text, ok):
        t = gpu_f32(t, name, shape_text, ok)
        if t.device != dev:
            raise A2PError(f"{name} is on {t.device}, x on {dev}")
        t = t.contiguous()
        keep.append(t)
        return t

    weight = operand(weight, "weight", "[C_out, C_in / groups, k, k]", lambda s: len(s) == 4 and s[2] == s[3])
    C_out, k = weight.shape[0], weight.shape[2]
    if groups < 1 or C_in % groups or C_out % groups or weight.shape[1] != C_in // groups:
        raise A2PError(f"weight {list(weight.shape)} does not fit C_in={C_in}, groups={groups}: need [C_out, {C_in}/groups, k, k] "
                       "with C_in and C_out multiples of groups")
    d = _lib.A2PConv2dDesc()
    d.x, d.weight, d.N, d.C_out, d.H, d.W, d.k, d.groups = xs, _lib.ptr(weight), N, C_out, H, W, k, groups
    if bias is not None:
        bias = operand(bias, "bias", f"[{C_out}] or [{C_out}, {H}, {W}]", lambda s: s in ((C_out,), (C_out, H, W)))
        d.bias, d.bias_mode = _lib.ptr(bias), _lib.CONV_BIAS_TIED if bias.dim() == 1 else _lib.CONV_BIAS_UNTIED
    if slope is not None:
        d.act, d.slope = 1, float(slope)
    if skip is not None and skip_src is not None:
        raise A2PError("pass skip (a tensor) or skip_src (a source to convolve), not both")
    if skip is not None:
        skip = operand(skip, "skip", f"[{N}, {C_out}, {H}, {W}]", lambda s: s == (N, C_out, H, W))
        d.skip, d.skip_mode = _lib.ptr(skip), _lib.CONV_SKIP_TENSOR
    if skip_src is not None:
        skip_src, ss = source(skip_src, "skip_src")
        keep.append(skip_src)
        C_s = skip_src.shape[1]
        if skip_src.shape[0] != N or skip_src.device != dev or C_s % groups:
            raise A2PError(f"skip_src {list(skip_src.shape)} on {skip_src.device}: need {N} frames on {dev} and channels a multiple of groups={groups}")
        if skip_weight is None:
            raise A2PError("skip_src needs skip_weight")
        skip_weight = operand(skip_weight, "skip_weight", f"[{C_out}, {C_s // groups}] or [{C_out}, {C_s // groups}, 1, 1]",
                              lambda s: s in ((C_out, C_s // groups), (C_out, C_s // groups, 1, 1)))
        d.skip_src, d.skip_weight, d.skip_mode = ss, _lib.ptr(skip_weight), _lib.CONV_SKIP_CONV
        if skip_bias is not None:
            d.skip_bias = _lib.ptr(operand(skip_bias, "skip_bias", f"[{C_out}]", lambda s: s == (C_out,)))
    if mask is not None:
        d.mask = _lib.ptr(operand(mask, "mask", f"[{H}, {W}]", lambda s: s == (H, W)))
    out = torch.empty(N, C_out, H, W, dtype=torch.float32, device=dev)
    d.out = _lib.ptr(out)
    if N == 0:
        return out
    with _lib.on_device_of(x):
        _lib.check(_lib.load().a2p_conv2d_ub(ctypes.byref(d), _lib.current_stream(dev)), "a2p_conv2d_ub")
    return out


# ------------------------------------------------------------------------------------------------ the decoder
class BodyDecoder(HostNet):
    """ConvDecoder of mesh_vae_drivable.py: pose, embedding and face embedding to the UV displacement of the unposed mesh and the
    mean texture.  Host arrays (folded float32 weights under the reference's key names, `name.weight` / `name.bias`) live on the
    object in `params`; device copies are made on first use, per device."""

    @classmethod
    def from_state_dict(cls, state_dict, assets, surface, prefix: str = "decoder.", uv_size: int = 1024, init_uv_size: int = 64,
                        n_pose_dims: int = 98, n_pose_enc_channels: int = 16, n_embs: int = 1024, n_embs_enc_channels: int = 32,
                        n_face_embs: int = 256, n_init_channels: int = 64, n_min_channels: int = 4) -> "BodyDecoder":
        """state_dict: the reference's keys under `prefix` (local_pose_conv_block.conv1.weight_v, conv_blocks.3.conv2.bias,
        embs_fc.0.weight_g, ...; a fused `weight` is accepted in place of a `_g` / `_v` pair).  assets: pose_cond_mask
        [n_pose_dims, S, S], head_cond_mask, face_cond_mask, body_cond_mask [S, S] with S = init_uv_size, and seam_data_1024 (the
        seam table at uv_size, whatever its name says).  surface: the surface.BodySurface whose from_uv turns the UV displacement
        into vertices.  Every shape is checked against the configuration."""
        self = object.__new__(cls)
        if int(init_uv_size) != 64:
            raise ValueError(f"init_uv_size={init_uv_size}: only 64 is supported (the reference's merge of the face features "
                             "hard-codes the 32-texel quadrant [32:, :32])")
        n_blocks = int(np.log2(int(uv_size) // 64)) if int(uv_size) >= 64 else -1
        if n_blocks < 0 or 64 * 2 ** n_blocks != int(uv_size) or uv_size > _lib.CONV_MAX_SIZE:
            raise ValueError(f"uv_size={uv_size}: need 64 times a power of two, at most {_lib.CONV_MAX_SIZE}")
        for name, v in (("n_pose_dims", n_pose_dims), ("n_pose_enc_channels", n_pose_enc_channels), ("n_embs", n_embs),
                        ("n_embs_enc_channels", n_embs_enc_channels), ("n_face_embs", n_face_embs), ("n_init_channels", n_init_channels),
                        ("n_min_channels", n_min_channels)):
            if not 1 <= int(v) <= _lib.CONV_MAX_CHANNELS:
                raise ValueError(f"{name}={v} is outside [1, {_lib.CONV_MAX_CHANNELS}]")
        self.uv_size, self.init_uv_size, self.n_blocks = int(uv_size), 64, n_blocks
        self.n_pose_dims, self.n_pose_enc_channels, self.n_embs = int(n_pose_dims), int(n_pose_enc_channels), int(n_embs)
        self.n_embs_enc_channels, self.n_face_embs = int(n_embs_enc_channels), int(n_face_embs)
        self.sizes = [64 * 2 ** s for s in range(n_blocks + 1)]
        self.n_channels = [max(int(n_init_channels) // 2 ** b, int(n_min_channels)) for b in range(n_blocks + 1)]
        self.surface = surface
        E, S, C = self.n_embs_enc_channels, 64, self.n_channels
        # (name, C_in, C_out, size, k, groups): the residual blocks in forward order
        self.embs_blocks = [("embs_conv_block.0", 128, 128, 8, 3, 1), ("embs_conv_block.1", 128, 128, 16, 3, 1),
                            ("embs_conv_block.2", 128, 64, 32, 3, 1), ("embs_conv_block.3", 64, E, 64, 3, 1)]
        self.face_blocks = [("face_embs_conv_block.0", 32, 64, 8, 3, 1), ("face_embs_conv_block.1", 64, 64, 16, 3, 1),
                            ("face_embs_conv_block.2", 64, E, 32, 3, 1)]
        self.pose_block = ("local_pose_conv_block", self.n_pose_dims, self.n_pose_enc_channels, S, 1, 1)
        self.joint_block = ("joint_conv_block", self.n_pose_enc_channels + E, C[0], S, 3, 1)
        self.up_blocks = [(f"conv_blocks.{b}", 2 * C[b], 2 * C[b + 1], self.sizes[b + 1], 3, 2) for b in range(n_blocks)]

        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        p = {}
        for name, cin, cout, size, k, groups in [self.pose_block, *self.embs_blocks, *self.face_blocks, self.joint_block, *self.up_blocks]:
            p[f"{name}.conv_resize.weight"] = folded_weight(sd, f"{name}.conv_resize", (cout, cin // groups, 1, 1))
            p[f"{name}.conv_resize.bias"] = checked(sd, f"{name}.conv_resize.bias", (cout,))
            p[f"{name}.conv1.weight"] = folded_weight(sd, f"{name}.conv1", (cin, cin // groups, k, k))
            p[f"{name}.conv1.bias"] = checked(sd, f"{name}.conv1.bias", (cin, size, size))
            p[f"{name}.conv2.weight"] = folded_weight(sd, f"{name}.conv2", (cout, cin // groups, k, k))
            p[f"{name}.conv2.bias"] = checked(sd, f"{name}.conv2.bias", (cout, size, size))
        for name, n_in, n_out in (("embs_fc.0", self.n_embs, 4 * 4 * 128), ("face_embs_fc.0", self.n_face_embs, 4 * 4 * 32)):
            p[f"{name}.weight"] = folded_weight(sd, name, (n_out, n_in))
            p[f"{name}.bias"] = checked(sd, f"{name}.bias", (n_out,))
        for name in ("verts_conv", "tex_conv"):
            p[f"{name}.weight"] = folded_weight(sd, name, (3, C[-1], 3, 3))
            p[f"{name}.bias"] = checked(sd, f"{name}.bias", (3, self.uv_size, self.uv_size))
        self.params = p

        def mask(key, shape):
            a = as_numpy(asset(assets, key, ASSET_KEYS))
            if tuple(a.shape) != shape:
                raise ValueError(f"assets `{key}` has shape {list(a.shape)}; the configuration expects {list(shape)}")
            return a.astype(np.float64)

        pose_m, head_m = mask("pose_cond_mask", (self.n_pose_dims, S, S)), mask("head_cond_mask", (S, S))
        face_m, body_m = mask("face_cond_mask", (S, S)), mask("body_cond_mask", (S, S))
        # the reference's buffers: pose_cond_mask * (1 - head_cond_mask) truncated to int32; the two float masks; and the
        # non_head_mask forward derives from them
        self.pose_cond_mask = np.ascontiguousarray((pose_m * (1 - head_m[None])).astype(np.int32), np.float32)
        self.face_cond_mask = np.ascontiguousarray(face_m, np.float32)
        self.body_cond_mask = np.ascontiguousarray(body_m, np.float32)
        self.non_head_mask = np.clip(self.body_cond_mask * (np.float32(1.0) - self.face_cond_mask), 0.0, 1.0).astype(np.float32)
        self.seam_sampler = SeamSampler(asset(assets, "seam_data_1024", ASSET_KEYS))
        if (self.seam_sampler.H, self.seam_sampler.W) != (self.uv_size, self.uv_size):
            raise ValueError(f"assets `seam_data_1024` is for {self.seam_sampler.H} x {self.seam_sampler.W} maps; uv_size={self.uv_size}")
        self._dev = {}
        return self

    def _tables(self, device):
        fresh = str(device) not in self._dev
        t = super()._tables(device)
        if fresh:
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device)
            t.update(pose_cond_mask=up(self.pose_cond_mask), non_head_mask=up(self.non_head_mask),
                     face_quadrant=up(self.face_cond_mask[32:, :32]), non_head_quadrant=up(self.non_head_mask[32:, :32]))
            for name in ("embs_fc.0", "face_embs_fc.0"):                      # a linear layer is a 1 x 1 convolution of a 1 x 1 plane
                t[f"{name}.weight"] = t[f"{name}.weight"][:, :, None, None]
        return t

    def activation_bytes_per_frame(self) -> int:
        """An upper bound of the bytes one frame's forward allocates (every intermediate counted as if none were freed)."""
        E, C, S = self.n_embs_enc_channels, self.n_channels, 64
        n = self.n_pose_dims * S * S * 2 + self.n_pose_enc_channels * S * S                      # tiled pose, conv1, pose_conv
        for _, cin, cout, size, _, _ in [*self.embs_blocks, *self.face_blocks, self.joint_block, *self.up_blocks]:
            n += (cin + cout) * size * size
        n += (E + self.n_pose_enc_channels + E) * S * S + 2 * C[0] * S * S                       # merge, two concatenations
        n += (2 * 2 * C[-1] + 6) * self.uv_size ** 2 + 3 * self.surface.V                        # two resamples, the two heads, from_uv
        return 4 * n

    def _block(self, t, x, spec, mask=None):
        """ConvBlock / UpConvBlockDeep in two launches: lrelu(conv1(up(x)) + b1), then lrelu(conv2(.) + b2) + conv_resize(up(x))."""
        name, _, _, size, _, groups = spec
        h = conv2d_ub(x, t[f"{name}.conv1.weight"], t[f"{name}.conv1.bias"], groups=groups, size=(size, size), slope=LRELU_SLOPE)
        return conv2d_ub(h, t[f"{name}.conv2.weight"], t[f"{name}.conv2.bias"], groups=groups, slope=LRELU_SLOPE, skip_src=x,
                         skip_weight=t[f"{name}.conv_resize.weight"], skip_bias=t[f"{name}.conv_resize.bias"], mask=mask)

    def _fc(self, t, x, name, channels):
        """LinearWN + LeakyReLU through the layer kernel (bit-identical for any number of frames), reshaped to [N, channels, 4, 4]."""
        y = conv2d_ub(x[:, :, None, None], t[f"{name}.weight"], t[f"{name}.bias"], slope=LRELU_SLOPE)
        return y.reshape(x.shape[0], channels, 4, 4)

    def forward(self, motion, embs, face_embs, embs_conv=None) -> dict:
        """ConvDecoder.forward: motion [N, 6 + n_pose_dims], embs [N, n_embs], face_embs [N, n_face_embs]; embs_conv [N,
        n_embs_enc_channels, 64, 64] skips the embedding branch (it is not modified).  Returns geom_delta_rec [N, V, 3],
        geom_uv_delta_rec and tex_mean_rec [N, 3, uv_size, uv_size], embs_conv (merged with the face features) and pose_conv."""
        P, E = self.n_pose_dims, self.n_embs_enc_channels
        motion = gpu_f32(motion, "motion", f"[N, {6 + P}]", lambda s: len(s) == 2 and s[1] == 6 + P)
        N, dev = motion.shape[0], motion.device
        embs = gpu_f32(embs, "embs", f"[{N}, {self.n_embs}]", lambda s: s == (N, self.n_embs))
        face_embs = gpu_f32(face_embs, "face_embs", f"[{N}, {self.n_face_embs}]", lambda s: s == (N, self.n_face_embs))
        if embs_conv is not None:
            embs_conv = gpu_f32(embs_conv, "embs_conv", f"[{N}, {E}, 64, 64]", lambda s: s == (N, E, 64, 64))
        for name, x in (("embs", embs), ("face_embs", face_embs), ("embs_conv", embs_conv)):
            if x is not None and x.device != dev:
                raise A2PError(f"{name} is on {x.device}, motion on {dev}")
        t = self._tables(dev)
        with _lib.on_device_of(motion):
            pose_masked = motion[:, 6:, None, None] * t["pose_cond_mask"]                        # tile2d(pose) * pose_cond_mask
            pose_conv = self._block(t, pose_masked, self.pose_block, mask=t["non_head_mask"])
            if embs_conv is None:
                embs_conv = self._fc(t, embs.contiguous(), "embs_fc.0", 128)
                for spec in self.embs_blocks:
                    embs_conv = self._block(t, embs_conv, spec)
            face_conv = self._fc(t, face_embs.contiguous(), "face_embs_fc.0", 32)
            for spec in self.face_blocks:
                face_conv = self._block(t, face_conv, spec)
            merged = embs_conv.clone()
            merged[:, :, 32:, :32] = face_conv * t["face_quadrant"] + embs_conv[:, :, 32:, :32] * t["non_head_quadrant"]
            joint = self._block(t, torch.cat([pose_conv, merged], dim=1), self.joint_block)
            x = torch.cat([joint, joint], dim=1)
            for spec in self.up_blocks:
                x = self._block(t, x, spec)
            x = self.seam_sampler.impaint(x)
            x = self.seam_sampler.resample(self.seam_sampler.resample(x))
            C = self.n_channels[-1]
            verts_uv = conv2d_ub(x[:, :C], t["verts_conv.weight"], t["verts_conv.bias"])
            tex_mean = conv2d_ub(x[:, C:], t["tex_conv.weight"], t["tex_conv.bias"])
            verts = self.surface.from_uv(verts_uv)
        return {"geom_delta_rec": verts, "geom_uv_delta_rec": verts_uv, "tex_mean_rec": tex_mean, "embs_conv": merged,
                "pose_conv": pose_conv}

    __call__ = forward


# ------------------------------------------------------------------------------------------------ convenience
def decode_motion(decoder: BodyDecoder, skeleton, poses, embs, face_embs, max_bytes: int = 1 << 30) -> dict:
    """{"vertices": [B, T, V, 3], "tex_mean": [B, T, 3, H, H], "geom_delta": [B, T, V, 3]} (float32 tensors on the GPU) of
    un-normalised body motion in the layouts skinning.pose_motion takes ([B, T, P], [B, P, 1, T] or [N, P] with P = 6 +
    n_pose_dims; flat frames give [N, ...] outputs) and the embeddings embs [.., n_embs], face_embs [.., n_face_embs] with the
    same leading axes.  The decoder runs in chunks of frames whose activations (BodyDecoder.activation_bytes_per_frame) stay
    under max_bytes, at least one frame; its geom_delta_rec goes to skeleton.pose_vertices as verts_unposed.  A frame's result
    does not depend on the chunking.  The outputs themselves take N (6 V + 3 H H) 4 bytes."""
    avatar.check_pose_width(skeleton, decoder)
    if skeleton.V != decoder.surface.V:
        raise A2PError(f"the skeleton skins V={skeleton.V} vertices; the decoder's surface has V={decoder.surface.V}")
    frames, lead = avatar.clip_frames("decode_motion", poses, skeleton.P_pos)
    N, dev = frames.shape[0], frames.device
    embs = avatar.per_frame(embs, "embs", lead, (decoder.n_embs,), dev)
    face_embs = avatar.per_frame(face_embs, "face_embs", lead, (decoder.n_face_embs,), dev)
    H, V = decoder.uv_size, skeleton.V
    out = {"vertices": torch.empty(N, V, 3, dtype=torch.float32, device=dev),
           "tex_mean": torch.empty(N, 3, H, H, dtype=torch.float32, device=dev),
           "geom_delta": torch.empty(N, V, 3, dtype=torch.float32, device=dev)}
    for a, b in avatar.frame_chunks(N, max_bytes, decoder.activation_bytes_per_frame()):
        preds, out["vertices"][a:b] = avatar.decode_and_pose(decoder, skeleton, frames[a:b], embs[a:b], face_embs[a:b])
        out["geom_delta"][a:b] = preds["geom_delta_rec"]
        out["tex_mean"][a:b] = preds["tex_mean_rec"]
    return {"vertices": out["vertices"].reshape(*lead, V, 3), "tex_mean": out["tex_mean"].reshape(*lead, 3, H, H),
            "geom_delta": out["geom_delta"].reshape(*lead, V, 3)}


def parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m audio2photoreal_amd.decoder",
                                 description="Decode body geometry and mean texture for the motions of a results.npy.")
    ap.add_argument("--results", required=True, help="results.npy of sample.generate (key `motions` [B, 104, 1, T], un-normalised)")
    ap.add_argument("--embeddings", required=True, help=".npz with `embs` [B, T, n_embs] and `face_embs` [B, T, n_face_embs]")
    ap.add_argument("--assets", required=True, help="static_assets.pt: topology, the skinning model, the four masks, seam_data_1024")
    ap.add_argument("--checkpoint", required=True, help="the body decoder's state dict (keys under --prefix)")
    ap.add_argument("--out", required=True, help="decoded.npy: a pickled dict of float32 arrays")
    ap.add_argument("--frames", default=None, metavar="A:B", help="frames A..B-1 of the time axis only")
    ap.add_argument("--max-bytes", type=int, default=1 << 30, help="activation budget of one decoder chunk")
    avatar.add_network_arguments(ap, decoder_only=True)
    return ap


def main(argv=None) -> int:
    args = parser().parse_args(argv)
    motions, embs, face_embs = avatar.load_motion_clip(args.results, args.embeddings, args.frames)
    avatar.require_gpu("the decoder runs")
    person = avatar.load_avatar(args.assets, args.checkpoint, args)
    out = decode_motion(person.decoder, person.skeleton, motions, embs, face_embs, max_bytes=args.max_bytes)
    np.save(args.out, {k: v.cpu().numpy() for k, v in out.items()})
    print(f"{args.out}: " + ", ".join(f"{k} {list(v.shape)}" for k, v in out.items()))
    return 0


if __name__ == "__main__":
    sys.exit(main())
