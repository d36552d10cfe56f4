"""From face codes and body poses to the renderer's embeddings on the MI355X: the reference's FaceDecoderFrontal (visualize/
ca_body/nn/face.py), FaceEncoder and Encoder (models/mesh_vae_drivable.py), the ConvDownBlock of nn/blocks.py they are made of,
la.LinearWN for all frames of a chunk, and AutoEncoder.encode's loop around them, as HIP launches (csrc/kernels_encode.h).

`linear` is one la.LinearWN (a2p_linear_f32: every weight is read once per 64 frames; the sum over the inputs is cut into slices
of 256 terms from the layer's shape alone, so a frame's bits do not depend on the chunk it is computed in).  `conv2d_down3_ub` is
the second launch of a ConvDownBlock, `conv_down_block` the block (the first launch is decoder.conv2d_ub); `face_tex_cond` is
FaceEncoder's texture conditioning in one launch.  `FaceDecoder`, `FaceEncoder` and `BodyEncoder` are built once from the
reference's state dict; `encode_motion` runs them over a clip.  Everything takes float32 tensors that live on the GPU and runs
on the caller's current stream; there is no CPU path.

Differences from the reference, on purpose:
  * the weight normalisation w = v g / ||v|| is folded once at construction, in float64, and rounded to float32 once;
  * FaceDecoder's view branch does not depend on the frame: it is computed once per device, with the same kernel;
  * FaceEncoder.forward takes face_tex_raw and the decoder's bias: face_tex = 255 (raw + bias + 0.5) is formed per tap inside the
    conditioning launch and written to memory only when FaceDecoder.forward is asked for it (return_tex=True);
  * BodySkeleton.unpose_vertices inverts the blended matrix in closed form (adjugate over determinant, fp32) where the reference
    calls Tensor.inverse() on the 4 x 4 matrix (an LU);
  * encode_motion(body_embs="rest") encodes a zero displacement once and broadcasts it; in the reference's render loop the
    displacement unpose(pose(template)) - template is rounding noise.  Not the default."""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _lib, avatar
from ._lib import A2PError
from .avatar import HostNet, as_numpy, asset, checked, f32, gpu_f32, operand, resize_axis_half64, source
from .decoder import LRELU_SLOPE, conv2d_ub
from .texture import conv_transpose2d_ub, folded_weight64, folded_weight_transposed, resize_bilinear

LOGVAR_SCALE = 0.1


# ------------------------------------------------------------------------------------------------ host preparation
def linear_slices(n_in: int) -> int:
    """The number of partial sums a2p_linear_f32 cuts a row of n_in terms into: a function of n_in alone."""
    return (int(n_in) + _lib.LINEAR_KSLICE - 1) // _lib.LINEAR_KSLICE


def _resize_axis_corners64(n_in: int, n_out: int):
    src = np.arange(n_out, dtype=np.float64) * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    i0 = np.minimum(src.astype(np.int64), n_in - 1)
    return i0, np.minimum(i0 + 1, n_in - 1), src - i0


def resize_mask64(mask, size: int, align_corners: bool) -> np.ndarray:
    """float64 [size, size]: F.interpolate(mask[None, None], (size, size), mode="bilinear", align_corners=...) restated."""
    m = as_numpy(mask).astype(np.float64)
    if m.ndim != 2 or min(m.shape) < 1:
        raise ValueError(f"a mask must be [H, W] (got {list(m.shape)})")
    axis = _resize_axis_corners64 if align_corners else resize_axis_half64
    (y0, y1, ly), (x0, x1, lx) = axis(m.shape[0], int(size)), axis(m.shape[1], int(size))
    top = (1 - lx) * m[y0][:, x0] + lx * m[y0][:, x1]
    bot = (1 - lx) * m[y1][:, x0] + lx * m[y1][:, x1]
    return (1 - ly)[:, None] * top + ly[:, None] * bot


def _linear_params(sd, name: str, n_out: int, n_in: int, p: dict):
    p[f"{name}.weight"] = f32(folded_weight64(sd, name, (n_out, n_in)))
    p[f"{name}.bias"] = checked(sd, f"{name}.bias", (n_out,))


def _first_dim(sd, key: str, ndim: int, axis: int = 0) -> int:
    """Size of `axis` of the weight of layer `key` (fused `weight` or `weight_v`), whichever the state dict holds."""
    for suffix in ("weight", "weight_v"):
        if f"{key}.{suffix}" in sd:
            shape = tuple(sd[f"{key}.{suffix}"].shape)
            if len(shape) != ndim:
                raise ValueError(f"`{key}.{suffix}` has shape {list(shape)}; expected {ndim} dimensions")
            return int(shape[axis])
    raise ValueError(f"the state dict has neither `{key}.weight` nor `{key}.weight_v`")


def _down_ladder(sd, names, size: int, c_in: int, p: dict):
    """Folds the ConvDownBlocks `names` (in forward order, the first at input `size` with c_in channels) into p; returns
    [(name, C_in, C_out, input size)] and the final (channels, size)."""
    specs = []
    for name in names:
        if size < 2 or size % 2:
            raise ValueError(f"`{name}` would halve a {size} x {size} map: the ladder is too deep for the input size")
        c_out = _first_dim(sd, f"{name}.conv2", 4)
        p[f"{name}.conv_resize.weight"] = f32(folded_weight64(sd, f"{name}.conv_resize", (c_out, c_in, 1, 1))).reshape(c_out, c_in)
        p[f"{name}.conv_resize.bias"] = checked(sd, f"{name}.conv_resize.bias", (c_out,))
        p[f"{name}.conv1.weight"] = f32(folded_weight64(sd, f"{name}.conv1", (c_in, c_in, 3, 3)))
        p[f"{name}.conv1.bias"] = checked(sd, f"{name}.conv1.bias", (c_in, size, size))
        p[f"{name}.conv2.weight"] = f32(folded_weight64(sd, f"{name}.conv2", (c_out, c_in, 3, 3)))
        p[f"{name}.conv2.bias"] = checked(sd, f"{name}.conv2.bias", (c_out, size // 2, size // 2))
        specs.append((name, c_in, c_out, size))
        c_in, size = c_out, size // 2
    return specs, c_in, size


def _numbered(sd, stem: str, probe: str = "", step: int = 1):
    """[stem.0, stem.step, ...]: the consecutive numbered children of `stem` whose layer `probe` (the child itself when empty)
    has a weight in the state dict, fused or as weight_v."""
    names, i = [], 0
    while True:
        layer = f"{stem}.{i}.{probe}" if probe else f"{stem}.{i}"
        if f"{layer}.weight" not in sd and f"{layer}.weight_v" not in sd:
            return names
        names.append(f"{stem}.{i}")
        i += step


# ------------------------------------------------------------------------------------------------ the launches
def linear(x, weight, bias=None, *, slope=None, out=None):
    """One launch pair of a2p_linear_f32: act(x weight^T + bias).  x [N, I] float32 on the GPU whose rows are dense (a column
    window of a wider matrix is passed as it is); weight [O, I], already folded; bias [O] or None; slope None = no activation.
    out: an [N, O] float32 tensor with dense rows to write into (a column window of a wider matrix: the concatenations of the
    networks are written in place), default a new tensor.  Returns out."""
    x = gpu_f32(x, "x", "[N, I] with I >= 1", lambda s: len(s) == 2 and s[1] >= 1)
    N, I = x.shape
    dev = x.device
    if x.stride(1) != 1 or (N > 1 and x.stride(0) < I):
        x = x.contiguous()
    weight = operand(weight, "weight", f"[O, {I}]", lambda s: len(s) == 2 and s[0] >= 1 and s[1] == I, dev)
    O = weight.shape[0]
    if bias is not None:
        bias = operand(bias, "bias", f"[{O}]", lambda s: s == (O,), dev)
    if out is None:
        out = torch.empty(N, O, dtype=torch.float32, device=dev)
    else:
        out = gpu_f32(out, "out", f"[{N}, {O}]", lambda s: s == (N, O))
        if out.device != dev or out.stride(1) != 1 or (N > 1 and out.stride(0) < O):
            raise A2PError(f"out must be on {dev} with dense rows (got {out.device}, strides {list(out.stride())})")
    if N == 0:
        return out
    S = linear_slices(I)
    scratch = torch.empty(S * N * O, dtype=torch.float32, device=dev) if S > 1 else None
    with _lib.on_device_of(x):
        _lib.check(_lib.load().a2p_linear_f32(_lib.ptr(x), x.stride(0) if N > 1 else I, _lib.ptr(weight), _lib.ptr(bias), N, I, O,
                                              int(slope is not None), float(slope or 0.0), _lib.ptr(out), out.stride(0) if N > 1 else O,
                                              _lib.ptr(scratch), 0 if scratch is None else scratch.numel(), _lib.current_stream(dev)),
                   "a2p_linear_f32")
    return out


def conv2d_down3_ub(h, x, w2, b2, wr, br=None, *, slope: float = LRELU_SLOPE):
    """One launch of a2p_conv2d_down3_ub: lrelu(conv2(h) + b2, slope) + conv_resize(x), the second half of a ConvDownBlock.  h and
    x [N, C_in, Hs, Ws] (channel windows of contiguous tensors are passed as they are); w2 [C_out, C_in, 3, 3] (stride 2, padding
    1), b2 [C_out, H, W] untied, wr [C_out, C_in] (or [.., 1, 1]; stride 2), br [C_out] or None.  Returns [N, C_out, H, W] with H =
    (Hs - 1) // 2 + 1, W = (Ws - 1) // 2 + 1."""
    h, hs = source(h, "h")
    N, C_in, Hs, Ws = h.shape
    dev = h.device
    x, xs = source(x, "x")
    if tuple(x.shape) != tuple(h.shape) or x.device != dev:
        raise A2PError(f"x is {list(x.shape)} on {x.device}; h is {list(h.shape)} on {dev}: they must agree")
    H, W = (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1
    w2 = operand(w2, "w2", f"[C_out, {C_in}, 3, 3]", lambda s: len(s) == 4 and s[0] >= 1 and s[1:] == (C_in, 3, 3), dev)
    C_out = w2.shape[0]
    b2 = operand(b2, "b2", f"[{C_out}, {H}, {W}]", lambda s: s == (C_out, H, W), dev)
    wr = operand(wr, "wr", f"[{C_out}, {C_in}] or [{C_out}, {C_in}, 1, 1]", lambda s: s in ((C_out, C_in), (C_out, C_in, 1, 1)), dev)
    if br is not None:
        br = operand(br, "br", f"[{C_out}]", lambda s: s == (C_out,), dev)
    out = torch.empty(N, C_out, H, W, dtype=torch.float32, device=dev)
    d = _lib.A2PDown3Desc()
    d.h, d.x, d.w2, d.b2, d.wr, d.br, d.out = hs, xs, _lib.ptr(w2), _lib.ptr(b2), _lib.ptr(wr), _lib.ptr(br), _lib.ptr(out)
    d.N, d.C_out, d.slope = N, C_out, float(slope)
    if N == 0:
        return out
    with _lib.on_device_of(h):
        _lib.check(_lib.load().a2p_conv2d_down3_ub(ctypes.byref(d), _lib.current_stream(dev)), "a2p_conv2d_down3_ub")
    return out


def conv_down_block(x, t, name: str):
    """ConvDownBlock `name` in two launches: h = lrelu(conv1(x) + b1), then lrelu(conv2(h) + b2) + conv_resize(x).  t maps
    `name.conv1.weight`, ... to device tensors."""
    h = conv2d_ub(x, t[f"{name}.conv1.weight"], t[f"{name}.conv1.bias"], slope=LRELU_SLOPE)
    return conv2d_down3_ub(h, x, t[f"{name}.conv2.weight"], t[f"{name}.conv2.bias"], t[f"{name}.conv_resize.weight"],
                           t[f"{name}.conv_resize.bias"], slope=LRELU_SLOPE)


def face_tex_cond(raw, bias, mask):
    """One launch of a2p_face_tex_cond: (resize(255 (raw + bias + 0.5)) / 255 - 0.5) * mask with F.interpolate's bilinear rule
    (align_corners=False) at the mask's size.  raw [N, C, Hs, Ws]; bias [C, Hs, Ws]; mask [H, W].  Returns [N, C, H, W]."""
    raw = gpu_f32(raw, "raw", "[N, C, Hs, Ws]", lambda s: len(s) == 4 and min(s[1:]) >= 1).contiguous()
    N, C, Hs, Ws = raw.shape
    dev = raw.device
    bias = operand(bias, "bias", f"[{C}, {Hs}, {Ws}]", lambda s: s == (C, Hs, Ws), dev)
    mask = operand(mask, "mask", "[H, W]", lambda s: len(s) == 2 and min(s) >= 1, dev)
    H, W = mask.shape
    out = torch.empty(N, C, H, W, dtype=torch.float32, device=dev)
    if N == 0:
        return out
    with _lib.on_device_of(raw):
        _lib.check(_lib.load().a2p_face_tex_cond(_lib.ptr(raw), _lib.ptr(bias), _lib.ptr(mask), N, C, Hs, Ws, H, W, _lib.ptr(out),
                                                 _lib.current_stream(dev)), "a2p_face_tex_cond")
    return out


# ------------------------------------------------------------------------------------------------ the networks
class FaceDecoder(HostNet):
    """FaceDecoderFrontal of nn/face.py: face codes [N, n_latent] to face_geom [N, V_f, 3] and the raw face texture."""

    @classmethod
    def from_state_dict(cls, state_dict, assets, prefix: str = "decoder_face.") -> "FaceDecoder":
        """state_dict: encmod.0, geommod.0, viewmod.0, texmod2.0, texmod.0 / 2 / 4 / ... and bias under `prefix` (a fused
        `weight` is accepted in place of a `_g` / `_v` pair); assets: face_frontal_view [3].  The depth and sizes of the texture
        ladder are read from the state dict (the reference's: eight layers, 4 x 4 to 1024 x 1024)."""
        self = object.__new__(cls)
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        p = {}
        self.n_hidden = _first_dim(sd, "encmod.0", 2)
        self.n_latent = _first_dim(sd, "encmod.0", 2, 1)
        n_vert_out = _first_dim(sd, "geommod.0", 2)
        if n_vert_out % 3:
            raise ValueError(f"`geommod.0` has {n_vert_out} outputs; three per vertex are expected")
        self.V = n_vert_out // 3
        self.n_view = _first_dim(sd, "viewmod.0", 2)
        view = as_numpy(asset(assets, "face_frontal_view")).astype(np.float32).reshape(-1)
        _linear_params(sd, "encmod.0", self.n_hidden, self.n_latent, p)
        _linear_params(sd, "geommod.0", n_vert_out, self.n_hidden, p)
        _linear_params(sd, "viewmod.0", self.n_view, view.size, p)
        layers = _numbered(sd, "texmod", step=2)
        if not layers:
            raise ValueError("the state dict has no `texmod.0.weight` / `texmod.0.weight_v`")
        c = _first_dim(sd, layers[0], 4)
        n_tex2 = _first_dim(sd, "texmod2.0", 2)
        s = int(round(np.sqrt(n_tex2 / c)))
        if s < 1 or c * s * s != n_tex2:
            raise ValueError(f"`texmod2.0` has {n_tex2} outputs; {c} channels of a square map are expected")
        _linear_params(sd, "texmod2.0", n_tex2, self.n_hidden + self.n_view, p)
        self.c0, self.s0, self.layers = c, s, []
        for name in layers:
            c_out = _first_dim(sd, name, 4, 1)
            p[f"{name}.weight"] = folded_weight_transposed(sd, name, (c, c_out, 4, 4))
            p[f"{name}.bias"] = checked(sd, f"{name}.bias", (c_out, 2 * s, 2 * s))
            self.layers.append((name, c, c_out, s))
            c, s = c_out, 2 * s
        if s > _lib.CONV_MAX_SIZE:
            raise ValueError(f"the texture ladder ends at {s} x {s}; a side is at most {_lib.CONV_MAX_SIZE}")
        self.tex_channels, self.tex_size = c, s
        p["bias"] = checked(sd, "bias", (c, s, s))
        p["frontal_view"] = view.reshape(1, -1)
        self.params, self._dev = p, {}
        return self

    def _tables(self, device):
        fresh = str(device) not in self._dev
        t = super()._tables(device)
        if fresh:
            with torch.cuda.device(device):
                t["viewout"] = linear(t["frontal_view"], t["viewmod.0.weight"], t["viewmod.0.bias"], slope=LRELU_SLOPE)
        return t

    def bias(self, device):
        """The texture bias [C, S, S] on `device`: what FaceEncoder.forward adds to face_tex_raw."""
        return self._tables(device)["bias"]

    def activation_floats_per_frame(self) -> int:
        n = 2 * self.n_hidden + self.n_view + 3 * self.V + self.c0 * self.s0 ** 2
        n += sum(c_out * 4 * s * s for _, _, c_out, s in self.layers)
        return n + self.tex_channels * self.tex_size ** 2                      # face_tex on request

    def forward(self, face_codes, return_tex: bool = False) -> dict:
        """face_codes [N, n_latent] -> {"face_geom": [N, V_f, 3], "face_tex_raw": [N, C, S, S]} and, with return_tex, "face_tex" =
        255 (face_tex_raw + bias + 0.5) (torch arithmetic, in the reference's order)."""
        x = gpu_f32(face_codes, "face_codes", f"[N, {self.n_latent}]", lambda s: len(s) == 2 and s[1] == self.n_latent)
        N, dev = x.shape[0], x.device
        t = self._tables(dev)
        with _lib.on_device_of(x):
            encview = torch.empty(N, self.n_hidden + self.n_view, dtype=torch.float32, device=dev)
            encout = linear(x, t["encmod.0.weight"], t["encmod.0.bias"], slope=LRELU_SLOPE, out=encview[:, :self.n_hidden])
            encview[:, self.n_hidden:] = t["viewout"]
            geom = linear(encout, t["geommod.0.weight"], t["geommod.0.bias"])
            y = linear(encview, t["texmod2.0.weight"], t["texmod2.0.bias"], slope=LRELU_SLOPE).reshape(N, self.c0, self.s0, self.s0)
            for i, (name, _, _, _) in enumerate(self.layers):
                y = conv_transpose2d_ub(y, t[f"{name}.weight"], t[f"{name}.bias"], slope=LRELU_SLOPE if i + 1 < len(self.layers) else None)
            out = {"face_geom": geom.reshape(N, self.V, 3), "face_tex_raw": y}
            if return_tex:
                out["face_tex"] = 255 * ((y + t["bias"][None]) + 0.5)
        return out

    __call__ = forward


class FaceEncoder(HostNet):
    """FaceEncoder of mesh_vae_drivable.py in eval mode: face geometry and texture to the face embedding in body space."""

    @classmethod
    def from_state_dict(cls, state_dict, assets, prefix: str = "encoder_face.", uv_size: int = 512, tex_channels: int = 3,
                        logvar_scale: float = LOGVAR_SCALE) -> "FaceEncoder":
        """state_dict: conv_blocks.0.., geommod.0, jointmod.0, mu, logvar under `prefix`; assets: mugsy_face_mask [H, W, >= 1], whose
        channel 0 is resized to uv_size with align_corners=True here, in float64.  The depth of the ladder is read from the state
        dict (the reference's: seven blocks, 512 x 512 to 4 x 4)."""
        self = object.__new__(cls)
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        if not 2 <= int(uv_size) <= _lib.CONV_MAX_SIZE:
            raise ValueError(f"uv_size={uv_size} is outside [2, {_lib.CONV_MAX_SIZE}]")
        self.uv_size, self.tex_channels, self.logvar_scale = int(uv_size), int(tex_channels), float(logvar_scale)
        p = {}
        blocks = _numbered(sd, "conv_blocks", "conv2")
        if not blocks:
            raise ValueError("the state dict has no `conv_blocks.0.conv2.weight` / `.weight_v`")
        self.blocks, c, s = _down_ladder(sd, blocks, self.uv_size, self.tex_channels, p)
        self.n_tex_enc = c * s * s
        self.n_geom_enc = _first_dim(sd, "geommod.0", 2)
        self.n_vert_in = _first_dim(sd, "geommod.0", 2, 1)
        self.n_joint = _first_dim(sd, "jointmod.0", 2)
        self.n_embs = _first_dim(sd, "mu", 2)
        _linear_params(sd, "geommod.0", self.n_geom_enc, self.n_vert_in, p)
        _linear_params(sd, "jointmod.0", self.n_joint, self.n_tex_enc + self.n_geom_enc, p)
        _linear_params(sd, "mu", self.n_embs, self.n_joint, p)
        _linear_params(sd, "logvar", self.n_embs, self.n_joint, p)
        mask = as_numpy(asset(assets, "mugsy_face_mask"))
        if mask.ndim != 3 or min(mask.shape) < 1:
            raise ValueError(f"assets `mugsy_face_mask` must be [H, W, C] (got {list(mask.shape)})")
        p["tex_cond_mask"] = f32(resize_mask64(mask[..., 0], self.uv_size, True))
        self.params, self._dev = p, {}
        return self

    def activation_floats_per_frame(self) -> int:
        n = self.tex_channels * self.uv_size ** 2 + self.n_tex_enc + self.n_geom_enc + self.n_joint + 2 * self.n_embs
        n += sum((c_in + c_out // 4) * s * s for _, c_in, c_out, s in self.blocks)
        return n + 2 * linear_slices(self.n_vert_in) * self.n_geom_enc

    def forward(self, face_geom, face_tex_raw, bias) -> dict:
        """face_geom [N, V_f, 3] (or [N, 3 V_f]), face_tex_raw [N, C, S, S] and the decoder's bias [C, S, S] -> {"face_embs",
        "face_embs_mu", "face_embs_logvar"} [N, n_embs] (face_embs is a copy of mu: eval mode) and "face_tex_cond"."""
        g = gpu_f32(face_geom, "face_geom", f"[N, {self.n_vert_in // 3}, 3] or [N, {self.n_vert_in}]",
                     lambda s: len(s) in (2, 3) and int(np.prod(s[1:])) == self.n_vert_in)
        N, dev = g.shape[0], g.device
        C = self.tex_channels
        raw = gpu_f32(face_tex_raw, "face_tex_raw", f"[{N}, {C}, S, S]", lambda s: len(s) == 4 and s[:2] == (N, C))
        if raw.device != dev:
            raise A2PError(f"face_tex_raw is on {raw.device}, face_geom on {dev}")
        t = self._tables(dev)
        with _lib.on_device_of(g):
            tex_cond = face_tex_cond(raw, bias, t["tex_cond_mask"])
            x = tex_cond
            for name, _, _, _ in self.blocks:
                x = conv_down_block(x, t, name)
            joint_in = torch.empty(N, self.n_tex_enc + self.n_geom_enc, dtype=torch.float32, device=dev)
            joint_in[:, :self.n_tex_enc] = x.reshape(N, self.n_tex_enc)
            linear(g.reshape(N, self.n_vert_in), t["geommod.0.weight"], t["geommod.0.bias"], slope=LRELU_SLOPE,
                   out=joint_in[:, self.n_tex_enc:])
            j = linear(joint_in, t["jointmod.0.weight"], t["jointmod.0.bias"], slope=LRELU_SLOPE)
            mu = linear(j, t["mu.weight"], t["mu.bias"])
            logvar = self.logvar_scale * linear(j, t["logvar.weight"], t["logvar.bias"])
        return {"face_embs": mu.clone(), "face_embs_mu": mu, "face_embs_logvar": logvar, "face_tex_cond": tex_cond}

    __call__ = forward


class BodyEncoder(HostNet):
    """Encoder of mesh_vae_drivable.py in eval mode: the unposed vertex displacement to the body embedding."""

    @classmethod
    def from_state_dict(cls, state_dict, assets, surface, prefix: str = "encoder.", uv_size: int = 512,
                        logvar_scale: float = LOGVAR_SCALE) -> "BodyEncoder":
        """state_dict: verts_conv, joint_conv_blocks.0.., mu, logvar under `prefix`; assets: face_mask [H, W], from which mask =
        F.interpolate(1 - face_mask, uv_size, "bilinear") != 0 is computed here in float64; surface: the surface.BodySurface whose
        to_uv maps vertices to UV space."""
        self = object.__new__(cls)
        sd = {k[len(prefix):]: v for k, v in state_dict.items() if k.startswith(prefix)}
        if not 2 <= int(uv_size) <= _lib.CONV_MAX_SIZE:
            raise ValueError(f"uv_size={uv_size} is outside [2, {_lib.CONV_MAX_SIZE}]")
        self.uv_size, self.logvar_scale, self.surface = int(uv_size), float(logvar_scale), surface
        p = {}
        blocks = ["verts_conv"] + _numbered(sd, "joint_conv_blocks", "conv2")
        self.blocks, c, s = _down_ladder(sd, blocks, self.uv_size, 3, p)
        self.n_flat = c * s * s
        self.n_embs = _first_dim(sd, "mu", 2)
        _linear_params(sd, "mu", self.n_embs, self.n_flat, p)
        _linear_params(sd, "logvar", self.n_embs, self.n_flat, p)
        face_mask = as_numpy(asset(assets, "face_mask")).astype(np.float64)
        p["mask"] = f32(resize_mask64(1.0 - face_mask, self.uv_size, False) != 0)
        self.params, self._dev = p, {}
        return self

    def activation_floats_per_frame(self) -> int:
        n = 3 * self.surface.uv_size ** 2 + 2 * 3 * self.uv_size ** 2 + 2 * self.n_embs
        n += sum((c_in + c_out // 4) * s * s for _, c_in, c_out, s in self.blocks)
        return n + 2 * linear_slices(self.n_flat) * self.n_embs

    def forward(self, verts_unposed) -> dict:
        """verts_unposed [N, V, 3] -> {"embs", "embs_mu", "embs_logvar"} [N, n_embs] (embs is a copy of mu: eval mode)."""
        v = gpu_f32(verts_unposed, "verts_unposed", f"[N, {self.surface.V}, 3]", lambda s: len(s) == 3 and s[1:] == (self.surface.V, 3))
        N = v.shape[0]
        t = self._tables(v.device)
        with _lib.on_device_of(v):
            x = resize_bilinear(self.surface.to_uv(v), (self.uv_size, self.uv_size)) * t["mask"]
            for name, _, _, _ in self.blocks:
                x = conv_down_block(x, t, name)
            x = x.reshape(N, self.n_flat)
            mu = linear(x, t["mu.weight"], t["mu.bias"])
            logvar = self.logvar_scale * linear(x, t["logvar.weight"], t["logvar.bias"])
        return {"embs": mu.clone(), "embs_mu": mu, "embs_logvar": logvar}

    __call__ = forward


# ------------------------------------------------------------------------------------------------ convenience
def activation_bytes_per_frame(face_decoder: FaceDecoder, face_encoder: FaceEncoder, body_encoder: BodyEncoder, skeleton) -> int:
    """An upper bound of the bytes one frame of encode_motion allocates (every intermediate counted as if none were freed)."""
    n = face_decoder.activation_floats_per_frame() + face_encoder.activation_floats_per_frame()
    n += body_encoder.activation_floats_per_frame() + skeleton.J * 12 + 3 * 3 * skeleton.V
    return 4 * n


def clip_inputs(name, skeleton, face_decoder, face_encoder, body_encoder, poses, face_codes):
    """(frames [N, P] and codes [N, n_latent] on the GPU, the leading axes) of a clip, after the checks the entry points share."""
    if skeleton.V != body_encoder.surface.V:
        raise A2PError(f"the skeleton skins V={skeleton.V} vertices; the encoder's surface has V={body_encoder.surface.V}")
    if 3 * face_decoder.V != face_encoder.n_vert_in or face_decoder.tex_channels != face_encoder.tex_channels:
        raise A2PError(f"the face decoder gives {face_decoder.V} vertices and {face_decoder.tex_channels} texture channels; the face "
                       f"encoder takes {face_encoder.n_vert_in // 3} and {face_encoder.tex_channels}")
    frames, lead = avatar.clip_frames(name, poses, skeleton.P_pos)
    return frames, avatar.per_frame(face_codes, "face_codes", lead, (face_decoder.n_latent,), frames.device), lead


def encode_chunk(face_decoder, face_encoder, body_encoder, skeleton, frames, codes, geom, rest_embs):
    """(embs, face_embs) of one chunk of frames: AutoEncoder.encode.  rest_embs [1, n_embs] replaces the body branch."""
    face = face_decoder.forward(codes)
    face_embs = face_encoder.forward(face["face_geom"], face["face_tex_raw"], face_decoder.bias(frames.device))["face_embs"]
    if rest_embs is not None:
        return rest_embs.expand(frames.shape[0], -1), face_embs
    g = skeleton.pose_vertices(frames) if geom is None else geom
    return body_encoder.forward(skeleton.unpose_vertices(frames, g))["embs"], face_embs


def rest_embs(body_encoder, skeleton, device):
    return body_encoder.forward(torch.zeros(1, skeleton.V, 3, dtype=torch.float32, device=device))["embs"]


def encode_motion(face_decoder: FaceDecoder, face_encoder: FaceEncoder, body_encoder: BodyEncoder, skeleton, poses, face_codes,
                  geom=None, body_embs: str = "per_frame", max_bytes: int = 1 << 30) -> dict:
    """{"embs": [.., n_embs], "face_embs": [.., n_face_embs]} (float32 tensors on the GPU) on the leading axes of `poses`: what
    AutoEncoder.encode computes for the render loop.  poses: un-normalised body motion in the layouts skinning.pose_motion takes;
    face_codes [.., n_latent] with the same leading axes; geom [.., V, 3]: the posed geometry to encode, default the posed
    template (the reference's render loop).  body_embs="per_frame" unposes and encodes every frame; "rest" encodes a zero
    displacement once and broadcasts it (only with geom=None; see the module docstring).  Runs in chunks of frames whose
    activations (activation_bytes_per_frame) stay under max_bytes, at least one frame; a frame's result does not depend on the
    chunking."""
    avatar.check_body_embs(body_embs)
    if body_embs == "rest" and geom is not None:
        raise A2PError("body_embs='rest' encodes the template: it takes no geom")
    frames, codes, lead = clip_inputs("encode_motion", skeleton, face_decoder, face_encoder, body_encoder, poses, face_codes)
    N, dev, V = frames.shape[0], frames.device, skeleton.V
    if geom is not None:
        geom = avatar.per_frame(geom, "geom", lead, (V, 3), dev)
    out = {"embs": torch.empty(N, body_encoder.n_embs, dtype=torch.float32, device=dev),
           "face_embs": torch.empty(N, face_encoder.n_embs, dtype=torch.float32, device=dev)}
    rest = rest_embs(body_encoder, skeleton, dev) if body_embs == "rest" and N else None
    for a, b in avatar.frame_chunks(N, max_bytes, activation_bytes_per_frame(face_decoder, face_encoder, body_encoder, skeleton)):
        out["embs"][a:b], out["face_embs"][a:b] = encode_chunk(face_decoder, face_encoder, body_encoder, skeleton, frames[a:b], codes[a:b],
                                                                None if geom is None else geom[a:b], rest)
    return {k: v.reshape(*lead, v.shape[1]) for k, v in out.items()}


def render_codes_motion(face_decoder: FaceDecoder, face_encoder: FaceEncoder, body_encoder: BodyEncoder, decoder, texture, skeleton,
                        rasterizer, poses, face_codes, K, Rt, camera_pos=None, body_embs: str = "per_frame", max_bytes: int = 1 << 30,
                        supersample: int = 1, background=None):
    """uint8 frames [B, T, H, C W, 3] (or [N, H, C W, 3] for flat frames) on the GPU of sampler output -- un-normalised body poses
    and face codes on the same leading axes -- seen by C cameras side by side: BodyRenderer._render_loop of visualize/
    render_codes.py, which uses 2.  K [C, 3, 3], Rt [C, 3, 4]; camera_pos [C, 3] defaults to render.camera_centre(Rt).  Per chunk
    of frames the embeddings are encoded (encode_motion with geom=None) and the body decoded and posed once; the texture, the
    rasterisation and texture.linear_to_display run per camera; the images are concatenated along the width, clipped to [0, 255]
    and truncated to uint8.  A chunk's activations stay under max_bytes, at least one frame; a frame's result does not depend on
    the chunking.  supersample and background as in texture.render_rgb_motion: s x s samples per pixel, and one display-space
    colour or [H, W, 3] / [3, H, W] panel in [0, 255] behind the avatar, the same for every camera; a pixel no sample covers holds
    the background's bytes exactly."""
    from .texture import display_background, display_frames
    supersample = rasterizer._supersample(supersample)
    background = display_background(background, rasterizer.height, rasterizer.width)
    avatar.check_body_embs(body_embs)
    avatar.check_pose_width(skeleton, decoder)
    avatar.check_embedding_widths(body_encoder, face_encoder, decoder)
    frames, codes, lead = clip_inputs("render_codes_motion", skeleton, face_decoder, face_encoder, body_encoder, poses, face_codes)
    N, dev = frames.shape[0], frames.device
    K, Rt, camera_pos, C = avatar.cameras(K, Rt, camera_pos, dev)
    per_frame = (activation_bytes_per_frame(face_decoder, face_encoder, body_encoder, skeleton) + decoder.activation_bytes_per_frame()
                 + texture.activation_bytes_per_frame())
    H, W = rasterizer.height, rasterizer.width
    background = tuple(None if x is None else x.to(dev) for x in background)
    out = torch.empty(N, H, C * W, 3, dtype=torch.uint8, device=dev)
    rest = rest_embs(body_encoder, skeleton, dev) if body_embs == "rest" and N else None
    for a, b in avatar.frame_chunks(N, max_bytes, per_frame):
        embs, face_embs = encode_chunk(face_decoder, face_encoder, body_encoder, skeleton, frames[a:b], codes[a:b], None, rest)
        preds, verts = avatar.decode_and_pose(decoder, skeleton, frames[a:b], embs.contiguous(), face_embs)
        for c in range(C):
            tex = texture.forward(verts, preds["tex_mean_rec"], camera_pos[c:c + 1], motion=frames[a:b] if texture.pose_shadow is not None else None)
            image = display_frames(rasterizer, verts, tex["tex_rec"], K[c:c + 1], Rt[c:c + 1], supersample, background)
            out[a:b, :, c * W:(c + 1) * W] = avatar.uint8_panel(image)
    return out.reshape(*lead, H, C * W, 3)


def parser():
    import argparse
    ap = argparse.ArgumentParser(
        prog="python -m audio2photoreal_amd.encoder",
        description="Video frames of sampler output: face codes and body poses to uint8 images, one panel per camera.")
    ap.add_argument("--results", required=True, help="results.npy: a pickled dict with `pose` [R, T, 104] and `face` [R, T, 256], un-normalised "
                    "(what sample.recording.generate_from_recording returns)")
    ap.add_argument("--assets", required=True, help="static_assets.pt: topology, skinning model, masks, tex_mean, seam tables, face_frontal_view, "
                    "mugsy_face_mask, face_mask")
    ap.add_argument("--checkpoint", required=True, help="the body model's state dict (encoder.*, encoder_face.*, decoder_face.*, decoder.*, ...)")
    ap.add_argument("--out", required=True, help="frames.npy: a uint8 array [R, T, H, C W, 3]")
    cam = avatar.add_camera_arguments(ap, per="camera")
    cam.add_argument("--defaults", metavar="FILE", help="render_defaults_*.pth of the reference's demo: a dict whose `K` [C, 3, 3], `Rt` [C, 3, 4] and "
                     "(optional) `campos` [C, 3] are read as the cameras.  The file is not part of the reference's tree: that it holds these keys "
                     "in these shapes is an assumption")
    avatar.add_render_arguments(ap, png="frame")
    avatar.add_video_arguments(ap)
    avatar.add_network_arguments(ap, encoders=True)
    return ap


def main(argv=None) -> int:
    from . import render as R
    from . import video
    args = parser().parse_args(argv)
    if args.defaults is not None and args.target is not None:
        raise A2PError("--target goes with --eye, not with --defaults")
    if args.audio is not None and args.video is None:
        raise A2PError("--audio goes with --video")
    pose, face = avatar.load_codes_clip(args.results)
    if pose.ndim != 3 or face.ndim != 3 or pose.shape[:2] != face.shape[:2]:
        raise A2PError(f"`pose` must be [R, T, P] and `face` [R, T, F] with the same R and T (got {list(pose.shape)} and {list(face.shape)})")
    window = avatar.frame_window(args.frames)
    pose, face = pose[:, window], face[:, window]
    avatar.require_gpu("the frames are rendered")
    person = avatar.load_avatar(args.assets, args.checkpoint, args)
    H, W = args.size
    poses = torch.from_numpy(pose).to("cuda")
    camera_pos = None
    if args.defaults is not None:
        d = torch.load(args.defaults, map_location="cpu", weights_only=False)
        for key in ("K", "Rt"):
            if key not in d:
                raise A2PError(f"{args.defaults} holds no `{key}` (keys: {sorted(d)})")
        K, Rt = torch.as_tensor(d["K"]).float().reshape(-1, 3, 3), torch.as_tensor(d["Rt"]).float()[..., :3, :4].reshape(-1, 3, 4)
        camera_pos = torch.as_tensor(d["campos"]).float().reshape(-1, 3) if "campos" in d else None
    else:
        rest = person.skeleton.pose_vertices(poses.reshape(-1, poses.shape[-1])[:1]).cpu().numpy()  # frames the default camera
        K, Rt = R._camera_from_args(args, rest, H, W)
    on_gpu = render_codes_motion(*person[:6], R.BodyRasterizer(person.surface, H, W), poses, face, K, Rt, camera_pos, body_embs=args.body_embs,
                                 max_bytes=args.max_bytes, supersample=args.supersample, background=args.background)
    frames = on_gpu.cpu().numpy()
    np.save(args.out, frames)
    print(f"{args.out}: frames {list(frames.shape)} uint8")
    if args.video is not None:
        audio, rate = avatar.video_audio(args)
        for r in range(on_gpu.shape[0]):
            path = video.sequence_path(args.video, r, on_gpu.shape[0])
            video.write_video(path, on_gpu[r], fps=args.fps, audio=audio, audio_rate=rate)
            print(f"{path}: {on_gpu.shape[1]} frames at {args.fps:g} fps")
    if args.png_dir is not None:
        print(f"{args.png_dir}: {R.write_pngs({'frame': frames.transpose(0, 1, 4, 2, 3)}, args.png_dir)} png files")
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
