"""TemporalVertexCodec: the reference's residual-VQ tokenizer (model/vqvae.py:467-521) on the sampling path.
`decode(tokens)` turns the guide transformer's tokens into the keyframe poses the body denoiser is conditioned on
(sample/generate.py:51-71).  Built with `with_encoder=True` it also has the encode side: `encode(poses)` (= `predict`) turns known
keyframe poses into the tokens the guide can be forced to (sample/generate.py `_replace_keyframes(known=...)`), and
`encoder(poses)` returns the encoder's latents.  Parameter names are the reference's; EMA buffers and `project_mean_shape` are
accepted by `load_state_dict(strict=False)` semantics of the caller and not needed here.  The arithmetic runs in liba2p_hip.so
(`a2p_vq_decode`: codebook gather + sum, 4 causal dilated Conv1d + LeakyReLU, 1x1 conv; `a2p_vq_encode`: the encoder convs and
the residual nearest-code search; one workgroup per sequence)."""
from __future__ import annotations

import ctypes as C

import torch
import torch.nn as nn

from .. import _lib


class _Codebook(nn.Module):
    def __init__(self, categories: int, dim: int):
        super().__init__()
        self.register_buffer("embed", torch.randn(categories, dim))     # EuclideanCodebook.embed (model/vqvae.py:86-110)


class _VQ(nn.Module):
    def __init__(self, categories: int, dim: int):
        super().__init__()
        self._codebook = _Codebook(categories, dim)


class _RVQ(nn.Module):
    def __init__(self, categories: int, dim: int, depth: int):
        super().__init__()
        self.layers = nn.ModuleList([_VQ(categories, dim) for _ in range(depth)])


class _Decoder(nn.Module):
    def __init__(self, n_vertices: int, latent_dim: int):
        super().__init__()
        lr = lambda: nn.LeakyReLU(0.2)                                   # noqa: E731
        self.dec = nn.Sequential(                                       # model/vqvae.py:440-450
            nn.Conv1d(latent_dim, latent_dim, 2, dilation=1), lr(), nn.Conv1d(latent_dim, latent_dim, 2, dilation=2), lr(),
            nn.Conv1d(latent_dim, latent_dim, 2, dilation=3), lr(), nn.Conv1d(latent_dim, latent_dim, 2, dilation=1), lr(),
            nn.Conv1d(latent_dim, n_vertices, 1))


class _Encoder(nn.Module):
    """TemporalVertexEncoder's parameters (model/vqvae.py:395-415); calling it runs `a2p_vq_encode` for the latents only."""
    def __init__(self, codec: "TemporalVertexCodec", n_vertices: int, latent_dim: int):
        super().__init__()
        # skip_init builds the convs without their random initialisation: constructing a codec leaves torch's global RNG alone
        conv = lambda cin, k, dl: nn.utils.skip_init(nn.Conv1d, cin, latent_dim, k, dilation=dl)       # noqa: E731
        lr = lambda: nn.LeakyReLU(0.2)                                                              # noqa: E731
        self.enc = nn.Sequential(conv(n_vertices, 1, 1), lr(), conv(latent_dim, 2, 1), lr(), conv(latent_dim, 2, 2), lr(),
                                 conv(latent_dim, 2, 3), lr(), conv(latent_dim, 2, 1))
        with torch.no_grad():
            for p in self.enc.parameters():
                p.zero_()
        self._codec = [codec]         # a list: not a sub-module (the codec owns this module)

    def forward(self, poses: torch.Tensor) -> torch.Tensor:
        """poses [B, T, n_vertices] -> the encoder's latents fp32 [B, T, latent_dim] (reference :417-430)."""
        return self._codec[0]._encode(poses, tokens=False)


class TemporalVertexCodec(nn.Module):
    def __init__(self, n_vertices: int = 338, latent_dim: int = 128, categories: int = 128, residual_depth: int = 4,
                 with_encoder: bool = False):
        super().__init__()
        self.latent_dim, self.categories, self.residual_depth = latent_dim, categories, residual_depth
        self.n_clusters, self.n_vertices = categories, n_vertices
        if with_encoder:
            self.encoder = _Encoder(self, n_vertices, latent_dim)
        self.decoder = _Decoder(n_vertices, latent_dim)
        self.quantizer = _RVQ(categories, latent_dim, residual_depth)
        self._staged = None           # (signature, fp32 device copies the kernel reads): kept alive across calls
        self._staged_enc = None       # the same for the encode side, with |embed|^2 per code

    @property
    def has_encoder(self) -> bool:
        return "encoder" in self._modules

    def _stage(self, device):
        """fp32 contiguous device copies of the codebooks / conv weights, rebuilt only when a parameter changes (round 1 re-staged
        and synchronised the stream on every call)."""
        src = [l._codebook.embed for l in self.quantizer.layers] + [t for i in (0, 2, 4, 6, 8)
                                                                     for t in (self.decoder.dec[i].weight, self.decoder.dec[i].bias)]
        sig = (str(device), _lib.content_key(*src))
        if self._staged is None or self._staged[0] != sig:
            f32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()   # noqa: E731
            nb = len(self.quantizer.layers)
            books = [f32(t) for t in src[:nb]]
            ws, bs = [f32(t) for t in src[nb::2]], [f32(t) for t in src[nb + 1::2]]
            self._staged = (sig, books, ws, bs, src)
        return self._staged[1:4]

    def decode(self, q: torch.Tensor) -> torch.Tensor:
        """q int64 [B, T, residual_depth] -> [B, T, n_vertices] (reference :508-521)."""
        _lib.require_gpu_tensor(q, "tokens")
        assert q.dim() == 3 and q.shape[-1] == self.residual_depth
        B, T, _ = q.shape
        q = q.to(torch.int64).contiguous()
        books, ws, bs = self._stage(q.device)
        arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])               # noqa: E731
        out = torch.empty(B, T, self.n_vertices, device=q.device, dtype=torch.float32)
        with _lib.on_device_of(q):
            _lib.check(_lib.load().a2p_vq_decode(_lib.ptr(q), B, T, self.residual_depth, self.categories, self.latent_dim, self.n_vertices,
                                                 arr(books), arr(ws), arr(bs), _lib.ptr(out), _lib.current_stream(q.device)), "a2p_vq_decode")
        return out   # no synchronise: the staged copies live on the module, `q` / `out` are ordered by the stream

    def _stage_encoder(self, device):
        """fp32 device copies of the codebooks and encoder convs plus |embed|^2 per code (summed in float64, rounded once),
        rebuilt only when a parameter changes."""
        src = [l._codebook.embed for l in self.quantizer.layers] + [t for i in (0, 2, 4, 6, 8)
                                                                     for t in (self.encoder.enc[i].weight, self.encoder.enc[i].bias)]
        sig = (str(device), _lib.content_key(*src))
        if self._staged_enc is None or self._staged_enc[0] != sig:
            if not any(bool(t.detach().any()) for t in src[len(self.quantizer.layers):]):
                # with_encoder builds zeros; a checkpoint loaded with strict=False may lack encoder.enc.*, and an all-zero encoder
                # would map every pose to the same tokens
                raise _lib.A2PError("the tokenizer's encoder weights are all zero: load the checkpoint's encoder.enc.* weights")
            f32 = lambda t: t.detach().to(device=device, dtype=torch.float32).contiguous()   # noqa: E731
            nb = len(self.quantizer.layers)
            books = [f32(t) for t in src[:nb]]
            norms = [b.double().pow(2).sum(1).float().contiguous() for b in books]
            ws, bs = [f32(t) for t in src[nb::2]], [f32(t) for t in src[nb + 1::2]]
            self._staged_enc = (sig, books, norms, ws, bs, src)
        return self._staged_enc[1:5]

    def _encode(self, poses: torch.Tensor, tokens: bool) -> torch.Tensor:
        if not self.has_encoder:
            raise _lib.A2PError("this TemporalVertexCodec has no encoder: construct it with with_encoder=True and load the "
                                "checkpoint's encoder.enc.* weights")
        if poses.dim() != 3 or poses.shape[-1] != self.n_vertices:
            raise _lib.A2PError(f"poses must be [B, T, {self.n_vertices}] (got {tuple(poses.shape)})")
        _lib.require_gpu_tensor(poses, "poses")
        books, norms, ws, bs = self._stage_encoder(poses.device)
        B, T, _ = poses.shape
        x = poses.to(torch.float32).contiguous()
        arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])               # noqa: E731
        q = torch.empty(B, T, self.residual_depth, device=x.device, dtype=torch.int64) if tokens else None
        lat = None if tokens else torch.empty(B, T, self.latent_dim, device=x.device, dtype=torch.float32)
        with _lib.on_device_of(x):
            _lib.check(_lib.load().a2p_vq_encode(_lib.ptr(x), B, T, self.residual_depth, self.categories, self.latent_dim, self.n_vertices,
                                                 arr(books), arr(norms), arr(ws), arr(bs), _lib.ptr(q), _lib.ptr(lat),
                                                 _lib.current_stream(x.device)), "a2p_vq_encode")
        return q if tokens else lat

    def encode(self, poses: torch.Tensor) -> torch.Tensor:
        """poses [B, T, n_vertices] (keyframe-rate rows in the normalised space) -> int64 [B, T, residual_depth]
        (reference :499-506: the causal encoder, then the residual nearest-code search, lowest index on an exact tie)."""
        return self._encode(poses, tokens=True)

    predict = encode                  # reference :495-497
