"""FiLMTransformer: drop-in for the reference denoiser on the sampling path.

Mirrors `model/diffusion.py:82-403` of the reference at its *interface*:
constructor arguments, the attributes callers read (`nfeats, cond_mode,
add_frame_cond, step, resume_trans, transformer, tokenizer`),
`forward(x, times, y, cond_drop_prob)` and the `state_dict()` key layout, so
reference checkpoints load unchanged and `ClassifierFreeSampleModel` /
`SpacedDiffusion` drive it as they drive the reference.

Nothing is computed in PyTorch: the torch sub-modules below are parameter
*containers* (they give the reference key names and initialisers); `forward`
hands device pointers to liba2p_hip.so, which runs the hand-written gfx950
kernels (csrc/).  Everything that does not depend on (x_t, t) -- the
conditioning-token path, the face cond-encoder, the audio / keyframe K,V of every
decoder layer, the unconditional branch -- is hoisted into `a2p_prepare_cond`
and cached per `y` (the reference recomputes it in every step and CFG pass,
model/diffusion.py:355-381).

The audio front end (vq-wav2vec conv stack + lip regressor, model/diffusion.py:285-313)
is part of the hoisted work: with `audio_frontend="native"` the module owns `audio_model`
/ `lip_model` like the reference does and takes the reference's `y["audio"]`
(model/audio_frontend.py, csrc/a2p_frontend.h; once per clip instead of twice per step).
`y["cond_embed"]` (the front end's output) is accepted too and takes precedence; any
other callable `audio_frontend(audio) -> cond_embed` works as well.
"""
from __future__ import annotations

import ctypes as C
from typing import Callable, Dict, Optional

import torch
import torch.nn as nn
from torch.nn import functional as F

from .. import _lib
from ..spec import DenoiserSpec

# "fp16": the 16-bit throughput mode with IEEE-half operands (liba2p_hip_f16.so, csrc/a2p_common.h A2P_HALF) -- same speed as
# bf16, 8x smaller operand rounding error; "bf16" is the dtype BASELINE's configs name and the default throughput mode
_PRECISIONS = {"fp32": _lib.PREC_F32, "f32": _lib.PREC_F32, "bf16": _lib.PREC_BF16, "fp16": _lib.PREC_BF16, "f16": _lib.PREC_BF16}
_HALF = ("fp16", "f16")


def init_weight(m: nn.Module) -> None:
    """xavier-normal weights, zero bias (reference model/utils.py:29-38)."""
    if isinstance(m, (nn.Conv1d, nn.Linear, nn.ConvTranspose1d)):
        nn.init.xavier_normal_(m.weight)
        if m.bias is not None:
            nn.init.constant_(m.bias, 0)


class RotaryEmbedding(nn.Module):
    """Holds the `freqs` buffer (rotary_embedding_torch.py:99-114); the rotation itself
    is fused into the LayerNorm kernel (csrc/kernels_misc.h: ln_rope_kernel)."""

    def __init__(self, dim: int, theta: float = 10000.0):
        super().__init__()
        self.register_buffer("freqs", 1.0 / (theta ** (torch.arange(0, dim, 2)[: dim // 2].float() / dim)))


class SinusoidalPosEmb(nn.Module):
    """Parameter-free slot 0 of `time_mlp` (model/utils.py:67-79); computed in the HIP time path."""

    def __init__(self, dim: int):
        super().__init__()
        self.dim = dim


class DenseFiLM(nn.Module):
    def __init__(self, d: int):
        super().__init__()
        self.block = nn.Sequential(nn.Mish(), nn.Linear(d, 2 * d))


class _EncoderLayerParams(nn.Module):
    """Parameter layout of TransformerEncoderLayerRotary (transformer_modules.py:36-66)."""

    def __init__(self, d, nhead, ff, dropout, rotary):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d, nhead, dropout=dropout, batch_first=True)
        self.linear1 = nn.Linear(d, ff)
        self.linear2 = nn.Linear(ff, d)
        self.norm1 = nn.LayerNorm(d)
        self.norm2 = nn.LayerNorm(d)
        self.rotary = rotary


class _DecoderLayerParams(nn.Module):
    """Parameter layout of FiLMTransformerDecoderLayer (transformer_modules.py:127-175)."""

    def __init__(self, d, nhead, ff, dropout, rotary, use_cm):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d, nhead, dropout=dropout, batch_first=True)
        self.multihead_attn = nn.MultiheadAttention(d, nhead, dropout=dropout, batch_first=True)
        self.linear1 = nn.Linear(d, ff)
        self.linear2 = nn.Linear(ff, d)
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(d), nn.LayerNorm(d), nn.LayerNorm(d)
        self.film1, self.film2, self.film3 = DenseFiLM(d), DenseFiLM(d), DenseFiLM(d)
        if use_cm:
            self.multihead_attn2 = nn.MultiheadAttention(d, nhead, dropout=dropout, batch_first=True)
            self.norm2a = nn.LayerNorm(d)
            self.film2a = DenseFiLM(d)
        self.rotary = rotary


class DecoderLayerStack(nn.Module):
    def __init__(self, stack: nn.ModuleList):
        super().__init__()
        self.stack = stack


class FiLMTransformer(nn.Module):
    def __init__(self, args, nfeats: int, latent_dim: int = 512, ff_size: int = 1024, num_layers: int = 4,
                 num_heads: int = 4, dropout: float = 0.1, cond_feature_dim: int = 4800,
                 activation: Callable = F.gelu, use_rotary: bool = True, cond_mode: str = "audio",
                 split_type: str = "train", device: str = "cuda", audio_frontend=None, audio_resample: str = "sinc", audio_geometry=None,
                 precision: str = "fp32", max_batch: int = 32, auto_escalate: bool = True, **kwargs) -> None:
        super().__init__()
        if not use_rotary:
            raise NotImplementedError("--not_rotary (absolute PE) is not on the accelerated path")
        if cond_mode != "audio":
            raise NotImplementedError("only cond_mode='audio' is on the accelerated path")
        if activation is not F.gelu:
            raise NotImplementedError("the reference factory always passes F.gelu (utils/model_util.py:66)")
        self.nfeats = nfeats
        self.cond_mode = cond_mode
        self.cond_feature_dim = cond_feature_dim
        self.add_frame_cond = args.add_frame_cond
        self.data_format = args.data_format
        self.split_type = split_type
        self.device = device
        self.seq_len = args.max_seq_length
        self.audio_frontend = audio_frontend          # None | callable(audio) -> cond_embed | "native" (set up below)
        self.precision = precision
        self.max_batch = max_batch
        self.last_logit_max = float("-inf")           # largest attention logit of the denoiser evaluations covered by the last check_finite()
        # 16-bit modes outside their validated range (a2p_precision_verdict): True = move this model to precision="fp32" for good the
        # first time that happens and tell the sampling loop to repeat the call; False = rounds 1-4's behaviour (warn, return the result)
        self.auto_escalate = auto_escalate
        self.escalated_from: Optional[str] = None     # the precision this model was constructed with, once it has escalated
        self.global_batch_hint = 0                   # set by sample_parallel: size of the unsharded batch (a2p_set_batch_hint)
        d = latent_dim
        self.latent_dim, self.ff_size, self.num_layers, self.num_heads = d, ff_size, num_layers, num_heads

        self.rotary = RotaryEmbedding(dim=d)
        self.abs_pos_encoding = nn.Identity()
        self.time_mlp = nn.Sequential(SinusoidalPosEmb(d), nn.Linear(d, d * 4), nn.Mish())
        self.to_time_cond = nn.Sequential(nn.Linear(d * 4, d))
        self.to_time_tokens = nn.Sequential(nn.Linear(d * 4, d * 2), nn.Identity())
        emb_len = 1998  # same hard-coded length as model/diffusion.py:136
        self.emb_len = emb_len
        self.null_cond_embed = nn.Parameter(torch.randn(1, emb_len, d))
        self.null_cond_hidden = nn.Parameter(torch.randn(1, d))
        self.norm_cond = nn.LayerNorm(d)

        self.input_projection = nn.Linear(nfeats, d)
        if self.data_format == "pose":
            cond_feature_dim = 1024
            self.step = 30
            self.use_cm = True
            n_key = len(list(range(self.seq_len))[:: self.step])
            self.null_pose_embed = nn.Parameter(torch.randn(1, n_key, d))
            self.frame_cond_projection = nn.Linear(104, d)
            self.frame_norm_cond = nn.LayerNorm(d)
            self.resume_trans = getattr(args, "resume_trans", None) if split_type == "test" else None
            hid = max(256, nfeats)
            chans = [(nfeats, hid, 1), (hid, nfeats, 2), (nfeats, nfeats, 3), (nfeats, nfeats, 1),
                     (nfeats, nfeats, 2), (nfeats, nfeats, 3)]
            self.post_pose_layers = nn.ModuleList([nn.Conv1d(ci, co, kernel_size=3, dilation=dl) for ci, co, dl in chans])
            self.post_pose_layers.apply(init_weight)
            self.final_conv = nn.Conv1d(nfeats, nfeats, kernel_size=1)
            self.receptive_field = 25
        elif self.data_format == "face":
            self.use_cm = False
            cond_feature_dim = 1024 + 1014
            self.cond_encoder = nn.Sequential(*[_EncoderLayerParams(d, num_heads, ff_size, dropout, self.rotary)
                                                for _ in range(2)])
            self.cond_encoder.apply(init_weight)
        else:
            raise ValueError(f"unknown data_format {self.data_format}")
        self.cond_feature_dim = cond_feature_dim
        self.cond_projection = nn.Linear(cond_feature_dim, d)
        self.non_attn_cond_projection = nn.Sequential(nn.LayerNorm(d), nn.Linear(d, d), nn.SiLU(), nn.Linear(d, d))
        self.seqTransDecoder = DecoderLayerStack(nn.ModuleList(
            [_DecoderLayerParams(d, num_heads, ff_size, dropout, self.rotary, self.use_cm) for _ in range(num_layers)]))
        self.seqTransDecoder.apply(init_weight)
        self.final_layer = nn.Linear(d, nfeats)
        self.final_layer.apply(init_weight)

        if audio_frontend == "native":
            # the reference's own front end on the GPU: vq-wav2vec conv features of both channels and, for the
            # face model, the lip regressor -- the modules own the parameters under the reference's keys (`audio_model.*`,
            # `lip_model.*`), the arithmetic is csrc/a2p_frontend.h; `y["audio"]` is then all the caller passes
            from .audio_frontend import STUB, Audio2LipRegressionTransformer, NativeAudioFrontend, Wav2VecModel
            geo = audio_geometry or STUB             # audio_frontend.FAIRSEQ: fairseq's published blocks (GroupNorm, log compression, aggregator)
            self.audio_model = Wav2VecModel(group_norm=geo.a_group_norm)
            if self.data_format == "face":
                self.lip_model = Audio2LipRegressionTransformer(geometry=geo)
            for m in (self.audio_model, getattr(self, "lip_model", None)):
                if m is not None:
                    for q in m.parameters():
                        q.requires_grad = False
            self.audio_frontend = NativeAudioFrontend(self, resample=audio_resample, max_batch=max_batch, max_frames=self.seq_len, geometry=geo)

        self._ctx: Optional[C.c_void_p] = None
        self._ctx_lib = None
        self._param_list = None
        self._ctx_key = None
        self._weights_key = None
        self._cond_key = None
        self._cond_refs = None

    # ------------------------------------------------------------------ plumbing
    def spec(self) -> DenoiserSpec:
        return DenoiserSpec(self.data_format, self.nfeats, self.latent_dim, self.num_layers, self.num_heads,
                            self.ff_size, self.cond_feature_dim, self.seq_len, self.emb_len)

    def parameters_w_grad(self):
        return [p for p in self.parameters() if p.requires_grad]

    def _hot_state(self) -> Dict[str, torch.Tensor]:
        # the guide transformer / tokenizer sub-modules (setup_guide_predictor) own their native contexts
        return {k: v for k, v in self.state_dict().items()
                if not (k.endswith("rotary.freqs") or k.startswith(("transformer.", "tokenizer.", "audio_model.", "lip_model.")))}

    def setup_guide_predictor(self, transformer: nn.Module, tokenizer: nn.Module, resume_trans: str = "<in-memory>") -> None:
        """model/diffusion.py:244-271 with the modules passed in (the reference builds them from `args.json` + checkpoint files
        next to `cp_path`): attaches the guide transformer and the VQ tokenizer that `_replace_keyframes` calls."""
        assert self.data_format == "pose", "the guide transformer predicts body keyframes"
        self.tokenizer, self.transformer, self.resume_trans = tokenizer, transformer, resume_trans
        for p in list(transformer.parameters()) + list(tokenizer.parameters()):
            p.requires_grad = False
        self._param_list = None

    def _lib(self):
        return _lib.load(half=self.precision in _HALF)

    def _ensure_ctx(self, device: torch.device, batch: int):
        lib = self._lib()
        prec = _PRECISIONS[self.precision]
        cap = max(self.max_batch, batch)
        key = (str(device), prec, cap, self.precision in _HALF)
        if self._ctx is not None and self._ctx_key == key:
            return lib
        self.release()
        cfg = _lib.A2PConfig(
            data_format=_lib.POSE if self.data_format == "pose" else _lib.FACE, nfeats=self.nfeats,
            latent_dim=self.latent_dim, ff_size=self.ff_size, num_layers=self.num_layers, num_heads=self.num_heads,
            cond_feature_dim=self.cond_feature_dim, max_frames=self.seq_len, emb_len=self.emb_len,
            keyframe_dim=104, keyframe_step=30, precision=prec, max_batch=cap, reserved=0)
        ctx = C.c_void_p()
        with torch.cuda.device(device):
            _lib.check(lib.a2p_ctx_create(C.byref(cfg), C.byref(ctx)), "a2p_ctx_create")
        self._ctx, self._ctx_key, self._weights_key, self._ctx_lib = ctx, key, None, lib
        self._env_sig = _lib.env_signature()      # the context read the A2P_* switches just now
        self._hint_sent = 0
        self._guide_sent, self._guide_ref = _lib.GUIDE_JOINT, None     # a fresh context guides jointly
        self.invalidate_cond()
        return lib

    def _apply(self, fn, *args, **kwargs):
        """`.to()/.cuda()/.float()` re-seat parameter storage without touching the version counters: mark the device copy stale."""
        self._weights_key = None
        return super()._apply(fn, *args, **kwargs)

    def _weights_signature(self):
        # runs every denoising step: must stay cheap (building the state_dict here cost ~0.5-1.3 ms per step and made
        # small configurations host-bound).  In-place updates (load_state_dict, optimisers) bump `_version`;
        # storage re-seating goes through `_apply` above.
        if self._param_list is None:
            skip = {id(t) for n in ("transformer", "tokenizer", "audio_model", "lip_model") if isinstance(getattr(self, n, None), nn.Module)
                    for t in list(getattr(self, n).parameters()) + list(getattr(self, n).buffers())}
            self._param_list = [t for t in list(self.parameters()) + list(self.buffers()) if id(t) not in skip]
        return (len(self._param_list), sum(p._version for p in self._param_list))

    def _ensure_weights(self, lib, device):
        key = self._weights_signature()
        if key == self._weights_key:
            return
        state = self._hot_state()
        stream = _lib.current_stream(device)
        keep = []
        with torch.cuda.device(device):
            for name, t in state.items():
                t = t.detach().to(device=device, dtype=torch.float32).contiguous()
                keep.append(t)
                _lib.check(lib.a2p_set_weight(self._ctx, name.encode(), _lib.ptr(t), t.numel(), stream), f"a2p_set_weight({name})")
            _lib.check(lib.a2p_finalize_weights(self._ctx, stream), "a2p_finalize_weights")
        self._weights_key = key
        self.invalidate_cond()

    def invalidate_weights(self):
        """Force a re-upload on the next call (needed only after writes that bypass the version counters, e.g. `p.data.copy_`)."""
        self._weights_key = None
        self._param_list = None

    def release(self):
        if self._ctx is not None:
            (self._ctx_lib or _lib.load()).a2p_ctx_destroy(self._ctx)
            self._ctx = None
        self._cond_key = self._cond_refs = None

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass

    def set_precision(self, precision: str):
        assert precision in _PRECISIONS
        if precision != self.precision:
            self.precision = precision
            self.release()

    # ------------------------------------------------------------------ conditioning (hoisted)
    def _cond_source(self, y) -> torch.Tensor:
        """The caller-owned tensor the conditioning tokens derive from: y["cond_embed"] (front-end output) or y["audio"]."""
        if "cond_embed" in y:
            return y["cond_embed"]
        if self.audio_frontend is not None and "audio" in y:
            return y["audio"]
        raise _lib.A2PError(
            "no audio front end: pass the wav2vec(+lip) features as y['cond_embed'] "
            f"[B, n_tok, {self.cond_feature_dim}] or construct the model with audio_frontend=...")

    def _cond_embed(self, y) -> torch.Tensor:
        return y["cond_embed"] if "cond_embed" in y else self.audio_frontend(self._cond_source(y))

    def invalidate_cond(self) -> None:
        """Drop the hoisted conditioning (and the references that pin its source tensors)."""
        self._cond_key, self._cond_refs = None, None

    def prepare(self, x: torch.Tensor, y) -> None:
        """Hoist everything t-independent for this `y`.  Cached until y's tensors change: the key is address + version +
        geometry of the source tensors, and the module keeps STRONG references to them while the key is live, so the
        allocator cannot recycle a keyed address for a different clip (model/diffusion.py:355-381 recomputes all of this in
        every step and pass; here it runs once per clip, the audio front end included)."""
        _lib.require_gpu_tensor(x, "x")
        B, T = x.shape[0], x.shape[-1] if x.dim() == 4 else x.shape[1]
        lib = self._ensure_ctx(x.device, B)
        hint = int(getattr(self, "global_batch_hint", 0) or 0)
        if hint != self._hint_sent:                # sample_parallel: the size of the batch this call's block belongs to
            _lib.check(lib.a2p_set_batch_hint(self._ctx, hint), "a2p_set_batch_hint")
            self._hint_sent = hint
        sig = _lib.env_signature()
        if sig != self._env_sig:                   # an A2P_* switch changed since the context cached them (tests, A/B runs)
            _lib.check(lib.a2p_reload_env(self._ctx), "a2p_reload_env")
            self._env_sig = sig
        self._ensure_weights(lib, x.device)
        src = self._cond_source(y)
        kf = mask = None
        if self.data_format == "pose":
            kf, mask = y["keyframes"], y["mask"]
        key = (_lib.content_key(src, kf, mask), T)
        if key == self._cond_key:
            return
        ce = src if "cond_embed" in y else self.audio_frontend(src)       # the front end runs once per clip, not per step
        ce = ce.to(device=x.device, dtype=torch.float32).contiguous()
        assert ce.shape[0] == B and ce.shape[2] == self.cond_feature_dim, f"cond_embed shape {tuple(ce.shape)}"
        kf_d = mk_d = None
        n_key = 0
        if self.data_format == "pose":
            new_mask = mask[..., :: self.step].reshape(B, -1)           # y["mask"][..., ::step].squeeze((1, 2))
            kf[~new_mask.to(kf.device)] = 0.0                             # the reference pads y in place (:320)
            kf_d = kf.to(device=x.device, dtype=torch.float32).contiguous()
            mk_d = new_mask.to(device=x.device, dtype=torch.uint8).contiguous()
            n_key = kf_d.shape[1]
            assert mk_d.shape[1] == n_key, "mask[..., ::step] and keyframes disagree"
        with _lib.on_device_of(x):
            _lib.check(lib.a2p_prepare_cond(self._ctx, _lib.ptr(ce), B, ce.shape[1], _lib.ptr(kf_d), _lib.ptr(mk_d), n_key, T,
                                            _lib.current_stream(x.device)), "a2p_prepare_cond")
        # re-key AFTER the in-place zeroing above bumped kf's version; the references pin the keyed addresses
        self._cond_key = (_lib.content_key(src, kf, mask), T)
        self._cond_refs = (src, kf, mask)

    # ------------------------------------------------------------------ guidance of audio and keyframes separately
    def _guidance(self, y, B: int):
        """`y["guidance"]` and `y["scale_keyframes"]` checked on the host, before anything touches the library:
        (_lib.GUIDE_* id, scale_keyframes or None).  The mode is a Python string, never a tensor value: every shard of a batch
        takes the same plan.  absent / "joint": one scale moves both conditions (the reference); "audio": keyframes always on,
        y["scale"] guides the audio; "dual": y["scale_keyframes"] fp32 [B] guides the keyframes, y["scale"] the audio on top of
        them -- three branches, 3B sequences (INTEGRATION.md "Guiding audio and keyframes separately")."""
        mode = "joint" if y is None or y.get("guidance") is None else y["guidance"]
        if not isinstance(mode, str) or mode not in _lib.GUIDANCE_MODES:
            raise _lib.A2PError(f"y['guidance'] = {mode!r}: expected one of {sorted(_lib.GUIDANCE_MODES)}")
        if mode == "joint":
            return _lib.GUIDE_JOINT, None
        if self.data_format != "pose":
            raise _lib.A2PError(f"y['guidance'] = {mode!r} separates the audio from the keyframes: the {self.data_format} model has no "
                                "keyframes (only 'joint')")
        if mode == "audio":
            return _lib.GUIDE_AUDIO, None
        sk = y.get("scale_keyframes")
        if sk is None:
            raise _lib.A2PError("y['guidance'] = 'dual' needs y['scale_keyframes'] (fp32 [B]): the guidance scale of the keyframes")
        if not torch.is_tensor(sk) or sk.dtype != torch.float32 or tuple(sk.shape) != (B,):
            got = f"{sk.dtype} {tuple(sk.shape)}" if torch.is_tensor(sk) else type(sk).__name__
            raise _lib.A2PError(f"y['scale_keyframes'] must be a float32 tensor of shape ({B},) like y['scale'] (got {got})")
        cap = max(self.max_batch, B)              # what _ensure_ctx sizes the context for; it holds 2 * cap sequences
        if 3 * B > 2 * cap:
            raise _lib.A2PError(f"y['guidance'] = 'dual' runs 3 x {B} = {3 * B} sequences, max_batch={cap} holds {2 * cap}: construct the "
                                f"model with max_batch >= {(3 * B + 1) // 2}")
        return _lib.GUIDE_DUAL, sk

    def _send_guidance(self, guide, device) -> None:
        """Tell the context what its guided entry points evaluate (a2p_set_guidance).  Joint after joint: no call at all."""
        mode, sk = guide
        if mode == _lib.GUIDE_JOINT and self._guide_sent == _lib.GUIDE_JOINT:
            return
        skd = None if sk is None else sk.to(device=device, dtype=torch.float32).contiguous()
        _lib.check(self._lib().a2p_set_guidance(self._ctx, mode, _lib.ptr(skd)), "a2p_set_guidance")
        self._guide_sent, self._guide_ref = mode, skd       # the library reads scale_keyframes in every step: keep it alive

    # ------------------------------------------------------------------ forward
    def _run(self, x, times, y, pass_id, scale=None, guide=None) -> torch.Tensor:
        if x.dim() == 3:  # [B, T, C] accepted by the reference too (model/diffusion.py:345)
            x = x.permute(0, 2, 1).unsqueeze(2)
        x = x.to(torch.float32).contiguous()
        self.prepare(x, y)
        if guide is not None:
            self._send_guidance(guide, x.device)
        B, T = x.shape[0], x.shape[-1]
        out = torch.empty(B, T, self.nfeats, device=x.device, dtype=torch.float32)
        ts = times.to(device=x.device, dtype=torch.int64).contiguous()
        sc = None if scale is None else scale.to(device=x.device, dtype=torch.float32).contiguous()
        with _lib.on_device_of(x):
            _lib.check(self._lib().a2p_denoise_forward(self._ctx, _lib.ptr(x), _lib.ptr(ts), _lib.ptr(sc), pass_id, _lib.ptr(out),
                                                       _lib.current_stream(x.device)), "a2p_denoise_forward")
        return out

    def forward(self, x: torch.Tensor, times: torch.Tensor, y=None, cond_drop_prob: float = 0.0, *,
                keyframe_drop_prob: Optional[float] = None) -> torch.Tensor:
        """`cond_drop_prob` drops the audio (tokens and pooled hidden); `keyframe_drop_prob` drops the keyframe tokens of the body
        model, None = the same value (the reference, whose two dropout masks share one probability)."""
        kd = cond_drop_prob if keyframe_drop_prob is None else keyframe_drop_prob
        if cond_drop_prob not in (0.0, 1.0) or kd not in (0.0, 1.0):
            raise NotImplementedError("stochastic conditioning dropout is a training feature (out of scope)")
        if kd != cond_drop_prob and self.data_format != "pose":
            raise _lib.A2PError(f"keyframe_drop_prob={keyframe_drop_prob!r}: the {self.data_format} model has no keyframes")
        if kd != cond_drop_prob and kd == 1.0:
            raise NotImplementedError("audio kept with the keyframes dropped (cond_drop_prob=0, keyframe_drop_prob=1) has no pass in the "
                                      "library: no guidance mode needs that branch")
        if kd != cond_drop_prob:
            return self._run(x, times, y, _lib.PASS_KEYS)
        return self._run(x, times, y, _lib.PASS_COND if cond_drop_prob == 0.0 else _lib.PASS_UNCOND)

    def forward_cfg(self, x, times, y) -> torch.Tensor:
        """The guidance branches batched as 2B (y["guidance"] absent, "joint", "audio") or 3B ("dual") sequences + their combination
        (model/cfg_sampler.py:30-33; `_guidance`)."""
        guide = self._guidance(y, x.shape[0])
        pass_id = (_lib.PASS_CFG, _lib.PASS_CFG_AUDIO, _lib.PASS_CFG_DUAL)[guide[0]]
        return self._run(x, times, y, pass_id, y["scale"], guide)

    def wants_early_check(self) -> bool:
        return self.precision != "fp32" and self.auto_escalate

    a2p_wants_early_check = wants_early_check     # (a bare FiLMTransformer handed to the loops)

    def check_finite(self) -> Optional[str]:
        """Raise A2PError if any denoiser evaluation since the last check produced inf / nan outputs (include/a2p_hip.h
        a2p_check_finite: a device flag OR-ed by the fused step tail; reading it synchronises the stream).  The sampling loops of
        GaussianDiffusion call this after the first step and at the end of every sampling call; direct `forward` users call it when they
        want the answer.

        In the 16-bit modes it also asks the library whether the attention logits stayed inside the range those modes were validated
        on (a2p_precision_verdict; `self.last_logit_max`).  Outside it the 16-bit operand rounding costs more than the 1e-3 parity bar
        (2.6e-3 at a row maximum of 27, profiles/r04_trained_like_budget.json), so the model ESCALATES: it re-creates its context in
        precision="fp32" (exact fp32 MFMA: 1e-6..5e-6 on the same scenarios; ~9x the step time, bench.py legs.fp32), stays there
        for the rest of its life (`escalated_from` keeps the original mode), warns once (A2PPrecisionWarning) and returns
        "escalated" -- the loops then repeat the step / the call, so the samples a caller gets are inside the bar.
        `auto_escalate=False` restores the warn-and-return behaviour of rounds 1-4."""
        if self._ctx is None:
            return None
        dev = torch.device(self._ctx_key[0])
        lib = self._ctx_lib or self._lib()
        with torch.cuda.device(dev):
            stream = _lib.current_stream(dev)
            peak, outside = C.c_float(float("-inf")), C.c_int32(0)
            _lib.check(lib.a2p_precision_verdict(self._ctx, C.byref(peak), C.byref(outside), stream), "a2p_precision_verdict")
            self.last_logit_max = float(peak.value)
            rc = lib.a2p_check_finite(self._ctx, stream)      # reads AND clears the device flag
        # A 16-bit evaluation that overflowed to inf / nan is the hardest way of leaving the 16-bit envelope (the logit maximum may
        # itself be nan then and compare as "inside"): with auto_escalate it must end in the fp32 answer like any other excursion, not
        # in an exception.  Only the fp32 mode -- or a caller that switched escalation off -- raises.
        nonfinite_16bit = rc == _lib.ERR_NONFINITE and self.precision != "fp32" and self.auto_escalate
        if rc < 0 and not nonfinite_16bit:
            _lib.check(rc, "a2p_check_finite")
        elif rc < 0:
            del _lib._failed[:]                               # the failure note of the call we just absorbed
        if not outside.value and not nonfinite_16bit:
            return None
        import warnings
        if nonfinite_16bit:
            head = (f"a denoiser evaluation in precision=\"{self.precision}\" produced inf / nan (16-bit operand overflow; attention logit "
                    f"maximum {self.last_logit_max:.1f})")
        else:
            head = (f"attention logits reach {self.last_logit_max:.1f} (row maximum of q.k/sqrt(d_head)): beyond {_lib.LOGIT_ENVELOPE_FP16:g} the "
                    f"16-bit operand rounding of precision=\"{self.precision}\" costs more than the 1e-3 parity bar on the sampler's return "
                    "value (measured 2.8e-3 at 29, divergent at 54: profiles/r04_trained_like_budget.json)")
        if not self.auto_escalate:
            warnings.warn(head + "; precision=\"fp32\" is exact there", _lib.A2PPrecisionWarning, stacklevel=2)
            return None
        self.escalated_from = self.escalated_from or self.precision
        self.set_precision("fp32")              # releases the 16-bit context; weights and conditioning are rebuilt on the next call
        warnings.warn(head + "; this model now runs in precision=\"fp32\" (exact; sticky for its lifetime) and the sampling call is repeated",
                      _lib.A2PPrecisionWarning, stacklevel=2)
        return "escalated"

    def sample_step(self, sampler: int, x, t_idx, timestep_map, tables, y, noise, eta: float, clip_denoised: bool):
        """Fused p_mean_variance + ddim_sample / p_sample for one step (include/a2p_hip.h a2p_sample_step)."""
        guide = self._guidance(y, x.shape[0])
        x = x.to(torch.float32).contiguous()
        self.prepare(x, y)
        self._send_guidance(guide, x.device)
        x_next, x0 = torch.empty_like(x), torch.empty_like(x)
        sc = y["scale"].to(device=x.device, dtype=torch.float32).contiguous()
        nz = None if noise is None else noise.to(device=x.device, dtype=torch.float32).contiguous()
        with _lib.on_device_of(x):
            _lib.check(self._lib().a2p_sample_step(self._ctx, sampler, _lib.ptr(x), _lib.ptr(t_idx), _lib.ptr(timestep_map),
                                                   _lib.ptr(tables), tables.shape[1], _lib.ptr(sc), _lib.ptr(nz), float(eta),
                                                   int(bool(clip_denoised)), _lib.ptr(x_next), _lib.ptr(x0),
                                                   _lib.current_stream(x.device)), "a2p_sample_step")
        return x_next, x0

    def sample_step_windowed(self, sampler: int, x, t_idx, timestep_map, tables, y, noise, eta: float, clip_denoised: bool, starts,
                             weights, T_total: int):
        """One step of windowed joint sampling (include/a2p_hip.h a2p_sample_step_windowed): x [R*W, C, 1, T_w] windows,
        `starts` a ctypes int32 array of the W window starts, `weights` fp32 [W, T_w], `noise` global [R, C, 1, T_total] or None.
        Returns (x_next, pred_xstart) of the windows and (x_next, pred_xstart) global [R, C, 1, T_total]."""
        guide = self._guidance(y, x.shape[0])
        x = x.to(torch.float32).contiguous()
        self.prepare(x, y)
        self._send_guidance(guide, x.device)
        W = len(starts)
        B, Cf, T_w = x.shape[0], x.shape[1], x.shape[-1]
        R = B // W
        x_next, x0 = torch.empty_like(x), torch.empty_like(x)
        xg = torch.empty(R, Cf, 1, int(T_total), device=x.device, dtype=torch.float32)
        x0g = torch.empty_like(xg)
        sc = y["scale"].to(device=x.device, dtype=torch.float32).contiguous()
        nz = None if noise is None else noise.to(device=x.device, dtype=torch.float32).contiguous()
        if (B % W or sc.numel() != B or weights.dtype != torch.float32 or weights.numel() != W * T_w or not weights.is_contiguous()
                or (nz is not None and nz.numel() != xg.numel())):
            raise _lib.A2PError(f"windowed step: x {tuple(x.shape)} over {W} windows needs scale [{B}], fp32 weights [{W}, {T_w}] and "
                                f"noise [{R}, {Cf}, 1, {T_total}] (got {tuple(sc.shape)}, {tuple(weights.shape)}, "
                                f"{None if nz is None else tuple(nz.shape)})")
        with _lib.on_device_of(x):
            _lib.check(self._lib().a2p_sample_step_windowed(
                self._ctx, sampler, _lib.ptr(x), _lib.ptr(t_idx), _lib.ptr(timestep_map), _lib.ptr(tables), tables.shape[1], _lib.ptr(sc),
                _lib.ptr(nz), float(eta), int(bool(clip_denoised)), starts, _lib.ptr(weights), W, int(T_total), _lib.ptr(x_next),
                _lib.ptr(x0), _lib.ptr(xg), _lib.ptr(x0g), _lib.current_stream(x.device)), "a2p_sample_step_windowed")
        return x_next, x0, xg, x0g

    def sample_step_inpaint(self, sampler: int, x, t_idx, timestep_map, tables, y, noise, eta: float, clip_denoised: bool, known,
                            known_mask):
        """One step with held elements (include/a2p_hip.h a2p_sample_step_inpaint): a2p_sample_step whose x0 prediction takes
        `known` where `known_mask` is set.  `known` fp32 and `known_mask` uint8 are contiguous [B, C, 1, T] on x's device.
        Returns (x_next, pred_xstart)."""
        guide = self._guidance(y, x.shape[0])
        x = x.to(torch.float32).contiguous()
        if (known.dtype != torch.float32 or known_mask.dtype != torch.uint8 or known.shape != x.shape or known_mask.shape != x.shape
                or not known.is_contiguous() or not known_mask.is_contiguous() or known.device != x.device
                or known_mask.device != x.device):
            raise _lib.A2PError(f"inpaint step: x {tuple(x.shape)} needs contiguous known fp32 and known_mask uint8 of that shape on "
                                f"{x.device} (got {known.dtype} {tuple(known.shape)} on {known.device}, {known_mask.dtype} "
                                f"{tuple(known_mask.shape)} on {known_mask.device})")
        self.prepare(x, y)
        self._send_guidance(guide, x.device)
        x_next, x0 = torch.empty_like(x), torch.empty_like(x)
        sc = y["scale"].to(device=x.device, dtype=torch.float32).contiguous()
        nz = None if noise is None else noise.to(device=x.device, dtype=torch.float32).contiguous()
        with _lib.on_device_of(x):
            _lib.check(self._lib().a2p_sample_step_inpaint(self._ctx, sampler, _lib.ptr(x), _lib.ptr(t_idx), _lib.ptr(timestep_map),
                                                           _lib.ptr(tables), tables.shape[1], _lib.ptr(sc), _lib.ptr(nz), float(eta),
                                                           int(bool(clip_denoised)), _lib.ptr(known), _lib.ptr(known_mask),
                                                           _lib.ptr(x_next), _lib.ptr(x0), _lib.current_stream(x.device)),
                       "a2p_sample_step_inpaint")
        return x_next, x0

    def sample_step_steer(self, sampler: int, x, t_idx, timestep_map, tables, y, noise, eta: float, clip_denoised: bool, steer):
        """One step whose guided x0 prediction is steered towards joint targets before the clamp and the DDIM / DDPM update
        (include/a2p_hip.h a2p_sample_step_steer; sample/steer.py).  `steer`: (a2p_steer, keep-alive) of
        BodySkeleton.steer_description, targets [B T, K, 3] and weights [B T, K] on x's device.  Body model only.
        Returns (x_next, pred_xstart)."""
        guide = self._guidance(y, x.shape[0])
        x = x.to(torch.float32).contiguous()
        desc = steer[0]
        if self.nfeats != desc.P_pos:
            raise _lib.A2PError(f"steer step: the model has {self.nfeats} features, the skeleton {desc.P_pos} pose parameters "
                                "(the body model is steered)")
        self.prepare(x, y)
        self._send_guidance(guide, x.device)
        x_next, x0 = torch.empty_like(x), torch.empty_like(x)
        sc = y["scale"].to(device=x.device, dtype=torch.float32).contiguous()
        nz = None if noise is None else noise.to(device=x.device, dtype=torch.float32).contiguous()
        with _lib.on_device_of(x):
            _lib.check(self._lib().a2p_sample_step_steer(self._ctx, sampler, _lib.ptr(x), _lib.ptr(t_idx), _lib.ptr(timestep_map),
                                                         _lib.ptr(tables), tables.shape[1], _lib.ptr(sc), _lib.ptr(nz), float(eta),
                                                         int(bool(clip_denoised)), C.byref(desc), _lib.ptr(x_next), _lib.ptr(x0),
                                                         _lib.current_stream(x.device)), "a2p_sample_step_steer")
        return x_next, x0

    def sample_step_multistep(self, x, t_idx, timestep_map, coefs, y, x0_prev, clip_denoised: bool, known=None, known_mask=None):
        """One DPM-Solver++(2M) step (include/a2p_hip.h a2p_sample_step_multistep): the guided forward, then
        x_next = CX x + B x0 + P x0_prev from `coefs` fp32 [A2P_NMS, n_steps] (GaussianDiffusion._multistep_coefs).  `x0_prev`: the
        previous step's pred_xstart [B, C, 1, T], or None (first order).  `known` fp32 / `known_mask` uint8 [B, C, 1, T]: held
        elements, as sample_step_inpaint takes them, or both None.  Returns (x_next, pred_xstart)."""
        guide = self._guidance(y, x.shape[0])
        x = x.to(torch.float32).contiguous()
        if (known is None) != (known_mask is None):
            raise _lib.A2PError("multistep step: known and known_mask go together")
        if known is not None and (known.dtype != torch.float32 or known_mask.dtype != torch.uint8 or known.shape != x.shape
                                  or known_mask.shape != x.shape or not known.is_contiguous() or not known_mask.is_contiguous()
                                  or known.device != x.device or known_mask.device != x.device):
            raise _lib.A2PError(f"multistep step: x {tuple(x.shape)} needs contiguous known fp32 and known_mask uint8 of that shape on "
                                f"{x.device} (got {known.dtype} {tuple(known.shape)} on {known.device}, {known_mask.dtype} "
                                f"{tuple(known_mask.shape)} on {known_mask.device})")
        hist = None if x0_prev is None else x0_prev.to(device=x.device, dtype=torch.float32).contiguous()
        if hist is not None and hist.shape != x.shape:
            raise _lib.A2PError(f"multistep step: x0_prev {tuple(hist.shape)} does not match x {tuple(x.shape)}")
        cf = coefs.to(device=x.device, dtype=torch.float32).contiguous()
        self.prepare(x, y)
        self._send_guidance(guide, x.device)
        x_next, x0 = torch.empty_like(x), torch.empty_like(x)
        sc = y["scale"].to(device=x.device, dtype=torch.float32).contiguous()
        with _lib.on_device_of(x):
            _lib.check(self._lib().a2p_sample_step_multistep(self._ctx, _lib.ptr(x), _lib.ptr(t_idx), _lib.ptr(timestep_map), cf.shape[1],
                                                             _lib.ptr(sc), _lib.ptr(cf), _lib.ptr(hist), int(bool(clip_denoised)),
                                                             _lib.ptr(known), _lib.ptr(known_mask), _lib.ptr(x_next), _lib.ptr(x0),
                                                             _lib.current_stream(x.device)), "a2p_sample_step_multistep")
        return x_next, x0

    def sample_step_windowed_multistep(self, x, t_idx, timestep_map, coefs, y, x0_prev, clip_denoised: bool, starts, weights,
                                       T_total: int):
        """The windowed form of sample_step_multistep (include/a2p_hip.h a2p_sample_step_windowed_multistep): sample_step_windowed's
        windows and outputs, `x0_prev` the previous step's window pred_xstart [R*W, C, 1, T_w] or None.
        Returns (x_next, pred_xstart) of the windows and (x_next, pred_xstart) global [R, C, 1, T_total]."""
        guide = self._guidance(y, x.shape[0])
        x = x.to(torch.float32).contiguous()
        W = len(starts)
        B, Cf, T_w = x.shape[0], x.shape[1], x.shape[-1]
        R = B // W
        hist = None if x0_prev is None else x0_prev.to(device=x.device, dtype=torch.float32).contiguous()
        sc = y["scale"].to(device=x.device, dtype=torch.float32).contiguous()
        if (B % W or sc.numel() != B or weights.dtype != torch.float32 or weights.numel() != W * T_w or not weights.is_contiguous()
                or (hist is not None and hist.shape != x.shape)):
            raise _lib.A2PError(f"windowed multistep step: x {tuple(x.shape)} over {W} windows needs scale [{B}], fp32 weights [{W}, {T_w}] "
                                f"and x0_prev of x's shape (got {tuple(sc.shape)}, {tuple(weights.shape)}, "
                                f"{None if hist is None else tuple(hist.shape)})")
        cf = coefs.to(device=x.device, dtype=torch.float32).contiguous()
        self.prepare(x, y)
        self._send_guidance(guide, x.device)
        x_next, x0 = torch.empty_like(x), torch.empty_like(x)
        xg = torch.empty(R, Cf, 1, int(T_total), device=x.device, dtype=torch.float32)
        x0g = torch.empty_like(xg)
        with _lib.on_device_of(x):
            _lib.check(self._lib().a2p_sample_step_windowed_multistep(
                self._ctx, _lib.ptr(x), _lib.ptr(t_idx), _lib.ptr(timestep_map), cf.shape[1], _lib.ptr(sc), _lib.ptr(cf), _lib.ptr(hist),
                int(bool(clip_denoised)), starts, _lib.ptr(weights), W, int(T_total), _lib.ptr(x_next), _lib.ptr(x0), _lib.ptr(xg),
                _lib.ptr(x0g), _lib.current_stream(x.device)), "a2p_sample_step_windowed_multistep")
        return x_next, x0, xg, x0g
