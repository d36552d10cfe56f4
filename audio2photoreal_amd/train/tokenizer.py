"""Training the pose tokenizer on the MI355X: the reference's first training stage (train/train_vq.py on model/vqvae.py
TemporalVertexCodec) with the whole step -- forward, SmoothL1 losses, backward, AdamW, EMA codebook update -- in one C-ABI call
of five launches (`a2p_vq_train_step`, csrc/kernels_vq_train.h).

    trainer = TokenizerTrainer(TokenizerSpec(), lr=2e-4, warm_up_iter=1000, milestones=(300000,))
    trainer.init_codebooks(first_batch, seed=123)      # the reference's k-means on the first batch, once
    for keyframes in batches:                          # fp32 [B, K, 104] as CaptureBatches.batch() returns them
        trainer.step(keyframes)                        # no synchronisation
    print(trainer.losses())                            # the only read-back

What is the reference's and what is not (INTEGRATION.md "Training the tokenizer"): the arithmetic of a step is the reference's,
including its "velocity" loss that differences the channel axis and its learning-rate recipe (after the warm-up the rate stays at
lr W / (W + 1): MultiStepLR scales the rate the warm-up left).  Dead-code expiry is not built (the reference's EMA update
overwrites it in the same forward).  k-means draws its starting rows from a seeded generator of ours.  `data_format="face"`
(600 rows per sequence) is refused.  Every argument check happens before the HIP library is loaded."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import math
import os
import time
from typing import Dict, Iterable, List, Optional, Sequence

import numpy as np
import torch

from .. import _lib
from .._lib import A2PError
from ..model.vqvae import TemporalVertexCodec
from ..spec import TokenizerSpec

BETAS, ADAM_EPS, EMA_DECAY, EMA_EPS, KMEANS_ITERS = (0.9, 0.99), 1e-8, 0.99, 1e-5, 10
RECORD = ("loss", "loss_motion", "loss_commit", "loss_vel", "perplexity")
LDS_BYTES, LDS_SCRATCH = 64 * 1024, 64        # a2p_vq_train_step's LDS plan: two buffers of (T + 7) rows plus the reduction scratch


def max_rows(latent_dim: int) -> int:
    """The longest sequence one workgroup of the step holds (120 rows at latent 64)."""
    return (LDS_BYTES - LDS_SCRATCH) // (8 * latent_dim) - 7


def param_shapes(n_vertices: int, latent_dim: int):
    """Names and shapes of the reference codec's parameters() in order: the layout of the flat buffers."""
    e, nv = latent_dim, n_vertices
    s = [("encoder.enc.0.weight", (e, nv, 1)), ("encoder.enc.0.bias", (e,))]
    for i in (2, 4, 6, 8):
        s += [(f"encoder.enc.{i}.weight", (e, e, 2)), (f"encoder.enc.{i}.bias", (e,))]
    s += [("decoder.project_mean_shape.weight", (e, nv)), ("decoder.project_mean_shape.bias", (e,))]
    for i in (0, 2, 4, 6):
        s += [(f"decoder.dec.{i}.weight", (e, e, 2)), (f"decoder.dec.{i}.bias", (e,))]
    s += [("decoder.dec.8.weight", (nv, e, 1)), ("decoder.dec.8.bias", (nv,))]
    return s


def learning_rate(n: int, lr: float, warm_up_iter: int, milestones: Sequence[int], gamma: float) -> float:
    """The rate of the n-th step (0-based) of the reference's recipe: warm-up iterations it = 1 .. W - 1 at lr (it + 1) / (W + 1),
    then MultiStepLR stepped after every iteration, which scales the rate the warm-up LEFT (lr W / (W + 1)) by gamma at each
    milestone."""
    warm = max(int(warm_up_iter) - 1, 0)
    if n < warm:
        return lr * (n + 2) / (warm_up_iter + 1)
    cur = lr * warm_up_iter / (warm_up_iter + 1) if warm else lr
    for m in sorted(set(milestones)):              # scheduler.step() number m multiplies by gamma ** (times m is listed), as torch does
        if m <= n - warm:
            cur = cur * gamma ** list(milestones).count(m)
    return cur


def _check_hyper(lr, weight_decay, commit, loss_vel, warm_up_iter, milestones, gamma):
    for name, v in (("lr", lr), ("weight_decay", weight_decay), ("commit", commit), ("loss_vel", loss_vel), ("gamma", gamma)):
        if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or v < 0:
            raise A2PError(f"{name} must be a finite non-negative number (got {v!r})")
    if isinstance(warm_up_iter, bool) or not isinstance(warm_up_iter, (int, np.integer)) or warm_up_iter < 0:
        raise A2PError(f"warm_up_iter must be a non-negative integer (got {warm_up_iter!r})")
    if any(isinstance(m, bool) or not isinstance(m, (int, np.integer)) or m < 1 for m in milestones):
        raise A2PError(f"milestones must be positive iteration numbers (got {list(milestones)!r})")


def check_batch(keyframes, n_vertices: int, latent_dim: int) -> None:
    """Host-side refusals of a batch, before the library is loaded."""
    if not torch.is_tensor(keyframes) or keyframes.dim() != 3 or keyframes.shape[-1] != n_vertices or 0 in keyframes.shape:
        raise A2PError(f"keyframes must be a tensor [B, T, {n_vertices}] (got {tuple(getattr(keyframes, 'shape', ()))!r})")
    if not keyframes.dtype.is_floating_point:
        raise A2PError(f"keyframes must be floating point (got {keyframes.dtype})")
    T = keyframes.shape[1]
    if T > max_rows(latent_dim):
        raise A2PError(f"{T} rows per sequence: one workgroup of the training step holds at most {max_rows(latent_dim)} at latent "
                       f"width {latent_dim} (keyframe-rate pose sequences have 20; frame-rate data is out of scope)")
    if not keyframes.is_cuda and not bool(torch.isfinite(keyframes).all()):
        # a device batch is not checked: the read-back would synchronise every step; its NaN shows in losses()
        raise A2PError("keyframes hold non-finite values")


def kmeans(samples: torch.Tensor, num_clusters: int, generator: torch.Generator, iters: int = KMEANS_ITERS, start=None):
    """The reference's k-means (model/vqvae.py kmeans): nearest mean by squared distance, empty clusters keep their mean; the
    starting rows are drawn from `generator` (a permutation when there are enough rows, else with replacement) unless `start`
    gives them.  Plain torch ops on the samples' device: it runs once per training, not in the hot path.
    Returns (means, bins of the last assignment)."""
    n = samples.shape[0]
    if start is None:
        if n >= num_clusters:
            idx = torch.randperm(n, generator=generator)[:num_clusters]
        else:
            idx = torch.randint(0, n, (num_clusters,), generator=generator)
        start = samples[idx.to(samples.device)]
    means = start.clone()
    bins = None
    for _ in range(iters):
        d = (samples.pow(2).sum(1, keepdim=True) - 2 * samples @ means.t()) + means.pow(2).sum(1)[None]
        buckets = d.argmin(1)
        bins = torch.bincount(buckets, minlength=num_clusters)
        sums = torch.zeros_like(means).index_add_(0, buckets, samples)
        means = torch.where((bins == 0)[:, None], means, sums / bins.clamp_min(1)[:, None].to(means.dtype))
    return means, bins


def tokenizer_args(spec: TokenizerSpec) -> Dict[str, int]:
    """The args.json fields the reference's setup_tokenizer builds the codec from."""
    return {"nb_joints": spec.n_vertices, "output_emb_width": spec.latent_dim, "code_dim": spec.categories, "depth": spec.residual_depth}


def initial_parameters(shapes, seed: int = 0) -> torch.Tensor:
    """A flat host buffer with torch's default Conv1d / Linear initialisation (uniform +-1/sqrt(fan_in)) from a generator of our own."""
    g = torch.Generator().manual_seed(int(seed))
    by_name = dict(shapes)
    parts = []
    for name, shape in shapes:
        w_shape = shape if name.endswith("weight") else by_name[name[:-4] + "weight"]
        bound = 1.0 / math.sqrt(math.prod(w_shape[1:]))
        parts.append((torch.rand(math.prod(shape), generator=g) * 2 - 1) * bound)
    return torch.cat(parts)


def kmeans_codebooks(latents: torch.Tensor, categories: int, depth: int, generator: torch.Generator):
    """EuclideanCodebook.init_embed_ level by level: k-means on the residuals the previous levels leave.  latents [N, e] ->
    (means [depth x [categories, e]], bins [depth x [categories]])."""
    res, means_all, bins_all = latents, [], []
    for _ in range(depth):
        means, bins = kmeans(res, categories, generator)
        d = (res.pow(2).sum(1, keepdim=True) - 2 * res @ means.t()) + means.pow(2).sum(1)[None]
        res = res - means[d.argmin(1)]
        means_all.append(means), bins_all.append(bins)
    return means_all, bins_all


class TokenizerTrainer:
    """Owns the flat training state of a TemporalVertexCodec; `codec`'s parameters and codebooks are views of it, so
    `codec.encode` / `codec.decode` run on the trained weights with no copy."""

    def __init__(self, spec_or_codec=None, lr: float = 2e-4, weight_decay: float = 0.0, commit: float = 0.02, loss_vel: float = 0.1,
                 warm_up_iter: int = 1000, milestones: Sequence[int] = (300000,), gamma: float = 0.05, device="cuda",
                 data_format: str = "pose"):
        if data_format != "pose":
            raise A2PError(f"the tokenizer trainer covers data_format='pose' at keyframe rate only (got {data_format!r}): face "
                           "sequences have 600 rows, beyond what one workgroup of the step holds")
        src = None
        if isinstance(spec_or_codec, TemporalVertexCodec):
            src = spec_or_codec
            if not src.has_encoder:
                raise A2PError("training needs the codec's encoder: construct it with with_encoder=True")
            spec = TokenizerSpec(src.n_vertices, src.latent_dim, src.categories, src.residual_depth)
        else:
            spec = spec_or_codec if spec_or_codec is not None else TokenizerSpec()
            if not isinstance(spec, TokenizerSpec):
                raise A2PError(f"spec_or_codec must be a TokenizerSpec or a TemporalVertexCodec (got {type(spec_or_codec).__name__})")
        e, nv, depth, Cn = spec.latent_dim, spec.n_vertices, spec.residual_depth, spec.categories
        if not (1 <= depth <= 8 and e >= 4 and e % 4 == 0 and nv >= 1 and Cn >= 1 and max_rows(e) >= 1):
            raise A2PError(f"bad tokenizer shape {spec}: depth 1..8, latent width a multiple of 4 (at most {(LDS_BYTES - LDS_SCRATCH) // 64})")
        milestones = [int(m) for m in milestones] if not isinstance(milestones, (int, np.integer)) else [int(milestones)]
        _check_hyper(lr, weight_decay, commit, loss_vel, warm_up_iter, milestones, gamma)
        self.spec, self.lr, self.weight_decay, self.commit, self.loss_vel = spec, float(lr), float(weight_decay), float(commit), float(loss_vel)
        self.warm_up_iter, self.milestones, self.gamma = int(warm_up_iter), milestones, float(gamma)
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise A2PError(f"TokenizerTrainer runs on the MI355X (got device {self.device}); there is no CPU implementation")
        # ---- flat state
        dev = self.device
        self.shapes = param_shapes(nv, e)
        self.n_params = sum(math.prod(s) for _, s in self.shapes)
        f32 = dict(dtype=torch.float32, device=dev)
        self.params, self.exp_avg, self.exp_avg_sq = (torch.zeros(self.n_params, **f32) for _ in range(3))
        self.embed, self.embed_avg = torch.zeros(depth, Cn, e, **f32), torch.zeros(depth, Cn, e, **f32)
        self.cluster_size = torch.zeros(depth, Cn, **f32)
        self.record = torch.zeros(6, **f32)
        self.inited = False
        self.iteration = 0            # steps made: the warm-up iterations come first
        self._ws, self._ws_key, self._tokens = None, None, None
        self.codec = TemporalVertexCodec(nv, e, Cn, depth, with_encoder=True)
        views = self._views(self.params)
        for name, _ in self.shapes:
            if "project_mean_shape" in name:
                continue
            mod, leaf = self.codec.get_submodule(name.rsplit(".", 1)[0]), name.rsplit(".", 1)[1]
            setattr(mod, leaf, torch.nn.Parameter(views[name], requires_grad=False))
        for k, layer in enumerate(self.codec.quantizer.layers):
            layer._codebook._buffers["embed"] = self.embed[k]
        if src is not None:
            self.load_net({k: v for k, v in src.state_dict().items()}, inited=True, strict=False)
        else:
            self._init_parameters()

    # ---- state ----------------------------------------------------------------------------------------------------------
    def _views(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        out, o = {}, 0
        for name, shape in self.shapes:
            n = math.prod(shape)
            out[name] = flat[o:o + n].view(shape)
            o += n
        return out

    def _init_parameters(self, seed: int = 0) -> None:
        self.params.copy_(initial_parameters(self.shapes, seed))
        self._touched()

    def _touched(self) -> None:
        self.codec._staged = self.codec._staged_enc = None     # the kernels write the views in place: torch's version counters do not move

    def net_state_dict(self) -> Dict[str, torch.Tensor]:
        """The reference codec's exact key set, on the host."""
        v = self._views(self.params)
        sd = {n: v[n].detach().cpu().clone() for n, _ in self.shapes if n.startswith("encoder.")}
        sd.update({n: v[n].detach().cpu().clone() for n, _ in self.shapes if n.startswith("decoder.")})
        for k in range(self.spec.residual_depth):
            p = f"quantizer.layers.{k}._codebook."
            sd[p + "inited"] = torch.tensor([float(self.inited)])
            sd[p + "cluster_size"] = self.cluster_size[k].cpu().clone()
            sd[p + "embed"] = self.embed[k].cpu().clone()
            sd[p + "embed_avg"] = self.embed_avg[k].cpu().clone()
        return sd

    def load_net(self, sd: Dict[str, torch.Tensor], inited: Optional[bool] = None, strict: bool = True) -> None:
        """Parameters and codebook state from a reference-layout `net` dictionary.  Not strict: EMA statistics that are absent
        are derived as after k-means (embed_avg = embed, cluster_size = 1), project_mean_shape stays as it is."""
        v = self._views(self.params)
        for name, shape in self.shapes:
            if name not in sd:
                if strict or "project_mean_shape" not in name:
                    raise A2PError(f"the state lacks {name}")
                continue
            if tuple(sd[name].shape) != tuple(shape):
                raise A2PError(f"{name}: shape {tuple(sd[name].shape)}, expected {tuple(shape)}")
            v[name].copy_(sd[name].detach().to(torch.float32))
        flags = []
        for k in range(self.spec.residual_depth):
            p = f"quantizer.layers.{k}._codebook."
            if p + "embed" not in sd or (strict and any(p + n not in sd for n in ("embed_avg", "cluster_size", "inited"))):
                raise A2PError(f"the state lacks {p}embed / embed_avg / cluster_size / inited")
            self.embed[k].copy_(sd[p + "embed"].to(torch.float32))
            self.embed_avg[k].copy_(sd.get(p + "embed_avg", sd[p + "embed"]).to(torch.float32))
            self.cluster_size[k].copy_(sd[p + "cluster_size"].to(torch.float32) if p + "cluster_size" in sd
                                       else torch.ones(self.spec.categories))
            flags.append(bool(sd[p + "inited"].item()) if p + "inited" in sd else True)
        if len(set(flags)) != 1:
            raise A2PError("the codebooks' `inited` flags differ between levels")
        self.inited = flags[0] if inited is None else inited
        self._touched()

    def optimizer_state_dict(self) -> dict:
        """torch.optim.AdamW.state_dict() layout: parameter i of parameters(); project_mean_shape has no state, as in torch."""
        m, v = self._views(self.exp_avg), self._views(self.exp_avg_sq)
        state = {}
        if self.iteration:
            for i, (name, _) in enumerate(self.shapes):
                if "project_mean_shape" not in name:
                    state[i] = {"step": torch.tensor(float(self.iteration)), "exp_avg": m[name].cpu().clone(), "exp_avg_sq": v[name].cpu().clone()}
        group = {"lr": learning_rate(max(self.iteration - 1, 0), self.lr, self.warm_up_iter, self.milestones, self.gamma),
                 "betas": BETAS, "eps": ADAM_EPS, "weight_decay": self.weight_decay, "amsgrad": False, "maximize": False,
                 "foreach": None, "capturable": False, "differentiable": False, "fused": None, "initial_lr": self.lr,
                 "params": list(range(len(self.shapes)))}
        return {"state": state, "param_groups": [group]}

    def scheduler_state_dict(self) -> dict:
        """A plain dictionary (the reference pickles the MultiStepLR object itself)."""
        return {"iteration": self.iteration, "lr": self.lr, "warm_up_iter": self.warm_up_iter, "milestones": list(self.milestones),
                "gamma": self.gamma, "weight_decay": self.weight_decay, "commit": self.commit, "loss_vel": self.loss_vel}

    def state_dict(self) -> dict:
        return {"net": self.net_state_dict(), "optimizer": self.optimizer_state_dict(), "scheduler": self.scheduler_state_dict()}

    def args_dict(self) -> dict:
        """What the reference's setup_tokenizer reads from args.json next to a checkpoint."""
        return {**tokenizer_args(self.spec), "data_format": "pose", "lr": self.lr, "weight_decay": self.weight_decay, "commit": self.commit, "loss_vel": self.loss_vel,
                "warm_up_iter": self.warm_up_iter, "lr_scheduler": list(self.milestones), "gamma": self.gamma}

    def save(self, out_dir: str, name: str = "net_last.pth", extra_args: Optional[dict] = None) -> str:
        os.makedirs(out_dir, exist_ok=True)
        path = os.path.join(out_dir, name)
        torch.save(self.state_dict(), path)
        with open(os.path.join(out_dir, "args.json"), "w") as f:
            json.dump({**(extra_args or {}), **self.args_dict()}, f, indent=4, sort_keys=True)
        return path

    def load(self, path: str) -> None:
        """Resume from a checkpoint written by `save` (a reference checkpoint resumes its `net` and optimizer moments; its pickled
        scheduler object is not read: the schedule is this trainer's)."""
        ckpt = torch.load(path, map_location="cpu", weights_only=False)
        self.load_net(ckpt["net"], strict=True)
        opt = ckpt.get("optimizer", {"state": {}})
        m, v = self._views(self.exp_avg), self._views(self.exp_avg_sq)
        self.exp_avg.zero_(), self.exp_avg_sq.zero_()
        steps = set()
        for i, st in opt["state"].items():
            name = self.shapes[int(i)][0]
            m[name].copy_(st["exp_avg"]), v[name].copy_(st["exp_avg_sq"])
            steps.add(int(st["step"]))
        if len(steps) > 1:
            raise A2PError(f"the optimizer state holds different step counts {sorted(steps)}")
        sch = ckpt.get("scheduler")
        self.iteration = int(sch["iteration"]) if isinstance(sch, dict) and "iteration" in sch else (steps.pop() if steps else 0)
        self.record.zero_()

    # ---- training -------------------------------------------------------------------------------------------------------
    def current_lr(self) -> float:
        return learning_rate(self.iteration, self.lr, self.warm_up_iter, self.milestones, self.gamma)

    def _prepare(self, keyframes: torch.Tensor) -> torch.Tensor:
        check_batch(keyframes, self.spec.n_vertices, self.spec.latent_dim)
        return keyframes.to(device=self.device, dtype=torch.float32).contiguous()

    def _pointers(self, t: torch.Tensor):
        return (C.c_void_p * t.shape[0])(*[t[k].data_ptr() for k in range(t.shape[0])])

    def step(self, keyframes: torch.Tensor, grads_out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One training step on keyframes [B, T, n_vertices]; returns the step's tokens int64 [B, T, depth] (device, not
        synchronised).  `grads_out`: a flat fp32 device buffer like `params` that receives the gradient."""
        x = self._prepare(keyframes)
        if not self.inited:
            raise A2PError("the codebooks are not initialised: call init_codebooks(first_batch, seed) or load a checkpoint")
        if grads_out is not None and (grads_out.device != self.device or grads_out.dtype != torch.float32
                                      or grads_out.numel() != self.n_params or not grads_out.is_contiguous()):
            raise A2PError(f"grads_out must be a contiguous fp32 device tensor of {self.n_params} elements")
        s, (B, T, _) = self.spec, x.shape
        lib = _lib.load()
        key = (B, T)
        if self._ws_key != key:
            n = C.c_int64(0)
            _lib.check(lib.a2p_vq_train_workspace_bytes(B, T, s.residual_depth, s.categories, s.latent_dim, s.n_vertices, C.byref(n)),
                       "a2p_vq_train_workspace_bytes")
            self._ws, self._ws_key = torch.empty(n.value, dtype=torch.uint8, device=self.device), key
        tokens = torch.empty(B, T, s.residual_depth, dtype=torch.int64, device=self.device)
        step_no = self.iteration + 1
        hp = _lib.A2PVqTrainHyper(self.current_lr(), 1 - BETAS[0] ** step_no, 1 - BETAS[1] ** step_no, self.weight_decay, self.commit,
                                  self.loss_vel, EMA_DECAY, EMA_EPS)
        with _lib.on_device_of(x):
            _lib.check(lib.a2p_vq_train_step(_lib.ptr(x), B, T, s.residual_depth, s.categories, s.latent_dim, s.n_vertices,
                                             _lib.ptr(self.params), _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq),
                                             self._pointers(self.embed), self._pointers(self.embed_avg), self._pointers(self.cluster_size),
                                             C.byref(hp), _lib.ptr(tokens), _lib.ptr(self.record), _lib.ptr(grads_out), _lib.ptr(self._ws),
                                             self._ws.numel(), _lib.current_stream(self.device)), "a2p_vq_train_step")
        self.iteration = step_no
        self._touched()
        return tokens

    def losses(self) -> Dict[str, float]:
        """Means of the loss record since the last call, then reset: the only synchronisation of training."""
        rec = self.record.cpu().tolist()
        self.record.zero_()
        n = rec[5]
        out = {k: (rec[i] / n if n else float("nan")) for i, k in enumerate(RECORD)}
        out["steps"] = int(n)
        return out

    @torch.no_grad()
    def init_codebooks(self, keyframes: torch.Tensor, seed: int = 0) -> None:
        """The reference's k-means initialisation (EuclideanCodebook.init_embed_) level by level on the first batch's residuals:
        embed = embed_avg = the means, cluster_size = the bins; the starting rows come from torch.Generator().manual_seed(seed).
        Runs once, in plain torch ops on the GPU -- not the hot path."""
        x = self._prepare(keyframes)
        g = torch.Generator().manual_seed(int(seed))
        means, bins = kmeans_codebooks(self.codec.encoder(x).reshape(-1, self.spec.latent_dim), self.spec.categories,
                                       self.spec.residual_depth, g)
        for k in range(self.spec.residual_depth):
            self.embed[k].copy_(means[k]), self.embed_avg[k].copy_(means[k]), self.cluster_size[k].copy_(bins[k].to(torch.float32))
        self.inited = True
        self._touched()

    @torch.no_grad()
    def evaluate(self, batches: Iterable[torch.Tensor]) -> Dict[str, float]:
        """evaluation_vqvae: per sequence the eval-mode reconstruction SmoothL1, commitment (zero in eval mode, as the reference's
        quantiser returns it) and perplexity of the last level, averaged over the sequences; existing encode / decode launches."""
        recons = torch.zeros((), device=self.device, dtype=torch.float64)
        ppl = torch.zeros((), device=self.device, dtype=torch.float64)
        n = 0
        for keyframes in batches:
            x = self._prepare(keyframes)
            tok = self.codec.encode(x)
            pred = self.codec.decode(tok)
            recons += torch.nn.functional.smooth_l1_loss(pred, x, reduction="none").mean((1, 2)).double().sum()
            onehot = torch.nn.functional.one_hot(tok[..., -1], self.spec.categories).double().sum(1)      # [B, categories]
            prob = onehot / onehot.sum(1, keepdim=True)
            ppl += torch.exp(-(prob * torch.log(prob + 1e-7)).sum(1)).sum()
            n += x.shape[0]
        if not n:
            raise A2PError("evaluate() got no batch")
        return {"recons": float(recons) / n, "commit": 0.0, "perplexity": float(ppl) / n, "sequences": n}


# ---------------------------------------------------------------------------------------------------------------- the recipe
def _batches_of(cb, order: Sequence[int], batch_size: int):
    for i in range(0, len(order), batch_size):
        yield cb.batch(order[i:i + batch_size])[1]["y"]["keyframes"]


def train_tokenizer(data_root: str, out_dir: str, *, spec: Optional[TokenizerSpec] = None, batch_size: int = 64, total_iter: int = 300000,
                    warm_up_iter: int = 1000, lr: float = 2e-4, milestones: Sequence[int] = (300000,), gamma: float = 0.05,
                    weight_decay: float = 0.0, commit: float = 0.02, loss_vel: float = 0.1, print_iter: int = 200, eval_iter: int = 1000,
                    seed: int = 123, max_seq_length: int = 600, data_format: str = "pose", resume_pth: Optional[str] = None,
                    device="cuda", extra_args: Optional[dict] = None) -> "TokenizerTrainer":
    """train/train_vq.py main(): train split batches drawn from a seeded generator, warm-up, `total_iter` steps, evaluation on
    the val split with net_last.pth / net_best.pth (best perplexity) every `eval_iter`, a run.log line every `print_iter`."""
    if data_format != "pose":
        raise A2PError(f"train_tokenizer covers data_format='pose' only (got {data_format!r})")
    for name, v in (("batch_size", batch_size), ("print_iter", print_iter), ("eval_iter", eval_iter), ("max_seq_length", max_seq_length)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise A2PError(f"{name} must be a positive integer (got {v!r})")
    if isinstance(total_iter, bool) or not isinstance(total_iter, (int, np.integer)) or total_iter < 0:
        raise A2PError(f"total_iter must be a non-negative integer (got {total_iter!r})")
    if batch_size > _lib.DATASET_MAX_BATCH:
        raise A2PError(f"batch_size is at most {_lib.DATASET_MAX_BATCH} (got {batch_size})")
    spec = spec or TokenizerSpec()
    if len(range(0, max_seq_length, 30)) > max_rows(spec.latent_dim):
        raise A2PError(f"max_seq_length {max_seq_length} gives more than {max_rows(spec.latent_dim)} keyframe rows")
    from ..data import CaptureBatches, load_capture, split_indices
    from ..sample.generate import load_data_stats
    stats_path = os.path.join(data_root, "data_stats.pth")
    if not os.path.isfile(stats_path):
        raise A2PError(f"{stats_path} not found: the subject's data_stats.pth must lie in data_root")
    takes = load_capture(data_root)
    split = split_indices(len(takes))
    if not split["train"] or not split["val"]:
        raise A2PError(f"{len(takes)} takes leave no train or val split (the last 4 are test, the 2 before them val)")
    trainer = TokenizerTrainer(spec, lr=lr, weight_decay=weight_decay, commit=commit, loss_vel=loss_vel, warm_up_iter=warm_up_iter,
                               milestones=milestones, gamma=gamma, device=device)
    stats = load_data_stats(stats_path)
    train = CaptureBatches([takes[i] for i in split["train"]], stats, "pose", T=max_seq_length, seed=seed, device=device)
    val = CaptureBatches([takes[i] for i in split["val"]], stats, "pose", T=max_seq_length, seed=seed, device=device)
    os.makedirs(out_dir, exist_ok=True)
    log = open(os.path.join(out_dir, "run.log"), "a")

    def say(msg):
        line = f"{time.strftime('%Y-%m-%d %H:%M:%S')},000 INFO {msg}"
        log.write(line + "\n"), log.flush()
        print(line, flush=True)

    args = {"data_root": data_root, "out_dir": out_dir, "batch_size": batch_size, "total_iter": total_iter, "print_iter": print_iter,
            "eval_iter": eval_iter, "seed": seed, "max_seq_length": max_seq_length, "resume_pth": resume_pth, **(extra_args or {})}
    gen = torch.Generator().manual_seed(int(seed))
    draw = lambda: train.batch(torch.randint(0, len(train), (batch_size,), generator=gen).tolist())[1]["y"]["keyframes"]   # noqa: E731
    if resume_pth:
        trainer.load(resume_pth)
    else:
        trainer._init_parameters(seed)
        trainer.init_codebooks(draw(), seed)
    best = float("inf")

    def evaluate(it):
        nonlocal best
        m = trainer.evaluate(_batches_of(val, list(range(len(val))), batch_size))
        say(f"Eval. Iter {it} : \t Commit. {m['commit']:.5f} \t PPL. {m['perplexity']:.2f} \t Recons.  {m['recons']:.5f}")
        if total_iter > 0:
            trainer.save(out_dir, "net_last.pth", args)
            if m["perplexity"] < best:     # the reference's rule: net_best.pth follows the LOWER perplexity
                say(f"--> --> \t Perplexity Improved from {best:.5f} to {m['perplexity']:.5f} !!!")
                trainer.save(out_dir, "net_best.pth", args)
        best = min(best, m["perplexity"])
        return m

    warm = max(trainer.warm_up_iter - 1, 0)
    while trainer.iteration < warm:
        lr_now = trainer.current_lr()
        trainer.step(draw())
        if trainer.iteration % print_iter == 0:
            m = trainer.losses()
            say(f"Warmup. Iter {trainer.iteration} :  lr {lr_now:.5f} \t Commit. {m['loss_commit']:.5f} \t PPL. {m['perplexity']:.2f} "
                f"\t Recons.  {m['loss_motion']:.5f}")
    trainer.losses()
    if trainer.iteration == warm:
        evaluate(0)
    while trainer.iteration - warm < total_iter:
        trainer.step(draw())
        it = trainer.iteration - warm
        if it % print_iter == 0:
            m = trainer.losses()
            say(f"Train. Iter {it} : \t Commit. {m['loss_commit']:.5f} \t PPL. {m['perplexity']:.2f} \t Recons.  {m['loss_motion']:.5f}")
        if it % eval_iter == 0:
            evaluate(it)
    log.close()
    return trainer


def _parser() -> argparse.ArgumentParser:
    """The reference's argument names and defaults (utils/vq_parser_utils.py)."""
    ap = argparse.ArgumentParser(description="Train the residual-VQ pose tokenizer on the MI355X",
                                 formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    ap.add_argument("--dataname", type=str, default="kit")
    ap.add_argument("--data_root", type=str, default=None, help="capture directory of one person, with data_stats.pth")
    ap.add_argument("--max_seq_length", default=600, type=int)
    ap.add_argument("--add_frame_cond", type=float, choices=[1], default=None)
    ap.add_argument("--data_format", type=str, default="pose", choices=["pose", "face"])
    ap.add_argument("--dataset", default="social", type=str)
    ap.add_argument("--batch_size", default=64, type=int)
    ap.add_argument("--total_iter", default=300_000, type=int)
    ap.add_argument("--warm_up_iter", default=1000, type=int)
    ap.add_argument("--lr", default=2e-4, type=float)
    ap.add_argument("--lr_scheduler", default=[300_000], nargs="+", type=int)
    ap.add_argument("--gamma", default=0.05, type=float)
    ap.add_argument("--weight_decay", default=0.0, type=float)
    ap.add_argument("--commit", type=float, default=0.02)
    ap.add_argument("--loss_vel", type=float, default=0.1)
    ap.add_argument("--code_dim", type=int, default=512, help="codes per level")
    ap.add_argument("--depth", type=int, default=3, help="residual levels")
    ap.add_argument("--output_emb_width", type=int, default=512, help="latent width")
    ap.add_argument("--resume_pth", type=str, default=None)
    ap.add_argument("--out_dir", type=str, required=True)
    ap.add_argument("--print_iter", default=200, type=int)
    ap.add_argument("--eval_iter", default=1000, type=int)
    ap.add_argument("--seed", default=123, type=int)
    return ap


def main(argv: Optional[List[str]] = None) -> int:
    a = _parser().parse_args(argv)
    if a.data_root is None:
        raise A2PError("--data_root is required")
    spec = TokenizerSpec(n_vertices=104, latent_dim=a.output_emb_width, categories=a.code_dim, residual_depth=a.depth)
    train_tokenizer(a.data_root, a.out_dir, spec=spec, batch_size=a.batch_size, total_iter=a.total_iter, warm_up_iter=a.warm_up_iter,
                    lr=a.lr, milestones=a.lr_scheduler, gamma=a.gamma, weight_decay=a.weight_decay, commit=a.commit, loss_vel=a.loss_vel,
                    print_iter=a.print_iter, eval_iter=a.eval_iter, seed=a.seed, max_seq_length=a.max_seq_length,
                    data_format=a.data_format, resume_pth=a.resume_pth, extra_args={"dataname": a.dataname, "dataset": a.dataset})
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
