"""Orchestration of sampling with the reference's function surface
(reference sample/generate.py:74-152: `_run_single_diffusion`, `_generate_sequences`,
the results dict keys `motions/audio/gt/lengths/keyframes`).

Dataset loading, the guide transformer (`_replace_keyframes`) and rendering are outside the
accelerated path; callers pass `model_kwargs` directly
(y: cond_embed|audio, keyframes, mask, lengths ...) and an `inv_transform` callable
(data_loaders/data.py:71-110 semantics: x * std + mean).
"""
from __future__ import annotations

from typing import Callable, Dict, NamedTuple, Optional

import numpy as np
import torch

import itertools

from .. import _lib
from ..sample_parallel import derive_seed, per_sample_noise, sample_parallel, shared_base_seed

_CALLS = itertools.count()   # sampling calls of this process: every rank makes the same calls in the same order


class PoseGuidance(NamedTuple):
    """How the body model is guided when audio and keyframes are not moved by one scale (FiLMTransformer._guidance)."""
    scale: float                      # y["scale"]: the audio's guidance scale
    mode: str                         # y["guidance"]: "audio" | "dual"
    keyframe_scale: Optional[float]   # y["scale_keyframes"] of "dual"


def pose_guidance_plan(pose_scale: float, pose_guidance: str = "joint", pose_keyframe_scale: Optional[float] = None):
    """The entry points' `pose_scale`, `pose_guidance`, `pose_keyframe_scale` checked on the host: `pose_scale` itself for "joint"
    (the body's y is then what it always was), else a PoseGuidance.  A2PError names an unknown mode, "dual" without a keyframe
    scale, a keyframe scale given to another mode, and a keyframe scale that is no finite number."""
    if not isinstance(pose_guidance, str) or pose_guidance not in _lib.GUIDANCE_MODES:
        raise _lib.A2PError(f"pose_guidance = {pose_guidance!r}: expected one of {sorted(_lib.GUIDANCE_MODES)}")
    if pose_guidance != "dual":
        if pose_keyframe_scale is not None:
            raise _lib.A2PError(f"pose_keyframe_scale = {pose_keyframe_scale!r} goes with pose_guidance = 'dual' (got {pose_guidance!r})")
        return pose_scale if pose_guidance == "joint" else PoseGuidance(float(pose_scale), pose_guidance, None)
    if pose_keyframe_scale is None:
        raise _lib.A2PError("pose_guidance = 'dual' needs pose_keyframe_scale: the guidance scale of the keyframes")
    if isinstance(pose_keyframe_scale, bool) or not isinstance(pose_keyframe_scale, (int, float)) or not np.isfinite(pose_keyframe_scale):
        raise _lib.A2PError(f"pose_keyframe_scale = {pose_keyframe_scale!r} is not a finite number")
    return PoseGuidance(float(pose_scale), "dual", float(pose_keyframe_scale))


def pose_scale_entries(pose_scale, B: int, device) -> Dict[str, object]:
    """The guidance entries of the body model's y for B sequences: "scale" alone for a plain number, plus "guidance" (and
    "scale_keyframes") for a PoseGuidance."""
    if not isinstance(pose_scale, PoseGuidance):
        return {"scale": torch.full((B,), float(pose_scale), device=device)}
    out = {"scale": torch.full((B,), pose_scale.scale, device=device), "guidance": pose_scale.mode}
    if pose_scale.keyframe_scale is not None:
        out["scale_keyframes"] = torch.full((B,), pose_scale.keyframe_scale, device=device)
    return out


def check_pose_capacity(pose_scale, pose_denoiser, B: int) -> None:
    """A2PError when "dual" guidance of B sequences (3B in the denoiser) does not fit the pose model's context (2 * max_batch)."""
    if isinstance(pose_scale, PoseGuidance) and pose_scale.mode == "dual":
        cap = max(int(pose_denoiser.max_batch), B)
        if 3 * B > 2 * cap:
            raise _lib.A2PError(f"pose_guidance = 'dual' runs 3 x {B} = {3 * B} sequences, the pose model's max_batch={cap} holds {2 * cap}: "
                                f"construct it with max_batch >= {(3 * B + 1) // 2}")


def fixseed(seed: int) -> None:
    """utils/misc.py:138-142."""
    import random
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)


def load_data_stats(path: str) -> Dict[str, np.ndarray]:
    """A subject's `data_stats.pth` (numpy arrays `pose_mean/std[104]`, `code_mean/std[256]`, `audio_mean[2]`,
    `audio_std_flat[1]`, ...; data_loaders/data.py:100-110)."""
    return torch.load(path, map_location="cpu", weights_only=False)


def make_inv_transform(stats: Dict[str, np.ndarray]) -> Callable:
    """`Social.inv_transform` (data_loaders/data.py:71-91) over the statistics `Social._load_std` picks (:100-110): pose and
    face use the per-channel mean / std, audio the per-channel mean and the FLAT std.  Like the reference, tensors are scaled
    by `torch.tensor(std)` in the statistics' own dtype, so fp32 pose / face data comes back as float64."""
    table = {"pose": (np.asarray(stats["pose_std"]).reshape(-1), np.asarray(stats["pose_mean"]).reshape(-1)),
             "face": (np.asarray(stats["code_std"]), np.asarray(stats["code_mean"])),
             "audio": (np.asarray(stats["audio_std_flat"]), np.asarray(stats["audio_mean"]))}

    def inv(data, data_type: str):
        assert data_type in table, f"datatype not defined: {data_type}"
        std, mean = table[data_type]
        if torch.is_tensor(data):
            return data * torch.tensor(std, device=data.device, requires_grad=False) \
                + torch.tensor(mean, device=data.device, requires_grad=False)
        return data * std + mean
    return inv


def _setup_model(args, state_dict, guide=None, **model_kwargs):
    """Model + diffusion for sampling (reference sample/generate.py:165-198, with the checkpoint passed in instead of read
    from args.model_path): build, load, wrap for classifier-free guidance, move to args.device, eval.
    `guide=(transformer, tokenizer)`: the guide transformer and VQ tokenizer of the body model -- the reference's constructor
    loads them from `args.resume_trans` (model/diffusion.py:244-271); here the built modules are passed in."""
    from ..model.cfg_sampler import ClassifierFreeSampleModel
    from ..model_util import create_model_and_diffusion, load_model
    model, diffusion = create_model_and_diffusion(args, "test", **model_kwargs)
    load_model(model, state_dict)
    if guide is not None:
        model.setup_guide_predictor(*guide, resume_trans=getattr(args, "resume_trans", None) or "<in-memory>")
    if not getattr(args, "unconstrained", False):
        assert args.guidance_param != 1
    if args.guidance_param != 1:
        model = ClassifierFreeSampleModel(model)
    model.to(args.device)
    model.eval()
    return model, diffusion


def save_results(output_dir: str, data_block: Dict[str, np.ndarray]) -> str:
    """`results.npy` exactly as the reference writes it (sample/generate.py:282-285): a pickled dict."""
    import os
    os.makedirs(output_dir, exist_ok=True)
    npy_path = os.path.join(output_dir, "results.npy")
    np.save(npy_path, data_block)
    return npy_path


def load_results(npy_path: str) -> Dict[str, np.ndarray]:
    """reference sample/generate.py:288."""
    return np.load(npy_path, allow_pickle=True).item()


def _replace_keyframes(model_kwargs, model, uniforms: Optional[torch.Tensor] = None, top_p: Optional[float] = None,
                       known: Optional[torch.Tensor] = None, known_mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Keyframes predicted by the guide transformer instead of ground truth (reference sample/generate.py:51-71):
    `model.transformer.generate` -> `[B, T, residual_depth]` tokens -> `model.tokenizer.decode`.  The condition is
    `y["cond_embed"]` (audio features) when present, else `y["audio"]` through the transformer's `audio_frontend`.
    `top_p`: the nucleus of the token sampling (None = `generate`'s default, as reference sample/generate.py:60-65 leaves it;
    the demo passes 0.97, demo/demo.py:77-83).

    `known` (normalised poses [B, T, nv]) with `known_mask` (bool [B, T]): keyframes whose pose is given.  `model.tokenizer.encode`
    turns `known` into tokens (its causal encoder reads every row, masked or not: pass the best poses there are, or zeros), all
    `residual_depth` tokens of each known keyframe are forced in the guide's draw, the others are drawn after them, and the
    known rows of the result are `known`'s rows verbatim (the free rows are the decode).  The reference trained both routes on
    real poses: the body on `motion[::30]` (data_loaders/data.py:191), the guide teacher-forced on `tokenizer.predict` of those
    (train/train_guide.py:64-92)."""
    if known is None and known_mask is None:
        return _guide_keyframes(model_kwargs, model, uniforms, top_p)[0]
    y = model_kwargs["y"]
    B, T, nv = y["keyframes"].shape
    known, known_mask = check_known_keyframes(known, known_mask, B, T, nv)
    tok = model.tokenizer
    dev = model.transformer.final_layer.weight.device
    with torch.no_grad():
        kt = tok.encode(known.to(dev))
        m = known_mask.to(dev)
        forced = torch.where(m[:, :, None], kt, torch.full_like(kt, -1)).reshape(B, -1)
        pred, _ = _guide_keyframes(model_kwargs, model, uniforms, top_p, forced)
    return torch.where(known_mask.cpu()[:, :, None], known.cpu(), pred)


def check_known_keyframes(known, known_mask, B: int, T: int, nv: int):
    """(known fp32 [B, T, nv], known_mask bool [B, T]) or A2PError; host checks of `_replace_keyframes(known=...)`."""
    if not torch.is_tensor(known) or not torch.is_tensor(known_mask):
        raise _lib.A2PError("known and known_mask must both be tensors")
    if tuple(known.shape) != (B, T, nv) or not known.is_floating_point():
        raise _lib.A2PError(f"known must be floating point [{B}, {T}, {nv}] (got {known.dtype} {tuple(known.shape)})")
    if known_mask.dtype != torch.bool or tuple(known_mask.shape) != (B, T):
        raise _lib.A2PError(f"known_mask must be bool [{B}, {T}] (got {known_mask.dtype} {tuple(known_mask.shape)})")
    if not bool(torch.isfinite(known).all()):
        raise _lib.A2PError("known holds non-finite values")
    return known.to(torch.float32), known_mask


def _guide_keyframes(model_kwargs, model, uniforms=None, top_p=None, forced_tokens=None):
    """(decoded keyframes [B, T, nv] on the host, tokens int64 [B, T, residual_depth] on the device) of one guide launch."""
    y = model_kwargs["y"]
    B, T = y["keyframes"].shape[0], y["keyframes"].shape[1]
    cond = y["cond_embed"] if "cond_embed" in y else y["audio"]
    nucleus = {} if top_p is None else {"top_p": float(top_p)}
    forced = {} if forced_tokens is None else {"forced_tokens": forced_tokens}
    with torch.no_grad():
        tokens = model.transformer.generate(cond, T, layers=model.tokenizer.residual_depth, n_sequences=B, max_key_len=T,
                                            max_seq_len=30 * T, uniforms=uniforms, **nucleus, **forced)
    tokens = tokens.reshape((B, -1, model.tokenizer.residual_depth))
    pred = model.tokenizer.decode(tokens).detach().cpu()
    assert y["keyframes"].shape == pred.shape, f"{y['keyframes'].shape} vs {pred.shape}"
    return pred, tokens


def _run_single_diffusion(args, model_kwargs, diffusion, model, inv_transform: Callable, gt: Optional[torch.Tensor],
                          noise: Optional[torch.Tensor] = None, rep_i: Optional[int] = None, call_i: Optional[int] = None):
    """One ddim_sample_loop over the (possibly rank-sharded) batch + un-normalisation (reference :74-107).

    Under torch.distributed every random draw is a function of (shared base seed, repetition, GLOBAL sample id): the initial
    noise via `per_sample_noise`, the guide transformer's uniforms from one generator all ranks seed alike -- so the gathered
    result does not depend on the world size, the keyframes rank 0 saves are the ones every rank conditioned on, and every
    repetition of every sampling call draws fresh noise like the reference's `randn` does: seed = derive_seed(base, call,
    repetition, global id), where `call` counts the sampling calls of this process (`call_i`; `_generate_sequences` takes one
    number for all its repetitions; every rank makes the same calls in the same order)."""
    import torch.distributed as dist
    sharded = dist.is_available() and dist.is_initialized()
    base = shared_base_seed() if sharded else None
    call = next(_CALLS) if call_i is None else int(call_i)
    rep = 0 if rep_i is None else int(rep_i)
    has_guide = getattr(args, "resume_trans", None) is not None or getattr(model, "resume_trans", None) is not None
    if args.data_format == "pose" and has_guide:   # reference :82-83
        y = model_kwargs["y"]
        uniforms = None
        if sharded:
            n = y["keyframes"].shape[1] * model.tokenizer.residual_depth
            uniforms = torch.rand(n, y["keyframes"].shape[0], generator=torch.Generator().manual_seed(derive_seed(base, call, rep, 0x6775696465)))
        y["keyframes"] = _replace_keyframes(model_kwargs, model, uniforms).to(y["keyframes"].device)
    shape = (args.batch_size, model.nfeats, 1, args.curr_seq_length)
    if noise is None and sharded:
        noise = per_sample_noise(shape, [derive_seed(base, call, rep, g) for g in range(shape[0])])
    with torch.no_grad():
        sample = sample_parallel(diffusion.ddim_sample_loop, model, shape, model_kwargs, noise=noise,
                                 clip_denoised=False, init_image=None, progress=False, dump_steps=None, const_noise=False)
    sample = inv_transform(sample.cpu().permute(0, 2, 3, 1), args.data_format).permute(0, 3, 1, 2)
    y = model_kwargs["y"]
    curr_audio = inv_transform(y["audio"].cpu().numpy(), "audio") if "audio" in y else None
    keyframes = inv_transform(y["keyframes"].cpu(), args.data_format) if "keyframes" in y else None
    gt_seq = None if gt is None else inv_transform(gt.cpu().permute(0, 2, 3, 1), args.data_format).permute(0, 3, 1, 2)
    return sample, curr_audio, keyframes, gt_seq


def _generate_sequences(args, model_kwargs, diffusion, model, inv_transform: Callable, gt: Optional[torch.Tensor] = None):
    """Repetition loop + results dict (reference :110-152)."""
    motions, lengths, audio, gts, kfs = [], [], [], [], []
    call_i = next(_CALLS)   # two calls of one process (another clip, or the same clip again) must not reuse each other's noise
    for rep_i in range(args.num_repetitions):
        if args.guidance_param != 1:
            model_kwargs["y"]["scale"] = torch.ones(args.batch_size, device=args.device) * args.guidance_param
            # args.pose_guidance / args.pose_keyframe_scale (sample/dataset.py --pose_guidance, --pose_keyframe_scale): body model only
            plan = pose_guidance_plan(args.guidance_param, getattr(args, "pose_guidance", "joint"), getattr(args, "pose_keyframe_scale", None))
            if isinstance(plan, PoseGuidance):
                model_kwargs["y"].update(pose_scale_entries(plan, args.batch_size, args.device))
        model_kwargs["y"] = {k: v.to(args.device) if torch.is_tensor(v) else v for k, v in model_kwargs["y"].items()}
        sample, curr_audio, keyframes, gt_seq = _run_single_diffusion(args, model_kwargs, diffusion, model, inv_transform, gt,
                                                                      rep_i=rep_i, call_i=call_i)
        motions.append(sample.cpu().numpy())
        if curr_audio is not None:
            audio.append(curr_audio)
        if keyframes is not None:
            kfs.append(keyframes.cpu().numpy())
        if gt_seq is not None:
            gts.append(gt_seq.cpu().numpy())
        if "lengths" in model_kwargs["y"]:
            lengths.append(model_kwargs["y"]["lengths"].cpu().numpy())
    cat = lambda xs: np.concatenate(xs, axis=0) if xs else None
    return {"motions": cat(motions), "audio": cat(audio), "gt": cat(gts), "lengths": cat(lengths), "keyframes": cat(kfs)}
