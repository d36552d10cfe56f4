"""Steering body joints to 3D targets while sampling: reach a point, look at a point.

Guidance on the x0 prediction (GMD and OmniControl style): after every model evaluation the guided x0 prediction of each frame is
moved a few descent steps towards the constraints -- through a backward pass of the skeleton solve, not of the denoiser -- and
the DDIM / DDPM update then runs as usual (include/a2p_hip.h a2p_sample_step_steer, csrc/kernels_steer.h).

    targets = JointTargets(skeleton, B, T)
    targets.aim("head", slice(0, T), camera_position)             # the head's z axis towards the camera
    targets.reach("r_wrist", slice(100, 160), point, ramp=15)     # a hand at a point, fading in and out over 15 frames
    result = generate_steered(face, pose, stats, waveform, sr, skeleton, targets)

Loss of a frame, with p = global_scaling * t_j the position of joint j (the units of skinning.pose_motion's "joints"):
    reach   w / 2 |p - y|^2
    aim     w (1 - rot(q_j, axis) . d),  d = (y - p) / |y - p| held constant; 0 when y = p
Update, in the sampler's z-scored space (pose = mean + std z, g = std dL/dpose), `iterations` times per step:
    z <- z - min(alpha L / |g|^2, max_step / |g|inf) g
the first bound Polyak's step for a loss whose optimum is 0, the second a trust region: no element moves more than `max_step`
standard deviations per iteration, so an unreachable target (small gradient, large loss) cannot throw the pose.

Out of scope, refused with A2PError: the "dpm++2m" sampler, PLMS, windowed long-form sampling (clips longer than the models'
seq_len), and steering combined with held elements (sample/inpaint.py)."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch

from .. import _lib
from ..skinning import AIM, REACH, BodySkeleton, JointConstraints, check_axis

_SAMPLERS = {"ddim": _lib.SAMPLER_DDIM, "ddpm": _lib.SAMPLER_DDPM}


class JointTargets:
    """The constraints of a [B, T] batch of frames, built on the host: every `reach` / `aim` call adds one constraint (at most
    16) with dense targets [B, T, 3] and weights [B, T] that are zero outside its frames.  Everything is validated here, before
    any GPU work."""

    def __init__(self, skeleton: BodySkeleton, B: int, T: int):
        if not isinstance(skeleton, BodySkeleton):
            raise _lib.A2PError(f"skeleton must be a BodySkeleton (got {type(skeleton).__name__})")
        if int(B) < 1 or int(T) < 1:
            raise _lib.A2PError(f"B and T must be >= 1 (got {B}, {T})")
        self.skeleton, self.B, self.T = skeleton, int(B), int(T)
        self.joints, self.kinds, self.axes, self._targets, self._weights = [], [], [], [], []

    @property
    def K(self) -> int:
        return len(self.joints)

    def _joint(self, joint) -> int:
        if isinstance(joint, str):
            if joint not in self.skeleton.joint_names:
                raise _lib.A2PError(f"unknown joint {joint!r}: the skeleton's joint_names hold no such name")
            return self.skeleton.joint_names.index(joint)
        if isinstance(joint, bool) or not isinstance(joint, (int, np.integer)) or not 0 <= joint < self.skeleton.J:
            raise _lib.A2PError(f"unknown joint {joint!r}: a name from joint_names or an index in [0, {self.skeleton.J})")
        return int(joint)

    def _frames(self, frames) -> np.ndarray:
        if isinstance(frames, slice):
            idx = np.arange(self.T)[frames]
            lo, hi = frames.start, frames.stop
            if any(v is not None and not -self.T <= v <= self.T for v in (lo, hi)):
                raise _lib.A2PError(f"frames {frames} reach outside [0, {self.T})")
        else:
            idx = np.asarray(frames)
            if idx.ndim != 1 or not np.issubdtype(idx.dtype, np.integer):
                raise _lib.A2PError("frames must be a slice or a 1-D integer index array")
            if idx.size and (idx.min() < 0 or idx.max() >= self.T):
                raise _lib.A2PError(f"frames reach outside [0, {self.T})")
            if np.unique(idx).size != idx.size:
                raise _lib.A2PError("frames holds a frame twice")
        if idx.size == 0:
            raise _lib.A2PError("frames selects no frame")
        return idx.astype(np.int64)

    def _add(self, kind: int, joint, frames, point, axis, weight, ramp) -> "JointTargets":
        j, idx = self._joint(joint), self._frames(frames)
        if self.K >= _lib.STEER_MAX_CONSTRAINTS:
            raise _lib.A2PError(f"more than {_lib.STEER_MAX_CONSTRAINTS} constraints")
        if isinstance(weight, bool) or not np.isscalar(weight) or not np.isfinite(weight) or weight < 0:
            raise _lib.A2PError(f"weight must be a finite number >= 0 (got {weight!r})")
        if isinstance(ramp, bool) or not isinstance(ramp, (int, np.integer)) or ramp < 0:
            raise _lib.A2PError(f"ramp must be a number of frames >= 0 (got {ramp!r})")
        pt = np.asarray(point.detach().cpu() if torch.is_tensor(point) else point, np.float64)
        if pt.shape not in ((3,), (idx.size, 3), (self.B, idx.size, 3)):
            raise _lib.A2PError(f"the target must be [3], [{idx.size}, 3] or [{self.B}, {idx.size}, 3] (got {list(pt.shape)})")
        if not np.isfinite(pt).all():
            raise _lib.A2PError("the target holds non-finite values")
        ax = check_axis(axis, "aim") if kind == AIM else np.zeros(3, np.float32)
        pt = np.broadcast_to(pt, (self.B, idx.size, 3))
        targets = np.zeros((self.B, self.T, 3), np.float32)
        weights = ramp_weights(self.T, idx, float(weight), int(ramp))
        src = nearest_frame(self.T, idx)
        on = weights > 0
        targets[:, on] = pt[:, src[on]]
        self.joints.append(j)
        self.kinds.append(kind)
        self.axes.append(ax)
        self._targets.append(targets)
        self._weights.append(np.broadcast_to(weights, (self.B, self.T)))
        return self

    def reach(self, joint, frames, position, weight: float = 1.0, ramp: int = 0) -> "JointTargets":
        """Keep `joint` (a name from joint_names or an index) at `position` over `frames` (a slice or an index array of T'
        frames).  position: [3], [T', 3] or [B, T', 3], in the units of pose_motion's "joints".  `ramp`: the weight fades
        linearly to zero over that many frames before and after the frames (a frame at distance d from the nearest listed
        frame gets weight (1 - d / (ramp + 1)) and that frame's position)."""
        return self._add(REACH, joint, frames, position, None, weight, ramp)

    def aim(self, joint, frames, point, axis=(0, 0, 1), weight: float = 1.0, ramp: int = 0) -> "JointTargets":
        """Turn `axis` (a unit vector in the joint's own frame) of `joint` towards `point` over `frames`; arguments as `reach`."""
        return self._add(AIM, joint, frames, point, axis, weight, ramp)

    def dense(self):
        """(targets [B, T, K, 3], weights [B, T, K]) float32 numpy."""
        if not self.K:
            raise _lib.A2PError("no constraint was added: call reach() or aim()")
        return np.stack(self._targets, axis=2), np.stack(self._weights, axis=2).astype(np.float32)

    def constraints(self) -> JointConstraints:
        """The kernel's form over N = B T frames, frame n = b T + t."""
        targets, weights = self.dense()
        return JointConstraints(self.joints, self.kinds, np.stack(self.axes), targets.reshape(-1, self.K, 3),
                                weights.reshape(-1, self.K), self.skeleton.J)


def nearest_frame(T: int, idx: np.ndarray) -> np.ndarray:
    """[T]: for every frame the position in `idx` of the nearest listed frame (the first listed on a tie)."""
    return np.abs(np.arange(T)[:, None] - idx[None, :]).argmin(axis=1)


def ramp_weights(T: int, idx: np.ndarray, weight: float, ramp: int) -> np.ndarray:
    """[T] float32: `weight` on the listed frames, weight (1 - d / (ramp + 1)) at distance d <= ramp from the nearest of them,
    0 beyond."""
    d = np.abs(np.arange(T)[:, None] - idx[None, :]).min(axis=1)
    return (weight * np.clip(1.0 - d / (ramp + 1.0), 0.0, 1.0)).astype(np.float32)


def _stat(v, n: int, name: str, device) -> torch.Tensor:
    t = torch.as_tensor(np.asarray(v.detach().cpu() if torch.is_tensor(v) else v, np.float32)).reshape(-1)
    if t.numel() != n or not bool(torch.isfinite(t).all()):
        raise _lib.A2PError(f"{name} must hold {n} finite values (got {t.numel()})")
    return t.to(device).contiguous()


def steered_sample_loop(diffusion, model, y, skeleton: BodySkeleton, mean, std, targets: JointTargets, noise: Optional[torch.Tensor],
                        sampler: str = "ddim", eta: float = 0.0, step_noise=None, clip_denoised: bool = False, iterations: int = 2,
                        alpha: float = 1.0, max_step: float = 0.25, skip_timesteps: int = 0, progress: bool = False, known=None,
                        known_mask=None) -> torch.Tensor:
    """`ddim_sample_loop` / `p_sample_loop` of the body model in which every step's guided x0 prediction is steered towards
    `targets` (module docstring; include/a2p_hip.h a2p_sample_step_steer).

    `model`: a ClassifierFreeSampleModel of the body model; `mean` / `std` [P_pos]: the statistics the model's space is z-scored
    with (stats["pose_mean"] / stats["pose_std"]); `targets`: JointTargets of the batch [B, T]; `noise`: the initial state
    [B, P_pos, 1, T] on the GPU; `step_noise` as the plain loops take it.  The skeleton's scale parameters are its lbs_scale.
    The loop is GaussianDiffusion._loop: skip_timesteps, the finite checks and the fp32 escalation repeat work as in the plain
    loops.  A frame whose weights are all zero is sampled exactly as the plain loop samples it given the same state.

    Returns the final pred_xstart for "ddim", the final sample for "ddpm".  Out of scope and refused with A2PError before any GPU
    work: "dpm++2m", PLMS, more frames than the model's seq_len (windowed sampling), held elements (`known` / `known_mask`)."""
    if sampler not in _SAMPLERS:
        what = {"dpm++2m": "the multistep solver keeps a history of x0 predictions that steering would have to rewrite",
                "plms": "PLMS is not supported"}.get(sampler, "unknown sampler")
        raise _lib.A2PError(f"steering runs 'ddim' or 'ddpm' (got {sampler!r}: {what})")
    if known is not None or known_mask is not None:
        raise _lib.A2PError("steering combined with held elements is out of scope: hold frames with inpaint_sample_loop, or steer")
    if not hasattr(model, "a2p_sample_step_steer"):
        raise _lib.A2PError("steering needs this package's ClassifierFreeSampleModel (a2p_sample_step_steer)")
    if not isinstance(targets, JointTargets) or targets.skeleton is not skeleton:
        raise _lib.A2PError("targets must be JointTargets built on `skeleton`")
    if not torch.is_tensor(noise) or noise.dim() != 4 or noise.shape[2] != 1:
        raise _lib.A2PError(f"noise must be a [B, C, 1, T] tensor (got {tuple(getattr(noise, 'shape', ()))})")
    B, Cf, _, T = noise.shape
    if Cf != skeleton.P_pos or model.nfeats != Cf:
        raise _lib.A2PError(f"noise has {Cf} channels, the model {model.nfeats} features, the skeleton {skeleton.P_pos} pose parameters")
    if (targets.B, targets.T) != (B, T):
        raise _lib.A2PError(f"targets cover [{targets.B}, {targets.T}] frames, noise [{B}, {T}]")
    seq_len = getattr(getattr(model, "model", model), "seq_len", None)
    if seq_len is not None and T > seq_len:
        raise _lib.A2PError(f"{T} frames exceed the model's seq_len = {seq_len}: windowed long-form sampling is out of scope for steering")
    cons = targets.constraints()
    if skeleton.P_scale and skeleton.lbs_scale is None:
        raise _lib.A2PError("the skeleton has scale parameters and no lbs_scale")
    _lib.require_gpu_tensor(noise, "noise")
    device = noise.device
    tab = skeleton._tables(device)
    tg, wt = cons.on(device)
    desc = skeleton.steer_description(tab, cons, tg, wt, _stat(mean, Cf, "mean", device), _stat(std, Cf, "std", device),
                                      tab["lbs_scale"], 0, alpha, iterations, max_step)
    sid = _SAMPLERS[sampler]
    tmap, tables = diffusion._timestep_map(device), diffusion._tables(device)

    def step(model, img, t, model_kwargs=None, noise=None, **_):
        if noise is None and (sid == _lib.SAMPLER_DDPM or eta != 0.0):
            noise = torch.randn_like(img)
        x_next, x0 = model.a2p_sample_step_steer(sid, img, t.to(torch.int64).contiguous(), tmap, tables, model_kwargs["y"], noise, eta,
                                                 clip_denoised, desc)
        return {"sample": x_next, "pred_xstart": x0}

    def run():
        final = None
        for out in diffusion._loop(step, model, (B, Cf, 1, T), noise, {"y": y}, device, progress, skip_timesteps, None, False,
                                   step_noise):
            final = out
        return final["pred_xstart" if sid == _lib.SAMPLER_DDIM else "sample"]
    return diffusion._run_call(run, model, device)


def steer_residual(skeleton: BodySkeleton, targets: JointTargets, poses: torch.Tensor) -> torch.Tensor:
    """[B, T, K]: per constraint and frame, the distance |p - y| of a reach or 1 - cos of an aim at un-normalised `poses`
    [B, T, P_pos] on the GPU (whatever the constraint's weight there), from one a2p_skin_steer call with iterations = 0: frame
    (n, k) of the call carries constraint k alone with weight 1, so its loss is d^2 / 2 or 1 - cos."""
    cons = targets.constraints()
    K, N = cons.K, cons.N
    flat = poses.reshape(N, skeleton.P_pos).to(torch.float32)
    one = JointConstraints(cons.joints, cons.kinds, cons.axes, cons.targets.repeat_interleave(K, dim=0),
                           torch.eye(K).repeat(N, 1), skeleton.J)
    loss, _ = skeleton.joint_loss_grad(flat.repeat_interleave(K, dim=0), one)
    loss = loss.reshape(targets.B, targets.T, K)
    reach = torch.tensor([k == REACH for k in cons.kinds], device=loss.device)
    return torch.where(reach, torch.sqrt(2.0 * loss), loss)


def generate_steered(face, pose, stats: Dict[str, np.ndarray], waveform, sr: int, skeleton: BodySkeleton, targets: JointTargets,
                     num_repetitions: int = 1, top_p: float = 0.97, face_scale: float = 10.0, pose_scale: float = 2.0, seed: int = 10,
                     overlap: bool = True, share_features: bool = True, known_keyframes=None, sampler: str = "ddim",
                     pose_guidance: str = "joint", pose_keyframe_scale: Optional[float] = None, iterations: int = 2,
                     alpha: float = 1.0, max_step: float = 0.25) -> Dict[str, object]:
    """generate_from_recording with the body steered towards `targets`: the same arguments, draws and result keys, for clips of up
    to the models' seq_len (600) frames.  The face runs the plain loop, the body steered_sample_loop (ddim) with
    stats["pose_mean"] / stats["pose_std"]; `targets` is JointTargets(skeleton, num_repetitions, T) with T =
    long_form.recording_frames(waveform, sr).  Dual and audio-only pose guidance work as in generate_from_recording.

    The result also carries "steer_residual" [R, T, K]: per constraint and frame, the distance (reach) or 1 - cos (aim) of the
    returned poses (steer_residual).

    Out of scope and refused with A2PError before any GPU work: sampler "dpm++2m", PLMS, recordings longer than seq_len
    (generate_from_long_recording's windowed sampling), and held elements (continue_recording / regenerate_segment)."""
    from .generate import pose_guidance_plan
    from .long_form import recording_frames
    from .recording import (SAMPLE_RATE, _check_models, _denoiser, _face_body_runs, _known_keyframes, _overlapped, _recording_draws,
                            _unnormalised, prepare_recording)
    if sampler != "ddim":
        raise _lib.A2PError(f"generate_steered runs 'ddim' (got {sampler!r}): 'dpm++2m' and PLMS are out of scope for steering")
    face_m, face_d = face
    pose_m, pose_d = pose
    fm, pm = _denoiser(face_m), _denoiser(pose_m)
    _check_models(fm, pm)
    pose_scale = pose_guidance_plan(pose_scale, pose_guidance, pose_keyframe_scale)
    R = int(num_repetitions)
    T = recording_frames(waveform, sr)
    seq_len = min(fm.seq_len, pm.seq_len)
    if T > seq_len:
        raise _lib.A2PError(f"the recording has {T} frames, the models' seq_len is {seq_len}: windowed long-form sampling is out of "
                            "scope for steering")
    if not isinstance(targets, JointTargets) or targets.skeleton is not skeleton or (targets.B, targets.T) != (R, T):
        raise _lib.A2PError(f"targets must be JointTargets(skeleton, {R}, {T}) for this recording and num_repetitions")
    targets.constraints()
    known = None
    if known_keyframes is not None:
        from .inpaint import require_encoder
        require_encoder(pm)
        known = _known_keyframes(known_keyframes, T, stats, pm.nfeats)
    device = fm.null_cond_embed.device
    prep = prepare_recording(waveform, sr, stats, R, seed, device, max_frames=seq_len)
    assert prep.T == T
    nk = len(range(T)[::30])
    uniforms, noise_pose, noise_face = _recording_draws(seed, R, nk * pm.tokenizer.residual_depth, (pm.nfeats, fm.nfeats), T)

    def body_loop(d, m, noise, y):
        return steered_sample_loop(d, m, y, skeleton, stats["pose_mean"], stats["pose_std"], targets, noise, sampler="ddim",
                                   iterations=iterations, alpha=alpha, max_step=max_step)

    with torch.no_grad():
        run_face, run_body, y_body = _face_body_runs(face, pose, prep.audio, T, nk, uniforms, noise_face.to(device),
                                                     noise_pose.to(device), top_p, face_scale, pose_scale, "ddim", share_features,
                                                     known=known, body_loop=body_loop)
        if overlap:
            face_s, body_s = _overlapped(face, pose, run_face, run_body, device)
        else:
            face_s = run_face()
            body_s = run_body()
        out = _unnormalised(face_s, body_s, y_body["keyframes"].cpu().numpy(), stats)
        poses = torch.from_numpy(np.ascontiguousarray(out["pose"], np.float32)).to(device)
        residual = steer_residual(skeleton, targets, poses).cpu().numpy()
    return {**out, "audio": prep.dual_audio, "T": T, "sr": SAMPLE_RATE, "steer_residual": residual}
