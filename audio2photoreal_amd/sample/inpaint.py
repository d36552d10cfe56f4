"""Motion around fixed frames: sampling with held elements (MDM's x0 replacement), clip continuation and segment re-rolls.

`inpaint_sample_loop` is `ddim_sample_loop` / `p_sample_loop` in which, after every model evaluation, the held elements of the x0
prediction are overwritten with the caller's values before the DDIM / DDPM update (csrc/kernels_inpaint.h
inpaint_step_tail_kernel, fused into the step tail).  The initial state is plain noise; the held elements are not q-sampled in.

`continue_recording` extends a clip when more audio arrives: the last `context_frames` frames of the previous result are held at
the start of a window that also covers the new audio, so the new motion starts from where the clip ended.  `regenerate_segment`
re-rolls frames [start, end) of a result, face, body or both, and holds the rest of a window around them.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from .. import _lib
from ..diffusion.gaussian_diffusion import GaussianDiffusion
from ..sample_parallel import derive_seed, per_sample_noise
from .generate import _replace_keyframes, check_pose_capacity, pose_guidance_plan, pose_scale_entries
from .long_form import KEYFRAME_STEP, recording_frames
from .recording import (MULTISTEP, SAMPLE_RATE, SAMPLES_PER_FRAME, _audio_stats, _check_sampler, _denoiser, _overlapped, can_share_features,
                        prepare_recording)

_SAMPLERS = {"ddim": _lib.SAMPLER_DDIM, "ddpm": _lib.SAMPLER_DDPM}

# derive_seed stream ids: generate_from_recording draws 1 (keyframe uniforms), 2 (body noise) and 3 (face noise)
_CONT_PARTNER, _CONT_UNIFORMS, _CONT_POSE, _CONT_FACE = 4, 5, 6, 7
_REGEN_UNIFORMS, _REGEN_POSE, _REGEN_FACE = 8, 9, 10


def _check_mask(known_mask, B: int, C: int, T: int) -> None:
    if not torch.is_tensor(known_mask) or known_mask.dtype != torch.bool:
        raise _lib.A2PError(f"known_mask must be a bool tensor (got {getattr(known_mask, 'dtype', type(known_mask).__name__)})")
    if tuple(known_mask.shape) not in ((B, T), (B, 1, 1, T), (B, C, 1, T)):
        raise _lib.A2PError(f"known_mask must be [{B}, {T}], [{B}, 1, 1, {T}] or [{B}, {C}, 1, {T}] (got {tuple(known_mask.shape)})")


def expand_mask(known_mask: torch.Tensor, B: int, C: int, T: int) -> torch.Tensor:
    """bool [B, T], [B, 1, 1, T] (frames) or [B, C, 1, T] (elements) -> contiguous uint8 [B, C, 1, T], 1 = held."""
    _check_mask(known_mask, B, C, T)
    return known_mask.reshape(B, -1, 1, T).expand(B, C, 1, T).to(torch.uint8).contiguous()


def inpaint_sample_loop(diffusion, model, y, known: torch.Tensor, known_mask: torch.Tensor, noise: Optional[torch.Tensor],
                        sampler: str = "ddim", eta: float = 0.0, step_noise=None, clip_denoised: bool = False, skip_timesteps: int = 0,
                        progress: bool = False) -> torch.Tensor:
    """`ddim_sample_loop` / `p_sample_loop` with held elements (include/a2p_hip.h a2p_sample_step_inpaint).

    `model`: a ClassifierFreeSampleModel; `known`: fp32 [B, C, 1, T] in the model's normalised space; `known_mask`: bool [B, T],
    [B, 1, 1, T] or [B, C, 1, T], True = held (expanded once per call); `noise`: the initial state [B, C, 1, T] (None: randn);
    `step_noise` as the plain loops take it.  Without `step_noise`, DDPM steps and DDIM steps with eta != 0 draw randn per step.
    The loop is GaussianDiffusion._loop: skip_timesteps, the finite checks and the fp32 escalation repeat work as in the plain loops.

    `sampler="dpm++2m"`: DPM-Solver++(2M) over the same steps (GaussianDiffusion.dpm_solver_sample_loop; a2p_sample_step_multistep
    with known / known_mask): held elements replace x0 after the clamp, and the history of the second-order update is the previous
    step's pred_xstart, held elements included.  It is deterministic: eta != 0 or `step_noise` is refused.

    Returns the final pred_xstart for "ddim" (its held elements are `known`'s bits), the final sample for "ddpm" and "dpm++2m" (for
    the latter the last step's pred_xstart bits).  PLMS, a model without a2p_sample_step_inpaint (a2p_sample_step_multistep for
    "dpm++2m"), and wrong shapes, dtypes or devices raise A2PError before any GPU work."""
    multistep = sampler == MULTISTEP
    if sampler not in _SAMPLERS and not multistep:
        raise _lib.A2PError(f"inpainting runs 'ddim', 'ddpm' or '{MULTISTEP}' (got {sampler!r}; PLMS is not supported)")
    if multistep:
        GaussianDiffusion.check_multistep_args(2, eta, step_noise)
    need = "a2p_sample_step_multistep" if multistep else "a2p_sample_step_inpaint"
    if not hasattr(model, need):
        raise _lib.A2PError(f"inpainting needs this package's ClassifierFreeSampleModel ({need})")
    if not torch.is_tensor(known) or known.dim() != 4 or known.shape[2] != 1:
        raise _lib.A2PError(f"known must be a [B, C, 1, T] tensor (got {tuple(getattr(known, 'shape', ()))})")
    if known.dtype != torch.float32:
        raise _lib.A2PError(f"known must be float32 (got {known.dtype})")
    B, Cf, _, T = known.shape
    _check_mask(known_mask, B, Cf, T)
    if noise is not None and (not torch.is_tensor(noise) or tuple(noise.shape) != tuple(known.shape)):
        raise _lib.A2PError(f"noise must be [{B}, {Cf}, 1, {T}] (got {tuple(getattr(noise, 'shape', ()))})")
    _lib.require_gpu_tensor(known, "known")
    device = known.device
    for name, t in (("known_mask", known_mask), ("noise", noise)):
        if t is not None and t.device != device:
            raise _lib.A2PError(f"{name} is on {t.device}, known on {device}")
    known_c = known.contiguous()
    mask_u8 = expand_mask(known_mask, B, Cf, T)
    tmap = diffusion._timestep_map(device)
    if multistep:
        coefs = diffusion._multistep_coefs(device)

        def ms_step(model, img, t, x0_prev, model_kwargs=None):
            x_next, x0 = model.a2p_sample_step_multistep(img, t.to(torch.int64).contiguous(), tmap, coefs, model_kwargs["y"], x0_prev,
                                                         clip_denoised, known_c, mask_u8)
            return {"sample": x_next, "pred_xstart": x0}

        def run_ms():
            final = None
            for out in diffusion._multistep_loop(ms_step, model, (B, Cf, 1, T), noise, {"y": y}, device, progress, skip_timesteps,
                                                 None, False):
                final = out
            return final["sample"]
        return diffusion._run_call(run_ms, model, device)
    sid = _SAMPLERS[sampler]
    tables = diffusion._tables(device)

    def step(model, img, t, model_kwargs=None, noise=None, **_):
        if noise is None and (sid == _lib.SAMPLER_DDPM or eta != 0.0):
            noise = torch.randn_like(img)
        x_next, x0 = model.a2p_sample_step_inpaint(sid, img, t.to(torch.int64).contiguous(), tmap, tables, model_kwargs["y"], noise,
                                                   eta, clip_denoised, known_c, mask_u8)
        return {"sample": x_next, "pred_xstart": x0}

    def run():
        final = None
        for out in diffusion._loop(step, model, (B, Cf, 1, T), noise, {"y": y}, device, progress, skip_timesteps, None, False,
                                   step_noise):
            final = out
        return final["pred_xstart" if sid == _lib.SAMPLER_DDIM else "sample"]
    return diffusion._run_call(run, model, device)


# ------------------------------------------------------------------------------------------------------------ recording level

def _check_models(face, pose, need_encoder: bool = False):
    face_m, pose_m = face[0], pose[0]
    fm, pm = _denoiser(face_m), _denoiser(pose_m)
    for name, m in (("face", fm), ("pose", pm)):
        if getattr(m, "audio_frontend", None) is None:
            raise _lib.A2PError(f"the {name} model has no audio front end: construct it with audio_frontend=\"native\"")
    if getattr(pm, "transformer", None) is None or getattr(pm, "tokenizer", None) is None:
        raise _lib.A2PError("the pose model has no guide transformer: attach it with setup_guide_predictor(transformer, tokenizer)")
    if need_encoder:
        require_encoder(pm)
    return fm, pm


def require_encoder(pm) -> None:
    """Keyframes from known poses need the encode side of the pose model's tokenizer."""
    if not getattr(pm.tokenizer, "has_encoder", False):
        raise _lib.A2PError("keyframes from known poses need the tokenizer's encoder: build TemporalVertexCodec(..., with_encoder=True) "
                            "and load its encoder.enc.* weights")


def _result_arrays(result, name: str):
    """(face [R, T, 256], pose [R, T, 104], audio float64 [2, T * 1600]) of a result dict, checked for shape and finiteness."""
    try:
        face, pose, audio = (np.asarray(result[k]) for k in ("face", "pose", "audio"))
    except (KeyError, TypeError):
        raise _lib.A2PError(f"{name} must be a result dict of generate_from_recording / continue_recording") from None
    if face.ndim != 3 or pose.ndim != 3 or face.shape[:2] != pose.shape[:2] or audio.ndim != 2 or audio.shape[0] != 2:
        raise _lib.A2PError(f"{name}: face [R, T, C], pose [R, T, C] and audio [2, L] expected (got {face.shape}, {pose.shape}, "
                            f"{audio.shape})")
    T = face.shape[1]
    if audio.shape[1] != T * SAMPLES_PER_FRAME:
        raise _lib.A2PError(f"{name}: {T} frames need {T * SAMPLES_PER_FRAME} audio samples (got {audio.shape[1]})")
    if not all(np.isfinite(a).all() for a in (face, pose, audio)):
        raise _lib.A2PError(f"{name} holds non-finite values")
    return face, pose, audio


def _window_audio(dual: np.ndarray, stats, R: int, device) -> torch.Tensor:
    """prepare_recording's z-normalisation of an un-normalised float64 dual audio [2, L] (csrc/kernels_audio.h dual_audio_kernel:
    float32((v - mean_c) / std) in float64), tiled over R: fp32 [R, L, 2] on `device`."""
    mean0, mean1, std = _audio_stats(stats)
    z = np.stack([(dual[0] - mean0) / std, (dual[1] - mean1) / std], axis=1).astype(np.float32)
    return torch.from_numpy(z).to(device)[None].expand(R, -1, -1).contiguous()


def _normalised(values: np.ndarray, mean, std, device) -> torch.Tensor:
    """[R, T, C] un-normalised motion -> fp32 [R, C, 1, T] in the model's space: ((v - mean) / std) in float64, cast to fp32."""
    z = ((np.asarray(values, np.float64) - np.asarray(mean, np.float64)) / np.asarray(std, np.float64)).astype(np.float32)
    return torch.from_numpy(np.ascontiguousarray(z.transpose(0, 2, 1)))[:, :, None].to(device)


def _conditions(face_m, pose_m, fm, pm, audio, share_features: bool):
    """The guide / body / face conditioning of generate_from_recording for one window's y["audio"]."""
    from ..model.audio_frontend import NativeAudioFrontend
    if share_features and can_share_features(face_m, pose_m):
        feats = pm.audio_frontend.encode_audio(audio)
        return ({"cond_embed": feats},
                {"cond_embed": pm.audio_frontend.encode_lip(audio, feats) if pm.audio_frontend.has_lip else feats},
                {"cond_embed": fm.audio_frontend.encode_lip(audio, feats) if fm.audio_frontend.has_lip else feats})
    if getattr(pm.transformer, "audio_frontend", None) is not None:
        guide_cond = {"audio": audio}
    elif isinstance(pm.audio_frontend, NativeAudioFrontend):
        guide_cond = {"cond_embed": pm.audio_frontend.encode_audio(audio)}
    else:
        raise _lib.A2PError("the guide transformer has no audio front end and the pose model's is not the native one: "
                            "construct GuideTransformer(audio_frontend=callable)")
    return guide_cond, {"audio": audio}, {"audio": audio}


def _inpaint_window(face, pose, audio, R: int, Tw: int, known_face, known_pose, mask, ids, seed: int,
                    top_p: float, face_scale: float, pose_scale: float, overlap: bool, share_features: bool, known_kf=None,
                    sampler: str = "ddim"):
    """Denoise one window of Tw frames with held elements: face and / or body (a part whose known tensor is None is not run).
    `known_kf`: None, or (normalised poses [R, Tw / 30, 104], bool mask [R, Tw / 30]) of keyframes the guide is forced to.
    Returns (face [R, C, 1, Tw] or None, body [R, C, 1, Tw] or None, keyframes [R, Tw / 30, 104] normalised, or None)."""
    face_m, face_d = face
    pose_m, pose_d = pose
    fm, pm = _denoiser(face_m), _denoiser(pose_m)
    device = fm.null_cond_embed.device
    check_pose_capacity(pose_scale, pm, R)
    nk = len(range(Tw)[::KEYFRAME_STEP])
    uni_id, pose_id, face_id = ids
    uniforms = torch.stack([torch.rand(nk * pm.tokenizer.residual_depth, generator=torch.Generator().manual_seed(derive_seed(seed, uni_id, r)))
                            for r in range(R)], dim=1)
    noise_pose = per_sample_noise((R, pm.nfeats, 1, Tw), [derive_seed(seed, pose_id, r) for r in range(R)]).to(device)
    noise_face = per_sample_noise((R, fm.nfeats, 1, Tw), [derive_seed(seed, face_id, r) for r in range(R)]).to(device)
    with torch.no_grad():
        guide_cond, body_cond, face_cond = _conditions(face_m, pose_m, fm, pm, audio, share_features)
        y_face = {**face_cond, "scale": torch.full((R,), float(face_scale), device=device)}
        y_body = {**body_cond, "mask": torch.ones(R, 1, 1, Tw, dtype=torch.bool, device=device),
                  **pose_scale_entries(pose_scale, R, device)}   # (pose_scale: a number, or generate.PoseGuidance)

        def run_face():
            return inpaint_sample_loop(face_d, face_m, y_face, known_face, mask, noise_face, sampler=sampler)

        def run_body():
            guide_y = {**guide_cond, "keyframes": torch.zeros(R, nk, pm.nfeats, device=device)}
            kk = {} if known_kf is None else {"known": known_kf[0], "known_mask": known_kf[1]}
            y_body["keyframes"] = _replace_keyframes({"y": guide_y}, pose_m, uniforms, top_p=top_p, **kk).to(device)
            return inpaint_sample_loop(pose_d, pose_m, y_body, known_pose, mask, noise_pose, sampler=sampler)

        face_s = body_s = None
        if known_face is not None and known_pose is not None and overlap:
            face_s, body_s = _overlapped(face, pose, run_face, run_body, device)
        else:
            if known_face is not None:
                face_s = run_face()
            if known_pose is not None:
                body_s = run_body()
    return face_s, body_s, (y_body["keyframes"] if body_s is not None else None)


def _motion(sample: torch.Tensor, mean, std) -> np.ndarray:
    return sample.squeeze(2).cpu().numpy().transpose(0, 2, 1) * std + mean


def continue_recording(face, pose, stats: Dict[str, np.ndarray], waveform, sr: int, previous: Dict[str, object], context_frames: int = 120,
                       num_repetitions: Optional[int] = None, top_p: float = 0.97, face_scale: float = 10.0, pose_scale: float = 2.0,
                       seed: int = 10, overlap: bool = True, share_features: bool = True,
                       guide_context: bool = False, sampler: str = "ddim", pose_guidance: str = "joint",
                       pose_keyframe_scale: Optional[float] = None) -> Dict[str, object]:
    """Continue a clip with new audio: face and body motion for `waveform` that starts from where `previous` ended.

    `previous`: a result of generate_from_recording or of an earlier continue_recording (its "face", "pose" and "audio" are read).
    `waveform` / `sr`: the NEW audio only, at any rate; it goes through prepare_recording (whole 4 s blocks, a seeded partner-noise
    draw) and is peak-normalised on its own, so a chunk's level does not follow the previous chunk's.

    One window of P = `context_frames` frames of the previous clip followed by the T_new new frames is denoised (ddim) by
    inpaint_sample_loop: all face and body channels of its first P frames are held at `previous`'s last P frames, normalised with
    `stats` in float64 and cast to fp32.  Its audio is the last P * 1600 samples of previous["audio"] followed by the new chunk's
    dual audio, z-normalised as prepare_recording does and tiled over the repetitions; the guide transformer predicts the window's
    keyframes from that audio alone (it is not told about the held frames).  `guide_context=True` tells it: the window's first
    P / 30 keyframes are the held frames 0, 30, ..., P - 30 verbatim, and their VQ tokens (the pose tokenizer's `encode`; it must
    be built with an encoder) are forced in the guide's draw, so the keyframes after them follow on from them.  Every random draw is a function of `seed` and the
    repetition index, so the result does not depend on `overlap`; pass a new seed per chunk for fresh noise.  `sampler`: "ddim" or
    "dpm++2m" (inpaint_sample_loop), over the steps the diffusions were built with.

    `pose_guidance` / `pose_keyframe_scale`: how the body model is guided, as generate_from_recording takes them ("joint", "audio"
    or "dual" with a keyframe scale; "dual" runs 1.5x the sequences and needs the pose model's max_batch >= ceil(1.5 x batch)).

    Returns generate_from_recording's keys for the NEW frames only -- {"face": [R, T_new, 256], "pose": [R, T_new, 104],
    "keyframes": [R, T_new / 30, 104], "audio": float64 [2, T_new * 1600], "T": T_new, "sr": 48000} -- plus "context": P.
    Concatenating `previous` with it along frames gives the continued clip, and it is itself a valid `previous`.

    Raises A2PError before any GPU work when P is not a positive multiple of 30 or exceeds the previous clip, when P + T_new exceeds
    the models' seq_len, when num_repetitions differs from previous's, when `previous` is not finite, for an unknown sampler and
    for what prepare_recording refuses."""
    _check_sampler(sampler)
    pose_scale = pose_guidance_plan(pose_scale, pose_guidance, pose_keyframe_scale)
    fm, pm = _check_models(face, pose, guide_context)
    prev_face, prev_pose, prev_audio = _result_arrays(previous, "previous")
    R, T_prev = prev_face.shape[:2]
    if num_repetitions is not None and int(num_repetitions) != R:
        raise _lib.A2PError(f"num_repetitions = {num_repetitions} but previous holds {R} repetitions")
    P = context_frames
    if int(P) != P or P <= 0 or P % KEYFRAME_STEP:
        raise _lib.A2PError(f"context_frames must be a positive multiple of {KEYFRAME_STEP} (got {P})")
    P = int(P)
    if P > T_prev:
        raise _lib.A2PError(f"context_frames = {P} but the previous clip has {T_prev} frames")
    T_new = recording_frames(waveform, sr)
    seq_len = min(fm.seq_len, pm.seq_len)
    if P + T_new > seq_len:
        raise _lib.A2PError(f"{P} context frames + {T_new} new frames exceed the models' seq_len = {seq_len}: use fewer context "
                            "frames or a shorter chunk")
    device = fm.null_cond_embed.device
    prep = prepare_recording(waveform, sr, stats, R, derive_seed(seed, _CONT_PARTNER) & 0xFFFFFFFF, device, max_frames=T_new)
    assert prep.T == T_new
    Tw = P + T_new
    dual = np.concatenate([prev_audio[:, (T_prev - P) * SAMPLES_PER_FRAME:], prep.dual_audio], axis=1)
    audio = _window_audio(dual, stats, R, device)

    def held(prev, mean, std):
        known = torch.zeros(R, prev.shape[2], 1, Tw, dtype=torch.float32)
        known[:, :, :, :P] = _normalised(prev[:, T_prev - P:], mean, std, "cpu")
        return known.to(device)
    mask = torch.zeros(R, Tw, dtype=torch.bool)
    mask[:, :P] = True
    mask = mask.to(device)
    known_pose = held(prev_pose, stats["pose_mean"], stats["pose_std"])
    known_kf = None
    if guide_context:
        nk, nc = len(range(Tw)[::KEYFRAME_STEP]), P // KEYFRAME_STEP
        kf_mask = torch.zeros(R, nk, dtype=torch.bool)
        kf_mask[:, :nc] = True
        known_kf = (known_pose[:, :, 0, ::KEYFRAME_STEP].transpose(1, 2).contiguous(), kf_mask)
    face_s, body_s, kf = _inpaint_window(face, pose, audio, R, Tw, held(prev_face, stats["code_mean"], stats["code_std"]),
                                         known_pose, mask, (_CONT_UNIFORMS, _CONT_POSE, _CONT_FACE), seed, top_p, face_scale,
                                         pose_scale, overlap, share_features, known_kf, sampler)
    kf = kf.cpu().numpy()[:, P // KEYFRAME_STEP:]
    return {"face": _motion(face_s, stats["code_mean"], stats["code_std"])[:, P:],
            "pose": _motion(body_s, stats["pose_mean"], stats["pose_std"])[:, P:],
            "keyframes": kf * stats["pose_std"] + stats["pose_mean"],
            "audio": prep.dual_audio, "T": T_new, "sr": SAMPLE_RATE, "context": P}


def segment_window(T: int, start: int, end: int, seq_len: int):
    """The window [ws, we) regenerate_segment denoises: the whole clip when T <= seq_len, else seq_len frames rounded down to the
    30-frame grid, on that grid, containing [start, end) and centred on it as far as the clip allows.  Host only."""
    if T <= seq_len:
        return 0, T
    Tw = seq_len // KEYFRAME_STEP * KEYFRAME_STEP
    if end - start > Tw:
        raise _lib.A2PError(f"a segment of {end - start} frames does not fit the models' window of {Tw} frames")
    ws = start - (Tw - (end - start)) // 2 // KEYFRAME_STEP * KEYFRAME_STEP
    ws = max(0, min(ws, (T - Tw) // KEYFRAME_STEP * KEYFRAME_STEP))
    return ws, ws + Tw


def regenerate_segment(face, pose, stats: Dict[str, np.ndarray], result: Dict[str, object], start_frame: int, end_frame: int,
                       parts: Sequence[str] = ("face", "pose"), top_p: float = 0.97, face_scale: float = 10.0, pose_scale: float = 2.0,
                       seed: int = 10, overlap: bool = True, share_features: bool = True,
                       guide_context: bool = False, sampler: str = "ddim", pose_guidance: str = "joint",
                       pose_keyframe_scale: Optional[float] = None) -> Dict[str, object]:
    """Re-roll frames [start_frame, end_frame) of a result and keep everything else.

    `result`: a dict with "face" [R, T, 256], "pose" [R, T, 104] and "audio" float64 [2, T * 1600] (generate_from_recording,
    continue_recording, generate_from_long_recording).  The window (segment_window) is the whole clip when it has at most seq_len
    frames, else seq_len frames on the 30-frame grid around the segment; its audio is the matching slice of result["audio"],
    z-normalised as prepare_recording does.  For every part in `parts` ("face", "pose" or both) the window is denoised (ddim) by
    inpaint_sample_loop with all its frames outside the segment held at the result's values (normalised with `stats`); the body's
    keyframes are predicted again from the window's audio.  `guide_context=True` (with "pose" in `parts`): every keyframe of the
    window outside [start, end) is the result's pose at that frame, verbatim, and its VQ tokens are forced in the guide's draw (the
    pose tokenizer must be built with an encoder).  The draw inside the segment follows the forced keyframes before it, and the
    body model is conditioned on all of them, the ones after the segment included.  Random draws are functions of `seed` and the repetition index.
    `sampler`: "ddim" or "dpm++2m" (inpaint_sample_loop), over the steps the diffusions were built with.

    `pose_guidance` / `pose_keyframe_scale`: how the body model is guided, as generate_from_recording takes them ("joint", "audio"
    or "dual" with a keyframe scale; "dual" runs 1.5x the sequences and needs the pose model's max_batch >= ceil(1.5 x batch)).

    Returns a copy of `result` in which only the listed parts' frames [start, end) are new: frames outside the segment and parts not
    listed are the input's arrays verbatim.  When the body is regenerated and result["keyframes"] is [R, T / 30, 104], its rows
    [start / 30, end / 30) are the new keyframes; other keyframe layouts are returned unchanged.

    Raises A2PError before any GPU work for bounds that are not multiples of 30 inside the clip with start < end, a segment longer
    than the window, unknown or no parts, an unknown sampler, and a result that is not finite."""
    _check_sampler(sampler)
    pose_scale = pose_guidance_plan(pose_scale, pose_guidance, pose_keyframe_scale)
    fm, pm = _check_models(face, pose)
    res_face, res_pose, res_audio = _result_arrays(result, "result")
    R, T = res_face.shape[:2]
    parts = tuple(parts) if not isinstance(parts, str) else (parts,)
    if not parts or any(p not in ("face", "pose") for p in parts):
        raise _lib.A2PError(f"parts must name 'face', 'pose' or both (got {parts!r})")
    if guide_context and "pose" in parts:
        require_encoder(pm)
    s, e = start_frame, end_frame
    if int(s) != s or int(e) != e or s % KEYFRAME_STEP or e % KEYFRAME_STEP or not 0 <= s < e <= T:
        raise _lib.A2PError(f"the segment [{start_frame}, {end_frame}) must have bounds that are multiples of {KEYFRAME_STEP} with "
                            f"0 <= start < end <= {T}")
    s, e = int(s), int(e)
    ws, we = segment_window(T, s, e, min(fm.seq_len, pm.seq_len))
    Tw = we - ws
    device = fm.null_cond_embed.device
    audio = _window_audio(res_audio[:, ws * SAMPLES_PER_FRAME:we * SAMPLES_PER_FRAME], stats, R, device)
    mask = torch.ones(R, Tw, dtype=torch.bool)
    mask[:, s - ws:e - ws] = False
    mask = mask.to(device)
    known_face = _normalised(res_face[:, ws:we], stats["code_mean"], stats["code_std"], device) if "face" in parts else None
    known_pose = _normalised(res_pose[:, ws:we], stats["pose_mean"], stats["pose_std"], device) if "pose" in parts else None
    known_kf = None
    if guide_context and known_pose is not None:
        kf_mask = torch.ones(R, len(range(Tw)[::KEYFRAME_STEP]), dtype=torch.bool)
        kf_mask[:, s // KEYFRAME_STEP - ws // KEYFRAME_STEP:e // KEYFRAME_STEP - ws // KEYFRAME_STEP] = False
        # every row, the segment's old poses included: the tokenizer's causal encoder reads them for the keyframes after it
        known_kf = (known_pose[:, :, 0, ::KEYFRAME_STEP].transpose(1, 2).contiguous(), kf_mask)
    face_s, body_s, kf = _inpaint_window(face, pose, audio, R, Tw, known_face, known_pose, mask,
                                         (_REGEN_UNIFORMS, _REGEN_POSE, _REGEN_FACE), seed, top_p, face_scale, pose_scale, overlap,
                                         share_features, known_kf, sampler)
    out = dict(result)
    if face_s is not None:
        new = np.array(result["face"], copy=True)
        new[:, s:e] = _motion(face_s, stats["code_mean"], stats["code_std"])[:, s - ws:e - ws]
        out["face"] = new
    if body_s is not None:
        new = np.array(result["pose"], copy=True)
        new[:, s:e] = _motion(body_s, stats["pose_mean"], stats["pose_std"])[:, s - ws:e - ws]
        out["pose"] = new
        old_kf = result.get("keyframes")
        if old_kf is not None and np.shape(old_kf) == (R, len(range(T)[::KEYFRAME_STEP]), pm.nfeats):
            new_kf = np.array(old_kf, copy=True)
            k0 = ws // KEYFRAME_STEP
            new_kf[:, s // KEYFRAME_STEP:e // KEYFRAME_STEP] = \
                (kf.cpu().numpy() * stats["pose_std"] + stats["pose_mean"])[:, s // KEYFRAME_STEP - k0:e // KEYFRAME_STEP - k0]
            out["keyframes"] = new_kf
    return out
