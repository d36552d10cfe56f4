"""From a recording to face codes and body poses: the library form of the demo's `generate_results` (demo/demo.py:156-216),
without gradio and rendering.

`prepare_recording` turns a waveform at any sample rate into the models' `y["audio"]` on the GPU (resample to 48 kHz, whole
4 s blocks, peak-normalised channel 0 + N(0, 0.001) partner channel, z-normalisation: csrc/kernels_audio.h);
`generate_from_recording` runs the face model and guide transformer -> VQ keyframes -> body model on it, with the audio
features computed once when the models' front ends are identical, and face / body on two HIP streams (`overlap=True`).
"""
from __future__ import annotations

from typing import Dict, NamedTuple, Optional

import numpy as np
import torch

from .. import _lib
from ..audio import _resample_rows, resampled_length, sinc_resample_table
from ..sample_parallel import derive_seed, per_sample_noise
from .generate import _replace_keyframes, check_pose_capacity, pose_guidance_plan, pose_scale_entries

SAMPLE_RATE = 48_000                  # the models' audio rate
BLOCK = 4 * SAMPLE_RATE               # the demo keeps whole 4 s blocks (demo/demo.py:169-171)
SAMPLES_PER_FRAME = SAMPLE_RATE // 30
MAX_FRAMES = 600                      # the denoisers' seq_len: null embeddings of 1998 audio tokens / 20 keyframes (20 s)
MULTISTEP = "dpm++2m"                 # DPM-Solver++(2M): GaussianDiffusion.dpm_solver_sample_loop
SAMPLERS = ("ddim", MULTISTEP)        # the `sampler` of the recording-level APIs


def _check_sampler(sampler) -> None:
    if sampler not in SAMPLERS:
        raise _lib.A2PError(f"sampler must be one of {SAMPLERS} (got {sampler!r})")


class PreparedRecording(NamedTuple):
    audio: torch.Tensor               # y["audio"]: z-normalised dual audio, fp32 [R, Lc, 2] on the GPU
    T: int                            # frames at 30 fps = Lc / 1600
    dual_audio: np.ndarray            # the demo's un-normalised dual audio, float64 [2, Lc] (demo/demo.py:212-216, before its float32 cast)


def _channels_last(waveform) -> torch.Tensor:
    """float32 [L, C] on the host, the demo's layout rule: 2-D input is averaged over dim 0 when it has 2 rows, else over dim 1."""
    t = waveform.detach().cpu() if torch.is_tensor(waveform) else torch.from_numpy(np.ascontiguousarray(np.asarray(waveform)))
    t = t.to(torch.float32)           # torch.Tensor(y)
    if t.dim() == 1:
        return t[:, None]
    if t.dim() == 2:
        return t.t() if t.shape[0] == 2 else t
    raise ValueError(f"a recording is [L] or 2-D [channels, L] / [L, channels] (got shape {tuple(t.shape)})")


def _audio_stats(stats):
    mean = np.asarray(stats["audio_mean"], dtype=np.float64).reshape(-1)
    std = np.asarray(stats["audio_std_flat"], dtype=np.float64).reshape(-1)
    if mean.size not in (1, 2) or std.size != 1:
        raise ValueError(f"audio_mean must hold 1 or 2 values and audio_std_flat 1 (got {mean.size}, {std.size})")
    return float(mean[0]), float(mean[-1]), float(std[0])


def prepare_recording(waveform, sr: int, stats: Dict[str, np.ndarray], num_repetitions: int, seed: int = 10, device="cuda",
                      max_frames: int = MAX_FRAMES) -> PreparedRecording:
    """demo/demo.py:159-186: mono -> torchaudio-style resample to 48 kHz -> whole 4 s blocks -> dual audio, tiled over the
    `num_repetitions` samples.  The partner channel is `np.random.RandomState(seed).normal(0, 0.001, (1, Lc, 2))[..., 1]`.

    `waveform`: [L], or 2-D averaged over `dim = 0 if shape[0] == 2 else 1` (numpy or torch, any numeric dtype, e.g. `read_wav`'s
    output).  Raises A2PError, before any GPU work, for recordings shorter than 4 s or longer than `max_frames` frames after
    resampling (longer recordings: sample.long_form.prepare_long_recording) and for num_repetitions < 1; ValueError for sr <= 0."""
    if sr <= 0 or int(sr) != sr:
        raise ValueError(f"sr must be a positive integer rate (got {sr})")
    sr = int(sr)
    if num_repetitions < 1:
        raise _lib.A2PError(f"num_repetitions must be at least 1 (got {num_repetitions})")
    x = _channels_last(waveform)
    L, C = x.shape
    if C > _lib.RESAMPLE_MAX_CHANNELS:
        raise ValueError(f"{C} channels: at most {_lib.RESAMPLE_MAX_CHANNELS}")
    Lr = resampled_length(L, sr, SAMPLE_RATE)
    if Lr < BLOCK:
        raise _lib.A2PError(f"the recording lasts {Lr / SAMPLE_RATE:.2f} s: at least 4 s are needed")
    Lc = (Lr // BLOCK) * BLOCK
    T = Lc // SAMPLES_PER_FRAME
    if T > max_frames:
        raise _lib.A2PError(f"the recording keeps {Lc // SAMPLE_RATE} s ({T} frames) but the models take at most {max_frames} frames "
                            f"({max_frames // 30} s); cut it into shorter clips")
    mean0, mean1, std = _audio_stats(stats)
    if sr != SAMPLE_RATE:
        sinc_resample_table(sr, SAMPLE_RATE)          # size check of the filter table on the host (A2PError) before any upload
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.A2PError(f"prepare_recording runs on the MI355X (got device {device}); there is no CPU implementation")

    xd = x.to(device).contiguous()
    mono = _resample_rows(xd, L, C, sr, SAMPLE_RATE)[0]                      # [Lr]
    noise = np.random.RandomState(seed).normal(0, 0.001, (1, Lc, 2))
    noise_d = torch.from_numpy(noise[0]).to(device)                          # float64 [Lc, 2]
    out = torch.empty(int(num_repetitions), Lc, 2, device=device, dtype=torch.float32)
    scratch = torch.empty(_lib.DUAL_AUDIO_SCRATCH, device=device, dtype=torch.float32)
    with _lib.on_device_of(mono):
        _lib.check(_lib.load().a2p_dual_audio(_lib.ptr(mono), Lc, _lib.ptr(scratch), _lib.ptr(noise_d), mean0, mean1, std,
                                              int(num_repetitions), _lib.ptr(out), _lib.current_stream(device)), "a2p_dual_audio")
    # the demo's float64 dual audio on the host (its return value, un-normalised again: demo/demo.py:178-186, 212-216)
    y = mono[:Lc].cpu().numpy()
    dual = noise.copy()
    dual[:, :, 0] = y / y.max()
    dual = (dual - stats["audio_mean"]) / stats["audio_std_flat"]
    dual = dual * stats["audio_std_flat"] + stats["audio_mean"]
    return PreparedRecording(out, T, np.ascontiguousarray(dual[0].T))


def _denoiser(m):
    return getattr(m, "model", m)


def _same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    if a.dtype != b.dtype or a.shape != b.shape or a.device != b.device:
        return False
    return bool(torch.equal(a.detach().contiguous().reshape(-1).view(torch.uint8), b.detach().contiguous().reshape(-1).view(torch.uint8)))


def can_share_features(face_model, pose_model) -> bool:
    """True when the two denoisers' native front ends compute the same `encode_audio` features: the same geometry, resampling,
    precision and bitwise-equal `audio_model.*` parameters (the reference loads one vq-wav2vec.pt into each model)."""
    from ..model.audio_frontend import NativeAudioFrontend
    fm, pm = _denoiser(face_model), _denoiser(pose_model)
    ff, pf = getattr(fm, "audio_frontend", None), getattr(pm, "audio_frontend", None)
    if not (isinstance(ff, NativeAudioFrontend) and isinstance(pf, NativeAudioFrontend)):
        return False
    if fm.precision != pm.precision or ff._precision() != pf._precision() or ff.geometry != pf.geometry or ff.resample != pf.resample:
        return False
    a, b = fm.audio_model.state_dict(), pm.audio_model.state_dict()
    return a.keys() == b.keys() and all(_same_bits(a[k], b[k]) for k in a)


def generate_from_recording(face, pose, stats: Dict[str, np.ndarray], waveform, sr: int, num_repetitions: int = 1, top_p: float = 0.97,
                            face_scale: float = 10.0, pose_scale: float = 2.0, seed: int = 10, overlap: bool = True,
                            share_features: bool = True, known_keyframes=None, sampler: str = "ddim",
                            pose_guidance: str = "joint", pose_keyframe_scale: Optional[float] = None) -> Dict[str, object]:
    """`generate_results` (demo/demo.py:156-216) for `num_repetitions` samples of one recording.

    `face` / `pose`: (ClassifierFreeSampleModel, SpacedDiffusion) pairs as `sample.generate._setup_model` builds them, the pose
    model with its guide transformer and VQ tokenizer attached (`setup_guide_predictor`) and both with an audio front end.
    Face: ddim_sample_loop at `face_scale`; body: keyframes from the guide transformer (nucleus `top_p`), all-true mask,
    ddim_sample_loop at `pose_scale`.  Every random draw is a function of `seed` and the repetition index (derive_seed /
    per_sample_noise), so the result does not depend on `overlap`.

    `share_features`: compute `encode_audio` once and give it to the guide, the body model and the face model's lip input when
    `can_share_features` holds (else each model runs its own front end on y["audio"]; a guide transformer without a front end
    of its own takes the body model's features).  `overlap`: face on one HIP stream, guide -> VQ decode -> body on another;
    False runs face, then body, as the demo does.

    `known_keyframes`: {frame: pose [104]} of un-normalised poses the body must take, e.g. to start or end in a given pose.  Frames
    are multiples of 30 inside the clip; the same poses apply to every repetition.  Those keyframes are the given poses (normalised
    with `stats` in float64, cast to fp32), and their VQ tokens (the pose tokenizer's `encode`; it must be built with an encoder) are
    forced in the guide's draw, so the keyframes drawn after them follow on from them.  Bad frames, shapes or non-finite poses
    raise A2PError before any GPU work.

    `sampler`: "ddim" (ddim_sample_loop) or "dpm++2m" (dpm_solver_sample_loop, DPM-Solver++(2M): second order, one model call per
    step), for face and body alike.  The number of steps is the one each SpacedDiffusion was built with (e.g.
    timestep_respacing="ddim20"); anything else raises A2PError before any GPU work.

    `pose_guidance` / `pose_keyframe_scale`: how the body model is guided (INTEGRATION.md "Guiding audio and keyframes separately").
    "joint" (the default, the reference): `pose_scale` moves audio and keyframes together.  "audio": the keyframes are followed as
    they are and `pose_scale` guides the audio alone.  "dual": `pose_keyframe_scale` guides the keyframes and `pose_scale` the audio
    on top of them; three branches per step, 1.5x the sequences, and the pose model needs max_batch >= ceil(1.5 x its batch).

    Returns {"face": [R, T, 256], "pose": [R, T, 104], "keyframes": [R, T / 30, 104] (un-normalised with the code_* / pose_*
    statistics: * std + mean), "audio": the un-normalised dual audio float64 [2, Lc], "T", "sr": 48000}."""
    face_m, face_d = face
    pose_m, pose_d = pose
    fm, pm = _denoiser(face_m), _denoiser(pose_m)
    _check_sampler(sampler)
    _check_models(fm, pm)
    pose_scale = pose_guidance_plan(pose_scale, pose_guidance, pose_keyframe_scale)
    known = None
    if known_keyframes is not None:
        from .inpaint import require_encoder
        from .long_form import recording_frames
        require_encoder(pm)
        known = _known_keyframes(known_keyframes, recording_frames(waveform, sr), stats, pm.nfeats)
    device = fm.null_cond_embed.device
    R = int(num_repetitions)
    prep = prepare_recording(waveform, sr, stats, R, seed, device, max_frames=min(fm.seq_len, pm.seq_len))
    audio, T = prep.audio, prep.T
    nk = len(range(T)[::30])
    uniforms, noise_pose, noise_face = _recording_draws(seed, R, nk * pm.tokenizer.residual_depth, (pm.nfeats, fm.nfeats), T)

    with torch.no_grad():
        run_face, run_body, y_body = _face_body_runs(face, pose, audio, T, nk, uniforms, noise_face.to(device), noise_pose.to(device),
                                                     top_p, face_scale, pose_scale, sampler, share_features, known=known)
        if overlap:
            face_s, body_s = _overlapped(face, pose, run_face, run_body, device)
        else:
            face_s = run_face()
            body_s = run_body()
    return {**_unnormalised(face_s, body_s, y_body["keyframes"].cpu().numpy(), stats),
            "audio": prep.dual_audio, "T": T, "sr": SAMPLE_RATE}


def _check_models(fm, pm) -> None:
    """A2PError unless both denoisers have an audio front end and the pose model its guide transformer and tokenizer."""
    for name, m in (("face", fm), ("pose", pm)):
        if getattr(m, "audio_frontend", None) is None:
            raise _lib.A2PError(f"the {name} model has no audio front end: construct it with audio_frontend=\"native\"")
    if getattr(pm, "transformer", None) is None or getattr(pm, "tokenizer", None) is None:
        raise _lib.A2PError("the pose model has no guide transformer: attach it with setup_guide_predictor(transformer, tokenizer)")


def _recording_draws(seed: int, R: int, n_u: int, nfeats, T: int, W: int = 1):
    """The random draws of `seed` on the host: keyframe uniforms [n_u, R * W] (column r * W + w; window 0 from derive_seed(seed,
    1, r), window w > 0 from derive_seed(seed, 1, r, w)), body noise and face noise [R, nfeats, 1, T] (derive_seed(seed, 2 / 3,
    r)).  W = 1: generate_from_recording's draws; W > 1: generate_from_long_recording's."""
    uniforms = torch.stack([torch.rand(n_u, generator=torch.Generator().manual_seed(derive_seed(seed, 1, r) if w == 0 else
                                                                                    derive_seed(seed, 1, r, w)))
                            for r in range(R) for w in range(W)], dim=1)
    noise_pose = per_sample_noise((R, nfeats[0], 1, T), [derive_seed(seed, 2, r) for r in range(R)])
    noise_face = per_sample_noise((R, nfeats[1], 1, T), [derive_seed(seed, 3, r) for r in range(R)])
    return uniforms, noise_pose, noise_face


def _conditions(face_m, pose_m, audio: torch.Tensor, share_features: bool):
    """(guide, body, face) conditioning of y["audio"] rows: the features once when `share_features` and the front ends agree,
    else each model's own front end (a guide without one takes the pose model's features)."""
    from ..model.audio_frontend import NativeAudioFrontend
    fm, pm = _denoiser(face_m), _denoiser(pose_m)
    if share_features and can_share_features(face_m, pose_m):
        feats = pm.audio_frontend.encode_audio(audio)
        guide_cond = {"cond_embed": feats}
        body_cond = {"cond_embed": pm.audio_frontend.encode_lip(audio, feats) if pm.audio_frontend.has_lip else feats}
        face_cond = {"cond_embed": fm.audio_frontend.encode_lip(audio, feats) if fm.audio_frontend.has_lip else feats}
    else:
        body_cond, face_cond = {"audio": audio}, {"audio": audio}
        if getattr(pm.transformer, "audio_frontend", None) is not None:
            guide_cond = {"audio": audio}
        elif isinstance(pm.audio_frontend, NativeAudioFrontend):
            guide_cond = {"cond_embed": pm.audio_frontend.encode_audio(audio)}
        else:
            raise _lib.A2PError("the guide transformer has no audio front end and the pose model's is not the native one: "
                                "construct GuideTransformer(audio_frontend=callable)")
    return guide_cond, body_cond, face_cond


def _face_body_runs(face, pose, audio: torch.Tensor, T: int, nk: int, uniforms, noise_face, noise_pose, top_p, face_scale, pose_scale,
                    sampler: str, share_features: bool, plan=None, known=None, chain_keyframes: bool = False, body_loop=None):
    """The conditioning of the B = audio.shape[0] sequences (computed here, on the current stream) and two closures: run_face()
    -> the face sample, run_body() -> guide keyframes into y_body["keyframes"], then the body sample.  plan None: the plain loops
    over T frames (known: the forced keyframes of generate_from_recording); else windowed_sample_loop over the plan's windows
    (rows r * W + w, T the window length, noise per global frame).  body_loop(diffusion, model, noise, y): the body's loop when it
    is not the face's (sample/steer.py)."""
    face_m, face_d = face
    pose_m, pose_d = pose
    fm, pm = _denoiser(face_m), _denoiser(pose_m)
    device = fm.null_cond_embed.device
    B = audio.shape[0]
    check_pose_capacity(pose_scale, pm, B)
    guide_cond, body_cond, face_cond = _conditions(face_m, pose_m, audio, share_features)
    y_face = {**face_cond, "scale": torch.full((B,), float(face_scale), device=device)}
    y_body = {**body_cond, "mask": torch.ones(B, 1, 1, T, dtype=torch.bool, device=device),
              **pose_scale_entries(pose_scale, B, device)}   # (pose_scale: a number, or generate.PoseGuidance)

    if plan is None:
        def loop(d, m, noise, y):
            run = d.ddim_sample_loop if sampler == "ddim" else d.dpm_solver_sample_loop
            return run(m, (B, noise.shape[1], 1, T), noise=noise, clip_denoised=False, model_kwargs={"y": y})
    else:
        from .long_form import _chained_keyframes, windowed_sample_loop

        def loop(d, m, noise, y):
            return windowed_sample_loop(d, m, plan, B // plan.W, y, noise, sampler=sampler)

    def run_face():
        return loop(face_d, face_m, noise_face, y_face)

    def run_body():
        if plan is not None and chain_keyframes and plan.W > 1:
            y_body["keyframes"] = _chained_keyframes(pose_m, plan, B // plan.W, guide_cond, uniforms, top_p, nk, pm.nfeats).to(device)
        else:
            guide_y = {**guide_cond, "keyframes": torch.zeros(B, nk, pm.nfeats, device=device)}
            kk = {} if known is None else {"known": known[0].expand(B, -1, -1), "known_mask": known[1].expand(B, -1)}
            y_body["keyframes"] = _replace_keyframes({"y": guide_y}, pose_m, uniforms, top_p=top_p, **kk).to(device)
        return (body_loop or loop)(pose_d, pose_m, noise_pose, y_body)

    return run_face, run_body, y_body


def _unnormalised(face_s: torch.Tensor, body_s: torch.Tensor, kf: np.ndarray, stats) -> Dict[str, np.ndarray]:
    """Samples [B, C, 1, T] -> {"face": [B, T, 256], "pose": [B, T, 104], "keyframes"}, un-normalised with `stats`."""
    face_np = face_s.squeeze(2).cpu().numpy().transpose(0, 2, 1)
    pose_np = body_s.squeeze(2).cpu().numpy().transpose(0, 2, 1)
    return {"face": face_np * stats["code_std"] + stats["code_mean"],
            "pose": pose_np * stats["pose_std"] + stats["pose_mean"],
            "keyframes": kf * stats["pose_std"] + stats["pose_mean"]}


def _known_keyframes(known_keyframes, T: int, stats, nv: int):
    """{frame: pose} -> (normalised fp32 [1, T / 30, nv], bool mask [1, T / 30]) on the host, or A2PError."""
    if not isinstance(known_keyframes, dict) or not known_keyframes:
        raise _lib.A2PError(f"known_keyframes must be a non-empty {{frame: pose[{nv}]}} dict")
    nk = len(range(T)[::30])
    known = np.zeros((nk, nv), np.float64)
    mask = np.zeros(nk, bool)
    mean = np.asarray(stats["pose_mean"], np.float64).reshape(-1)
    std = np.asarray(stats["pose_std"], np.float64).reshape(-1)
    for f, pose in known_keyframes.items():
        if isinstance(f, bool) or not isinstance(f, (int, np.integer)) or f % 30 or not 0 <= f < T:
            raise _lib.A2PError(f"known_keyframes: frame {f!r} must be a multiple of 30 in [0, {T})")
        v = np.asarray(pose.detach().cpu() if torch.is_tensor(pose) else pose, dtype=np.float64)
        if v.shape != (nv,):
            raise _lib.A2PError(f"known_keyframes[{f}] must be a pose of {nv} values (got shape {v.shape})")
        if not np.isfinite(v).all():
            raise _lib.A2PError(f"known_keyframes[{f}] holds non-finite values")
        known[f // 30] = (v - mean) / std
        mask[f // 30] = True
    return torch.from_numpy(known.astype(np.float32))[None], torch.from_numpy(mask)[None]


def _overlapped(face, pose, run_face, run_body, device):
    """Face on one HIP stream, guide -> VQ decode -> body on another, from this host thread (bench.py PipelineSubject.overlapped).
    The loops' once-per-call non-finite check waits for its stream, so it is deferred until both streams are loaded and then
    made per stream; a model that escalates to fp32 there (FiLMTransformer.check_finite) has its loop repeated, as the
    non-deferred loops do."""
    (face_s,), (body_s,) = _overlapped_jobs([(face, run_face)], [(pose, run_body)], device)
    return face_s, body_s


def _overlapped_jobs(face_jobs, body_jobs, device):
    """_overlapped for several (model pair, run) jobs per stream: every face job on one side stream, every guide -> body job on the
    other, in list order.  Each distinct denoiser is checked once on its stream after both are loaded, and every job of a denoiser
    that escalated is repeated.  Returns the two lists of results."""
    main = torch.cuda.current_stream(device)
    s_face, s_body = torch.cuda.Stream(device), torch.cuda.Stream(device)
    s_face.wait_stream(main)
    s_body.wait_stream(main)
    diffs = [pair[1] for pair, _ in face_jobs + body_jobs]
    escalated = set()
    for d in diffs:
        d.defer_finite_check = True
    try:
        with torch.cuda.stream(s_face):               # enqueued first: nothing on this stream blocks the host
            face_out = [run() for _, run in face_jobs]
        with torch.cuda.stream(s_body):
            body_out = [run() for _, run in body_jobs]
        for stream, jobs in ((s_face, face_jobs), (s_body, body_jobs)):
            with torch.cuda.stream(stream):
                for m in {id(_denoiser(pair[0])): pair[0] for pair, _ in jobs}.values():
                    if m.a2p_check_finite() == "escalated":
                        escalated.add(id(_denoiser(m)))
    finally:
        for d in diffs:
            d.defer_finite_check = False
    main.wait_stream(s_face)
    main.wait_stream(s_body)
    torch.cuda.synchronize(device)
    for jobs, out in ((face_jobs, face_out), (body_jobs, body_out)):
        for i, (pair, run) in enumerate(jobs):
            if id(_denoiser(pair[0])) in escalated:
                out[i] = run()
    return face_out, body_out


def __getattr__(name):
    """continue_recording and regenerate_segment (sample/inpaint.py), generate_conversation and prepare_conversation
    (sample/conversation.py) are importable from here, next to generate_from_recording."""
    if name in ("continue_recording", "regenerate_segment"):
        from . import inpaint
        return getattr(inpaint, name)
    if name in ("generate_conversation", "prepare_conversation"):
        from . import conversation
        return getattr(conversation, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
