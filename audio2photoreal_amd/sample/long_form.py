"""Face and body motion for recordings longer than the denoisers' 600-frame window: windowed joint sampling.

A recording of `T_total` frames is covered by `W` overlapping windows of `T_w` frames (`plan_windows`).  The R repetitions x W
windows are denoised as one batch of R*W sequences (b = r * W + w) through the ordinary fused step, and after every step one kernel
(csrc/kernels_window.h windowed_step_tail_kernel) reconciles them: for every global frame the covering windows' guided x0
predictions are blended with fixed feather weights, the DDIM / DDPM update is computed once from the blend, and the same bits are
written to every window copy of that frame.  The initial noise and any per-step noise are drawn per GLOBAL frame, so every copy of
a shared frame holds identical bits after every step: the state has no seams and the output is read off the windows.

`prepare_long_recording` is `prepare_recording` over the whole recording (global peak normalisation, one partner-noise draw) plus
the windows of its `y["audio"]`; `generate_from_long_recording` is `generate_from_recording` over windows.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from .. import _lib
from ..diffusion.gaussian_diffusion import GaussianDiffusion
from ..audio import resampled_length
from .generate import _guide_keyframes
from .recording import (BLOCK, MAX_FRAMES, MULTISTEP, SAMPLE_RATE, SAMPLES_PER_FRAME, _channels_last, _check_models, _check_sampler,
                        _denoiser, _face_body_runs, _overlapped, _recording_draws, _unnormalised, prepare_recording)

KEYFRAME_STEP = 30                    # the body model's keyframe step: window starts snap to it


class WindowPlan(NamedTuple):
    starts: List[int]                 # first global frame of every window, ascending
    W: int
    weights: np.ndarray               # fp32 [W, T_w]: the covering windows' weights of every global frame sum to 1
    T_w: int                          # frames per window (T_total when the recording fits one window)
    T_total: int


def plan_windows(T_total: int, T_w: int = MAX_FRAMES, min_overlap: int = 120, align: int = KEYFRAME_STEP) -> WindowPlan:
    """W = ceil((T_total - T_w) / stride) + 1 windows, stride = T_w - min_overlap rounded down to a multiple of `align`, with
    their starts spread evenly over [0, T_total - T_w] in whole `align` units (so every window's keyframe grid is the global
    grid and every overlap is at least `min_overlap`).  T_total <= T_w: one window of T_total frames, weights 1.

    Weights: a linear feather.  Window w's raw weight at local frame i is the distance to its nearer edge, min(i, T_w - 1 - i)
    + 0.5, where an edge at the recording's own start or end counts as infinitely far; the raw weights are normalised over the
    windows covering each global frame in float64 and cast to fp32.  Any number of windows may cover a frame.

    Raises A2PError for min_overlap outside [align, T_w / 2] or T_total not a multiple of align."""
    T_total, T_w, min_overlap, align = int(T_total), int(T_w), int(min_overlap), int(align)
    if align < 1 or T_w < 1 or T_total < 1:
        raise _lib.A2PError(f"bad window geometry: T_total {T_total}, T_w {T_w}, align {align}")
    if not align <= min_overlap <= T_w // 2:
        raise _lib.A2PError(f"min_overlap must lie in [{align}, {T_w // 2}] frames (got {min_overlap})")
    if T_total % align:
        raise _lib.A2PError(f"T_total = {T_total} frames is not a multiple of the keyframe step {align}")
    if T_total <= T_w:
        return WindowPlan([0], 1, np.ones((1, T_total), np.float32), T_total, T_total)
    if T_w % align:
        raise _lib.A2PError(f"the window of {T_w} frames is not a multiple of the keyframe step {align}")
    units = (T_total - T_w) // align                        # the last start, in align units
    stride = (T_w - min_overlap) // align                   # the largest gap between starts, in align units
    W = -(-units // stride) + 1
    if W > _lib.WINDOW_MAX:
        raise _lib.A2PError(f"{W} windows: at most {_lib.WINDOW_MAX}")
    starts = [align * ((2 * w * units + (W - 1)) // (2 * (W - 1))) for w in range(W)]   # round(w * units / (W - 1)) units
    i = np.arange(T_w, dtype=np.float64)
    raw = np.empty((W, T_w), np.float64)
    for w in range(W):
        left = np.full(T_w, np.inf) if w == 0 else i + 0.5
        right = np.full(T_w, np.inf) if w == W - 1 else (T_w - 1 - i) + 0.5
        raw[w] = np.minimum(left, right)
    total = np.zeros(T_total, np.float64)
    for w, s in enumerate(starts):
        total[s:s + T_w] += raw[w]
    weights = np.stack([raw[w] / total[s:s + T_w] for w, s in enumerate(starts)]).astype(np.float32)
    return WindowPlan(starts, W, weights, T_w, T_total)


def check_batch(plan: WindowPlan, num_repetitions: int, max_batch: int) -> None:
    if num_repetitions < 1:
        raise _lib.A2PError(f"num_repetitions must be at least 1 (got {num_repetitions})")
    if num_repetitions * plan.W > max_batch:
        raise _lib.A2PError(f"{num_repetitions} repetitions x {plan.W} windows = {num_repetitions * plan.W} sequences: the models take "
                            f"at most max_batch = {max_batch}; construct them with a larger max_batch or use fewer repetitions")


def _starts_host(plan: WindowPlan):
    return (C.c_int32 * plan.W)(*plan.starts)


def window_gather(src: torch.Tensor, plan: WindowPlan, k: int = 1, channels_first: bool = False) -> torch.Tensor:
    """Windows of a per-frame signal (csrc/kernels_window.h window_gather_kernel).  Channels last: src [R, T_total * k, ch] ->
    [R*W, T_w * k, ch]; channels first (k = 1): src [R, ch, (1,) T_total] -> [R*W, ch, (1,) T_w].  Row r * W + w is the bit-exact
    slice of src[r] from frame starts[w]."""
    _lib.require_gpu_tensor(src, "src")
    if src.dtype != torch.float32:
        raise _lib.A2PError(f"window_gather copies float32 (got {src.dtype})")
    src = src.contiguous()
    R = src.shape[0]
    if channels_first:
        ch = src.shape[1]
        if src.shape[-1] != plan.T_total or src.numel() != R * ch * plan.T_total or k != 1:
            raise _lib.A2PError(f"channels-first windows take [R, ch, (1,) {plan.T_total}] with k = 1 (got {tuple(src.shape)}, k {k})")
        out = torch.empty(R * plan.W, *src.shape[1:-1], plan.T_w, device=src.device, dtype=torch.float32)
    else:
        if src.dim() != 3 or src.shape[1] != plan.T_total * k:
            raise _lib.A2PError(f"channels-last windows take [R, {plan.T_total} * {k}, ch] (got {tuple(src.shape)})")
        ch = src.shape[2]
        out = torch.empty(R * plan.W, plan.T_w * k, ch, device=src.device, dtype=torch.float32)
    with _lib.on_device_of(src):
        _lib.check(_lib.load().a2p_window_gather(_lib.ptr(src), R, plan.T_total, int(k), int(ch), int(bool(channels_first)),
                                                 _starts_host(plan), plan.W, plan.T_w, _lib.ptr(out), _lib.current_stream(src.device)),
                   "a2p_window_gather")
    return out


_SAMPLERS = {"ddim": _lib.SAMPLER_DDIM, "ddpm": _lib.SAMPLER_DDPM}


def windowed_sample_loop(diffusion, model, plan: WindowPlan, R: int, y_windows, noise_global: torch.Tensor, sampler: str = "ddim",
                         eta: float = 0.0, step_noise=None, clip_denoised: bool = False, skip_timesteps: int = 0,
                         progress: bool = False) -> torch.Tensor:
    """`ddim_sample_loop` / `p_sample_loop` over the windows of `plan`, reconciled after every step.

    `model`: a ClassifierFreeSampleModel; `y_windows`: its `y` for the R*W window sequences (b = r * W + w; y["scale"] [R*W]);
    `noise_global` [R, C, 1, T_total]: the initial noise, per global frame; `step_noise` (sequence or callable(step) -> tensor,
    as the loops take it) in the same global layout.  Without `step_noise`, DDPM steps and DDIM steps with eta != 0 draw
    `randn(R, C, 1, T_total)` per step.  The loop is GaussianDiffusion._loop: skip_timesteps, the first-step and end-of-call
    finite checks and the fp32 escalation repeat work as in the plain loops.

    `sampler="dpm++2m"`: DPM-Solver++(2M) over the same steps (a2p_sample_step_windowed_multistep): the update is computed once per
    global frame from the blend, with the history (the previous step's pred_xstart) read from the first covering window like x.
    It is deterministic: eta != 0 or `step_noise` is refused.

    Returns the global [R, C, 1, T_total] result: the final pred_xstart for "ddim" (as ddim_sample_loop), the final sample for
    "ddpm" (as p_sample_loop) and for "dpm++2m" (the last step's pred_xstart bits).  PLMS is refused."""
    multistep = sampler == MULTISTEP
    if sampler not in _SAMPLERS and not multistep:
        raise _lib.A2PError(f"windowed sampling runs 'ddim', 'ddpm' or '{MULTISTEP}' (got {sampler!r}; PLMS is not supported)")
    if multistep:
        GaussianDiffusion.check_multistep_args(2, eta, step_noise)
    need = "a2p_sample_step_windowed_multistep" if multistep else "a2p_sample_step_windowed"
    if not hasattr(model, need):
        raise _lib.A2PError(f"windowed sampling needs this package's ClassifierFreeSampleModel ({need})")
    _lib.require_gpu_tensor(noise_global, "noise_global")
    if noise_global.dim() != 4 or noise_global.shape[0] != R or noise_global.shape[2] != 1 or noise_global.shape[3] != plan.T_total:
        raise _lib.A2PError(f"noise_global must be [{R}, C, 1, {plan.T_total}] (got {tuple(noise_global.shape)})")
    device = noise_global.device
    Cf = noise_global.shape[1]
    starts = _starts_host(plan)
    weights = torch.from_numpy(plan.weights).to(device).contiguous()
    tmap = diffusion._timestep_map(device)
    x_win = window_gather(noise_global.to(torch.float32), plan, channels_first=True)
    if multistep:
        coefs = diffusion._multistep_coefs(device)

        def ms_step(model, img, t, x0_prev, model_kwargs=None):
            x_next, x0, xg, x0g = model.a2p_sample_step_windowed_multistep(img, t.to(torch.int64).contiguous(), tmap, coefs,
                                                                           model_kwargs["y"], x0_prev, clip_denoised, starts, weights,
                                                                           plan.T_total)
            return {"sample": x_next, "pred_xstart": x0, "sample_global": xg, "pred_xstart_global": x0g}

        def run_ms():
            final = None
            for out in diffusion._multistep_loop(ms_step, model, (R * plan.W, Cf, 1, plan.T_w), x_win, {"y": y_windows}, device,
                                                 progress, skip_timesteps, None, False):
                final = out
            return final["sample_global"]
        return diffusion._run_call(run_ms, model, device)
    sid = _SAMPLERS[sampler]
    tables = diffusion._tables(device)

    def step(model, img, t, model_kwargs=None, noise=None, **_):
        if noise is None and (sid == _lib.SAMPLER_DDPM or eta != 0.0):
            noise = torch.randn(R, Cf, 1, plan.T_total, device=device)
        x_next, x0, xg, x0g = model.a2p_sample_step_windowed(sid, img, t.to(torch.int64).contiguous(), tmap, tables, model_kwargs["y"],
                                                             noise, eta, clip_denoised, starts, weights, plan.T_total)
        return {"sample": x_next, "pred_xstart": x0, "sample_global": xg, "pred_xstart_global": x0g}

    def run():
        final = None
        for out in diffusion._loop(step, model, (R * plan.W, Cf, 1, plan.T_w), x_win, {"y": y_windows}, device, progress,
                                   skip_timesteps, None, False, step_noise):
            final = out
        return final["pred_xstart_global" if sid == _lib.SAMPLER_DDIM else "sample_global"]
    return diffusion._run_call(run, model, device)


class LongRecording(NamedTuple):
    audio: torch.Tensor               # y["audio"] of the whole recording: fp32 [R, Lc, 2]
    T: int                            # T_total
    dual_audio: np.ndarray            # the un-normalised dual audio, float64 [2, Lc]
    plan: WindowPlan
    windows: torch.Tensor             # the windows' y["audio"]: fp32 [R*W, T_w * 1600, 2]


def recording_frames(waveform, sr: int) -> int:
    """Frames at 30 fps that `prepare_recording`'s rules keep of a recording (whole 4 s blocks at 48 kHz); host only."""
    if sr <= 0 or int(sr) != sr:
        raise ValueError(f"sr must be a positive integer rate (got {sr})")
    x = _channels_last(waveform)
    Lr = resampled_length(x.shape[0], int(sr), SAMPLE_RATE)
    if Lr < BLOCK:
        raise _lib.A2PError(f"the recording lasts {Lr / SAMPLE_RATE:.2f} s: at least 4 s are needed")
    return (Lr // BLOCK) * BLOCK // SAMPLES_PER_FRAME


def prepare_long_recording(waveform, sr: int, stats: Dict[str, np.ndarray], num_repetitions: int, seed: int = 10, device="cuda",
                           max_batch: Optional[int] = None, T_w: int = MAX_FRAMES, min_overlap: int = 120,
                           align: int = KEYFRAME_STEP) -> LongRecording:
    """`prepare_recording` over a recording of any length: the same resampler, 4 s block rule, dual-audio kernel and partner-noise
    draw over the WHOLE recording (peak normalisation is global), then the windows of `plan_windows(T_total, T_w, min_overlap,
    align)`, each a bit-exact slice of the global y["audio"].  Raises A2PError before any GPU work for a bad plan, for
    num_repetitions x W > `max_batch` (when given), and for what `prepare_recording` refuses other than the length."""
    if num_repetitions < 1:
        raise _lib.A2PError(f"num_repetitions must be at least 1 (got {num_repetitions})")
    T = recording_frames(waveform, sr)
    plan = plan_windows(T, T_w, min_overlap, align)
    if max_batch is not None:
        check_batch(plan, num_repetitions, max_batch)
    prep = prepare_recording(waveform, sr, stats, num_repetitions, seed, device, max_frames=T)
    assert prep.T == T
    windows = window_gather(prep.audio, plan, k=SAMPLES_PER_FRAME)
    return LongRecording(prep.audio, T, prep.dual_audio, plan, windows)


def _max_batch(*modules) -> int:
    return min(int(m.max_batch) for m in modules if m is not None and getattr(m, "max_batch", None) is not None)


def generate_from_long_recording(face, pose, stats: Dict[str, np.ndarray], waveform, sr: int, num_repetitions: int = 1,
                                 top_p: float = 0.97, face_scale: float = 10.0, pose_scale: float = 2.0, seed: int = 10,
                                 min_overlap: int = 120, overlap: bool = True, share_features: bool = True,
                                 chain_keyframes: bool = False, sampler: str = "ddim", pose_guidance: str = "joint",
                                 pose_keyframe_scale: Optional[float] = None) -> Dict[str, object]:
    """`generate_from_recording` for a recording of any length, over the windows of `plan_windows(T_total, seq_len, min_overlap)`.

    Per window (batch R*W): the audio front end / lip features, and guide transformer -> VQ keyframes.  The keyframes of two
    overlapping windows are predicted independently and may disagree on their shared frames; the body model's blend of the
    windows' x0 predictions absorbs that (the body follows a weighted mean of the two windows' keyframe-conditioned predictions).
    The face and body loops are `windowed_sample_loop` with `sampler` ("ddim" or "dpm++2m", over the steps the diffusions were
    built with), on two HIP streams when `overlap`.

    `chain_keyframes=True` makes the overlapping keyframes agree instead: the guide runs window by window, and window w > 0 forces
    its keyframes inside window w - 1 to window w - 1's VQ tokens and takes window w - 1's keyframe rows there verbatim (window
    starts are on the 30-frame grid, so the two windows' keyframes fall on the same frames).  Its draws after the overlap follow on
    from those keyframes.  Each free position draws the uniform it draws without chaining, so window 0 is unchanged.  This runs W
    guide launches of R sequences instead of one launch of R * W.

    Random draws: the initial noise is `per_sample_noise((R, C, 1, T_total), [derive_seed(seed, 3 or 2, r)])`, as
    `generate_from_recording` draws it for T frames; the keyframe uniforms of window 0 come from `derive_seed(seed, 1, r)`, as
    there, those of window w > 0 from `derive_seed(seed, 1, r, w)`.  A recording that fits one window gives exactly
    `generate_from_recording`'s result.

    `pose_guidance` / `pose_keyframe_scale`: how the body model is guided, as generate_from_recording takes them ("joint", "audio"
    or "dual" with a keyframe scale; "dual" runs 1.5x the sequences and needs the pose model's max_batch >= ceil(1.5 x batch)).

    Returns {"face": [R, T_total, 256], "pose": [R, T_total, 104], "keyframes": [R, W, T_w / 30, 104] (un-normalised),
    "audio": float64 [2, Lc], "T": T_total, "sr": 48000, "window_starts": [W] ints}."""
    face_m, face_d = face
    pose_m, pose_d = pose
    fm, pm = _denoiser(face_m), _denoiser(pose_m)
    _check_sampler(sampler)
    _check_models(fm, pm)
    from .generate import pose_guidance_plan
    pose_scale = pose_guidance_plan(pose_scale, pose_guidance, pose_keyframe_scale)
    device = fm.null_cond_embed.device
    R = int(num_repetitions)
    max_batch = _max_batch(fm, pm, pm.transformer, fm.audio_frontend, pm.audio_frontend)
    rec = prepare_long_recording(waveform, sr, stats, R, seed, device, max_batch=max_batch, T_w=min(fm.seq_len, pm.seq_len),
                                 min_overlap=min_overlap)
    plan, T, audio = rec.plan, rec.T, rec.windows
    W = plan.W
    nk = len(range(plan.T_w)[::KEYFRAME_STEP])
    uniforms, noise_pose, noise_face = _recording_draws(seed, R, nk * pm.tokenizer.residual_depth, (pm.nfeats, fm.nfeats), T, W)

    with torch.no_grad():
        run_face, run_body, y_body = _face_body_runs(face, pose, audio, plan.T_w, nk, uniforms, noise_face.to(device),
                                                     noise_pose.to(device), top_p, face_scale, pose_scale, sampler, share_features,
                                                     plan=plan, chain_keyframes=chain_keyframes)
        if overlap:
            face_s, body_s = _overlapped(face, pose, run_face, run_body, device)
        else:
            face_s = run_face()
            body_s = run_body()
    kf = y_body["keyframes"].cpu().numpy().reshape(R, W, nk, pm.nfeats)
    return {**_unnormalised(face_s, body_s, kf, stats),
            "audio": rec.dual_audio, "T": T, "sr": SAMPLE_RATE, "window_starts": list(plan.starts)}


def _chained_keyframes(pose_m, plan: WindowPlan, R: int, guide_cond, uniforms: torch.Tensor, top_p: float, nk: int,
                       nv: int) -> torch.Tensor:
    """generate_from_long_recording(chain_keyframes=True): one guide launch of R sequences per window, in window order.  Window
    w > 0 forces its first keyframes (those inside window w - 1) to window w - 1's tokens and takes window w - 1's decoded rows
    there.  Returns keyframes [R * W, nk, nv] on the host (row r * W + w)."""
    W = plan.W
    depth = pose_m.tokenizer.residual_depth
    kf = torch.empty(R, W, nk, nv)
    prev_tokens = None
    for w in range(W):
        cond = {k: v[w::W] for k, v in guide_cond.items()}          # rows r * W + w
        y = {**cond, "keyframes": torch.zeros(R, nk, nv)}
        forced, n_ov, off = None, 0, 0
        if w > 0:
            off = (plan.starts[w] - plan.starts[w - 1]) // KEYFRAME_STEP
            n_ov = nk - off                                            # keyframes of window w that window w - 1 also has
            forced = torch.full((R, nk, depth), -1, dtype=torch.int64, device=prev_tokens.device)
            forced[:, :n_ov] = prev_tokens[:, off:]
            forced = forced.reshape(R, -1)
        pred, prev_tokens = _guide_keyframes({"y": y}, pose_m, uniforms[:, w::W], top_p, forced)
        if w > 0:
            pred[:, :n_ov] = kf[:, w - 1, off:]
        kf[:, w] = pred
    return kf.reshape(R * W, nk, nv)
