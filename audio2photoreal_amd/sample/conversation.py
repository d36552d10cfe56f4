"""Both people of a two-channel conversation recording: the dataset's audio convention at the recording-level API.

The models were trained on two-channel audio, channel 0 the person's own microphone and channel 1 the conversation partner's
(data_loaders/get_data.py:79-92, z-normalised as in data_loaders/data.py:237); the partner's motion swaps the two channels
(flip_person, get_data.py:83-88).  The demo records one microphone and puts noise in the partner channel, and so do
`prepare_recording` / `generate_from_recording`.  Here a stereo recording (channel k = person k's microphone) gives each person
its own voice in channel 0 and the other's in channel 1 (csrc/kernels_audio.h conversation_audio_kernel), and
`generate_conversation` animates one or both of them with the face + body pipeline of `generate_from_recording` (recordings that
fit one window) or `generate_from_long_recording` (longer ones).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, NamedTuple, Optional

import numpy as np
import torch

from .. import _lib
from ..audio import _device_table, resampled_length, sinc_resample_table
from ..sample_parallel import derive_seed
from .long_form import KEYFRAME_STEP, WindowPlan, _max_batch, plan_windows, window_gather
from .recording import (BLOCK, MAX_FRAMES, SAMPLE_RATE, SAMPLES_PER_FRAME, _audio_stats, _check_models, _check_sampler, _denoiser,
                        _face_body_runs, _overlapped_jobs, _recording_draws, _unnormalised)

NORMALIZE = ("peak", "none")
_PERSON_SEED = 11                     # derive_seed stream id of the per-person base seeds (1-10: recording.py, inpaint.py)


class PreparedConversation(NamedTuple):
    audio: List[Optional[torch.Tensor]]       # person p's y["audio"]: fp32 [R, Lc, 2] (own, partner) on the GPU; None: not animated
    T: int                                    # frames at 30 fps = Lc / 1600
    dual_audio: List[Optional[np.ndarray]]    # person p's un-normalised dual audio, float64 [2, Lc] (own, partner)
    plan: Optional[WindowPlan]                # T > max_frames: the windows (plan_windows), else None
    windows: List[Optional[torch.Tensor]]     # with a plan: person p's windows of y["audio"], fp32 [R*W, T_w * 1600, 2]


def _two_channels(waveform) -> torch.Tensor:
    """float32 [L, 2] on the host from [2, L] / [L, 2] (numpy or torch, e.g. read_wav's stereo output) or a pair (a, b) of mono
    tracks.  ValueError for anything else."""
    def host(t):
        t = t.detach().cpu() if torch.is_tensor(t) else torch.from_numpy(np.ascontiguousarray(np.asarray(t)))
        return t.to(torch.float32)
    if isinstance(waveform, (tuple, list)):
        if len(waveform) != 2:
            raise ValueError(f"a conversation is one stereo recording or a pair of mono tracks (got {len(waveform)} tracks)")
        a, b = host(waveform[0]), host(waveform[1])
        if a.dim() != 1 or b.dim() != 1:
            raise ValueError(f"the two tracks must be mono [L] (got shapes {tuple(a.shape)} and {tuple(b.shape)})")
        if a.shape != b.shape:
            raise ValueError(f"the two tracks must have the same length (got {a.shape[0]} and {b.shape[0]} samples)")
        return torch.stack([a, b], dim=1)
    t = host(waveform)
    if t.dim() == 2 and t.shape[0] == 2:
        return t.t().contiguous()
    if t.dim() == 2 and t.shape[1] == 2:
        return t.contiguous()
    raise ValueError(f"a conversation recording has exactly 2 channels, [2, L] or [L, 2] (got shape {tuple(t.shape)}); a mono "
                     "recording takes generate_from_recording")


def _conversation_frames(x: torch.Tensor, sr) -> int:
    if sr <= 0 or int(sr) != sr:
        raise ValueError(f"sr must be a positive integer rate (got {sr})")
    Lr = resampled_length(x.shape[0], int(sr), SAMPLE_RATE)
    if Lr < BLOCK:
        raise _lib.A2PError(f"the recording lasts {Lr / SAMPLE_RATE:.2f} s: at least 4 s are needed")
    return (Lr // BLOCK) * BLOCK // SAMPLES_PER_FRAME


def _check_normalize(normalize) -> None:
    if normalize not in NORMALIZE:
        raise _lib.A2PError(f"normalize must be one of {NORMALIZE} (got {normalize!r})")


def _people_flags(people) -> List[bool]:
    flags = [bool(p) for p in people]
    if len(flags) != 2 or not any(flags):
        raise _lib.A2PError(f"people must be a pair with at least one person animated (got {people!r})")
    return flags


def person_seeds(seed):
    """(s0, s1): the base seeds of persons 0 and 1.  A pair is taken as it is; an int gives derive_seed(seed, 11, p)."""
    if isinstance(seed, (tuple, list)):
        if len(seed) != 2:
            raise _lib.A2PError(f"seed must be an int or a pair (s0, s1) (got {seed!r})")
        return int(seed[0]), int(seed[1])
    return derive_seed(int(seed), _PERSON_SEED, 0), derive_seed(int(seed), _PERSON_SEED, 1)


def prepare_conversation(waveform, sr: int, stats, num_repetitions: int, normalize: str = "peak", people=(True, True), device="cuda",
                         max_frames: Optional[int] = None, min_overlap: int = 120, max_batch: Optional[int] = None) -> PreparedConversation:
    """Each person's y["audio"] from a two-channel recording: every channel resampled to 48 kHz on its own
    (a2p_resample_channels), whole 4 s blocks kept (`prepare_recording`'s rule), then for person p (channel p its own voice,
    channel 1 - p the partner's) the dual audio (own, partner), z-normalised with `stats[p]` and tiled over the repetitions
    (a2p_conversation_audio).

    `normalize="peak"`: each channel divided by its own maximum (float32; the demo's y / max(y), applied to each voice); a silent
    or non-finite channel raises A2PError.  `"none"`: the samples as given, the dataset's rule for floats in [-1, 1]
    (integer PCM from read_wav: divide by the full scale first, e.g. 32768 for 16 bits).

    `stats`: a pair of stats dicts (audio_mean of 1 or 2 values, audio_std_flat), one per person (None for a person not
    animated); `people`: which persons to prepare.  `max_frames`: the window (default 600 frames); a longer recording also gets
    the windows of `plan_windows(T, max_frames, min_overlap)` (`prepare_long_recording`), and `max_batch`, when given, bounds
    the animated persons x repetitions x windows.  Raises A2PError / ValueError before any GPU work."""
    if num_repetitions < 1:
        raise _lib.A2PError(f"num_repetitions must be at least 1 (got {num_repetitions})")
    R = int(num_repetitions)
    _check_normalize(normalize)
    flags = _people_flags(people)
    x = _two_channels(waveform)
    T = _conversation_frames(x, sr)
    sr = int(sr)
    if not isinstance(stats, (tuple, list)) or len(stats) != 2:
        raise _lib.A2PError("stats must be a pair of stats dicts, one per person")
    st = np.zeros((2, 3), np.float64)
    for p in range(2):
        if flags[p]:
            if stats[p] is None:
                raise _lib.A2PError(f"person {p} is animated but has no stats")
            st[p] = _audio_stats(stats[p])
    T_w = MAX_FRAMES if max_frames is None else int(max_frames)
    plan = plan_windows(T, T_w, min_overlap) if T > T_w else None
    n_people = sum(flags)
    if max_batch is not None and n_people * R * (plan.W if plan else 1) > max_batch:
        raise _lib.A2PError(f"{n_people} people x {R} repetitions x {plan.W if plan else 1} windows: the models take at most "
                            f"max_batch = {max_batch} sequences")
    if sr != SAMPLE_RATE:
        sinc_resample_table(sr, SAMPLE_RATE)          # size check of the filter table on the host (A2PError) before any upload
    device = torch.device(device)
    if device.type != "cuda":
        raise _lib.A2PError(f"prepare_conversation runs on the MI355X (got device {device}); there is no CPU implementation")

    L = x.shape[0]
    Lr = resampled_length(L, sr, SAMPLE_RATE)
    Lc = T * SAMPLES_PER_FRAME
    xd = x.to(device).contiguous()
    chans = torch.empty(2, Lr, device=device, dtype=torch.float32)
    table, width, n_phase, n_taps = None, 0, 0, 0
    if sr != SAMPLE_RATE:
        table, width = _device_table(sr, SAMPLE_RATE, 6, 0.99, "sinc_interp_hann", None, torch.float32, device)
        n_phase, n_taps = table.shape
    out = torch.empty(2 * R, Lc, 2, device=device, dtype=torch.float32)
    scratch = torch.empty(_lib.CONVERSATION_SCRATCH, device=device, dtype=torch.float32)
    mode = _lib.NORMALIZE_PEAK if normalize == "peak" else _lib.NORMALIZE_NONE
    mask = int(flags[0]) | int(flags[1]) << 1
    stats_host = (C.c_double * 6)(*st.reshape(-1).tolist())
    lib = _lib.load()
    with _lib.on_device_of(xd):
        stream = _lib.current_stream(device)
        _lib.check(lib.a2p_resample_channels(_lib.ptr(xd), L, 2, sr, SAMPLE_RATE, _lib.ptr(table), n_phase, n_taps, width, _lib.ptr(chans),
                                             stream), "a2p_resample_channels")
        _lib.check(lib.a2p_conversation_audio(_lib.ptr(chans), Lr, Lc, mode, _lib.ptr(scratch), mask, stats_host, R, _lib.ptr(out), stream),
                   "a2p_conversation_audio")
    # each person's float64 dual audio on the host, un-normalised again as prepare_recording does (before the float32 cast)
    u = chans[:, :Lc].cpu().numpy()
    if normalize == "peak":
        u = u / u.max(axis=1, keepdims=True)
    audio, dual, windows = [None, None], [None, None], [None, None]
    for p in range(2):
        if not flags[p]:
            continue
        audio[p] = out[p * R:(p + 1) * R]
        d = np.stack([u[p], u[1 - p]], axis=-1)[None].astype(np.float64)
        d = (d - stats[p]["audio_mean"]) / stats[p]["audio_std_flat"]
        d = d * stats[p]["audio_std_flat"] + stats[p]["audio_mean"]
        dual[p] = np.ascontiguousarray(d[0].T)
        if plan is not None:
            windows[p] = window_gather(audio[p], plan, k=SAMPLES_PER_FRAME)
    return PreparedConversation(audio, T, dual, plan, windows)


def _same_stats(a, b) -> bool:
    if a is b:
        return True
    if a.keys() != b.keys():
        return False
    return all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def generate_conversation(people, waveform, sr: int, num_repetitions: int = 1, top_p: float = 0.97, face_scale: float = 10.0,
                          pose_scale: float = 2.0, seed=10, normalize: str = "peak", sampler: str = "ddim", min_overlap: int = 120,
                          overlap: bool = True, share_features: bool = True, chain_keyframes: bool = False,
                          pose_guidance: str = "joint", pose_keyframe_scale: Optional[float] = None) -> Dict[str, object]:
    """Face and body motion of the people of a two-channel conversation recording (channel k: person k's microphone).

    `people`: a pair of (face, pose, stats) triples as `generate_from_recording` takes them; an entry may be None, a partner who is
    heard but not animated (an avatar listening to a live user).  Person p hears its own channel as channel 0 and the other's
    as channel 1 (`prepare_conversation`, `normalize` "peak" or "none").  A recording that fits the models' window takes
    `generate_from_recording`'s path, a longer one `generate_from_long_recording`'s (the same plan, `min_overlap` and
    `chain_keyframes`); `sampler` is "ddim" or "dpm++2m".

    Batching: when both people use the same model objects and equal stats they are sampled as one batch of 2R sequences (2R*W
    windowed), person-major; otherwise each person's loops run with its own models.  `overlap=True` puts every face loop on one
    HIP stream and every guide -> body chain on another.  Neither choice changes the result beyond the batch-size dependence of
    the kernels (none at fp32 shapes that take the same kernels).

    Random draws: person p draws from a base seed s_p, `seed=(s0, s1)` or, for an int seed, derive_seed(seed, 11, p)
    (`person_seeds`); from s_p on they are the keyframe uniforms, face noise and body noise that generate_from_recording /
    generate_from_long_recording draw with seed=s_p.

    `pose_guidance` / `pose_keyframe_scale`: how the body model is guided, as generate_from_recording takes them ("joint", "audio"
    or "dual" with a keyframe scale; "dual" runs 1.5x the sequences and needs the pose model's max_batch >= ceil(1.5 x batch)).

    Returns {"people": [dict or None, dict or None], "T", "sr": 48000} (plus "window_starts" for long recordings); each person's
    dict has the keys and shapes of generate_from_recording's (or generate_from_long_recording's) result, un-normalised with that
    person's stats, its "audio" being (own, partner).  Bad input raises A2PError / ValueError before any GPU work."""
    if not isinstance(people, (tuple, list)) or len(people) != 2:
        raise _lib.A2PError("people must be a pair of (face, pose, stats) triples or None")
    flags = _people_flags([p is not None for p in people])
    for p in range(2):
        if flags[p] and (not isinstance(people[p], (tuple, list)) or len(people[p]) != 3):
            raise _lib.A2PError(f"people[{p}] must be a (face, pose, stats) triple or None")
    _check_sampler(sampler)
    _check_normalize(normalize)
    from .generate import pose_guidance_plan
    pose_scale = pose_guidance_plan(pose_scale, pose_guidance, pose_keyframe_scale)
    R = int(num_repetitions)
    if R < 1:
        raise _lib.A2PError(f"num_repetitions must be at least 1 (got {num_repetitions})")
    animated = [p for p in range(2) if flags[p]]
    for p in animated:
        face, pose, _ = people[p]
        _check_models(_denoiser(face[0]), _denoiser(pose[0]))
    seeds = person_seeds(seed)
    x = _two_channels(waveform)
    T = _conversation_frames(x, sr)
    fms = {p: _denoiser(people[p][0][0]) for p in animated}
    pms = {p: _denoiser(people[p][1][0]) for p in animated}
    devices = {str(fms[p].null_cond_embed.device) for p in animated} | {str(pms[p].null_cond_embed.device) for p in animated}
    if len(devices) != 1:
        raise _lib.A2PError(f"the models of a conversation live on one device (got {sorted(devices)})")
    device = fms[animated[0]].null_cond_embed.device
    T_w = min(min(fms[p].seq_len, pms[p].seq_len) for p in animated)
    long = T > T_w
    W = plan_windows(T, T_w, min_overlap).W if long else 1

    # groups of persons sampled in one batch: both people when they share the model objects and the stats
    batched = (len(animated) == 2 and people[0][0][0] is people[1][0][0] and people[0][0][1] is people[1][0][1]
               and people[0][1][0] is people[1][1][0] and people[0][1][1] is people[1][1][1] and _same_stats(people[0][2], people[1][2]))
    groups = [animated] if batched else [[p] for p in animated]
    for g in groups:
        fm, pm = fms[g[0]], pms[g[0]]
        cap = _max_batch(fm, pm, pm.transformer, fm.audio_frontend, pm.audio_frontend)
        if len(g) * R * W > cap:
            raise _lib.A2PError(f"{len(g)} people x {R} repetitions x {W} windows = {len(g) * R * W} sequences: the models take at most "
                                f"max_batch = {cap}; construct them with a larger max_batch or use fewer repetitions")

    prep = prepare_conversation(x, sr, [people[p][2] if flags[p] else None for p in range(2)], R, normalize, flags, device,
                                max_frames=T_w, min_overlap=min_overlap)
    plan = prep.plan
    T_run = plan.T_w if long else T
    nk = len(range(T_run)[::KEYFRAME_STEP])

    runs = []
    with torch.no_grad():
        for g in groups:
            face, pose, _ = people[g[0]]
            fm, pm = fms[g[0]], pms[g[0]]
            draws = [_recording_draws(seeds[p], R, nk * pm.tokenizer.residual_depth, (pm.nfeats, fm.nfeats), T, W) for p in g]
            uniforms = torch.cat([d[0] for d in draws], dim=1)
            noise_pose = torch.cat([d[1] for d in draws], dim=0)
            noise_face = torch.cat([d[2] for d in draws], dim=0)
            rows = [prep.windows[p] if long else prep.audio[p] for p in g]
            audio = rows[0] if len(rows) == 1 else torch.cat(rows, dim=0)
            run_face, run_body, y_body = _face_body_runs(face, pose, audio, T_run, nk, uniforms, noise_face.to(device),
                                                         noise_pose.to(device), top_p, face_scale, pose_scale, sampler, share_features,
                                                         plan=plan, chain_keyframes=chain_keyframes)
            runs.append((g, face, pose, run_face, run_body, y_body))
        if overlap:
            face_out, body_out = _overlapped_jobs([(r[1], r[3]) for r in runs], [(r[2], r[4]) for r in runs], device)
        else:
            face_out, body_out = [], []
            for _, _, _, run_face, run_body, _ in runs:
                face_out.append(run_face())
                body_out.append(run_body())

    result = [None, None]
    for (g, _, _, _, _, y_body), face_s, body_s in zip(runs, face_out, body_out):
        kf = y_body["keyframes"].cpu().numpy()
        for k, p in enumerate(g):
            rows = slice(k * R, (k + 1) * R)
            kf_p = kf[k * R * W:(k + 1) * R * W]
            if long:
                kf_p = kf_p.reshape(R, W, nk, -1)
            res = {**_unnormalised(face_s[rows], body_s[rows], kf_p, people[p][2]), "audio": prep.dual_audio[p], "T": T,
                   "sr": SAMPLE_RATE}
            if long:
                res["window_starts"] = list(plan.starts)
            result[p] = res
    out = {"people": result, "T": T, "sr": SAMPLE_RATE}
    if long:
        out["window_starts"] = list(plan.starts)
    return out
