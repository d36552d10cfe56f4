"""Test-split batches on the MI355X: the takes of a split are uploaded once in their stored dtypes and stay resident; one
`a2p_dataset_batch` launch (csrc/kernels_dataset.h) then builds what the reference's `Social.__getitem__` + `social_collate`
build for a set of chunks -- ground truth, keyframes, missing mask, z-normalised audio -- in the layouts the models take.

The outputs carry the reference's bits under its own conditions: pose / code statistics float64 and audio statistics float32
(as every released data_stats.pth stores them), poses float32 or float64, audio float32.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Sequence

import numpy as np
import torch

from .. import _lib
from .._lib import A2PError
from .capture import AUDIO_PER_FRAME, Take, chunk_plan

_STATS = {"pose": ("pose_mean", "pose_std"), "face": ("code_mean", "code_std")}


def check_stats(stats, data_format: str):
    """(mean float64 [C], std float64 [C], audio mean float32 [2], audio std float32) of a data_stats dict, or A2PError."""
    if data_format not in _STATS:
        raise A2PError(f"data_format must be 'pose' or 'face' (got {data_format!r})")
    keys = _STATS[data_format] + ("audio_mean", "audio_std_flat")
    absent = [k for k in keys if k not in stats]
    if absent:
        raise A2PError(f"the statistics lack {absent}")
    mean = np.ascontiguousarray(np.asarray(stats[keys[0]], np.float64).reshape(-1))
    std = np.ascontiguousarray(np.asarray(stats[keys[1]], np.float64).reshape(-1))
    amean = np.asarray(stats["audio_mean"], np.float32).reshape(-1)
    astd = np.asarray(stats["audio_std_flat"], np.float32).reshape(-1)
    if mean.shape != std.shape or amean.size != 2 or astd.size != 1:
        raise A2PError(f"statistics of unexpected shape: {keys[0]} {mean.shape}, {keys[1]} {std.shape}, audio_mean {amean.shape}, "
                       f"audio_std_flat {astd.shape}")
    return mean, std, amean, astd


class CaptureBatches:
    """The chunks of a split (`capture.test_split(load_capture(...))`) as device batches.

    `len()` is the number of T-frame chunks of `capture.chunk_plan([take lengths], T, seed)`; `plan[i]` is chunk i's (take,
    start).  `batch(indices)` returns `(gt, {"y": {...}})` on the device with the reference's collate layout:

        gt          fp32 [B, C, 1, T]     z-normalised motion (face: zero on the frames without a code)
        keyframes   fp32 [B, ceil(T / step), C]   gt at every `step`-th frame: step 30 for pose, 1 for face
        missing     fp32 [B, T, C]        0 on the frames without a face code (pose: ones)
        audio       fp32 [B, T * 1600, 2] z-normalised with audio_mean / audio_std_flat
        mask        bool [B, 1, 1, T] all true; lengths / alengths / klengths int64 [B] = T, T * 1600, ceil(T / step)

    `swap_channels` exchanges the audio channels in the kernel (takes loaded with `flip_person` are already swapped).
    Every check of the constructor's arguments happens on the host, before the HIP library is loaded or anything is uploaded."""

    def __init__(self, takes: Sequence[Take], stats: Dict[str, np.ndarray], data_format: str, T: int = 600, seed=10,
                 device="cuda", swap_channels: bool = False, audio_per_frame: int = AUDIO_PER_FRAME):
        self.mean_h, self.std_h, self.amean, self.astd = check_stats(stats, data_format)
        if isinstance(T, bool) or not isinstance(T, (int, np.integer)) or T < 1:
            raise A2PError(f"T must be a positive integer (got {T!r})")
        if audio_per_frame < 2 or audio_per_frame % 2:
            raise A2PError(f"audio_per_frame must be even (got {audio_per_frame})")
        if not len(takes):
            raise A2PError("the split holds no take")
        self.data_format, self.T, self.seed, self.face = data_format, int(T), seed, data_format == "face"
        self.step = 1 if self.face else 30                       # Social._register_keyframe_step
        self.K = len(range(0, self.T, self.step))
        self.audio_per_frame, self.swap_channels = int(audio_per_frame), bool(swap_channels)
        self.C = int(self.mean_h.shape[0])
        for k, t in enumerate(takes):
            m = t.face if self.face else t.pose
            if m.ndim != 2 or m.shape[1] != self.C:
                raise A2PError(f"take {k} ({t.name}): {data_format} data {m.shape} does not match the statistics' {self.C} channels")
            if m.dtype not in (np.float32, np.float64):
                raise A2PError(f"take {k} ({t.name}): {data_format} data must be float32 or float64 (got {m.dtype})")
            if t.audio.dtype != np.float32 or t.audio.shape != (len(m) * self.audio_per_frame, 2):
                raise A2PError(f"take {k} ({t.name}): audio {t.audio.dtype} {t.audio.shape} must be float32 "
                               f"[{len(m) * self.audio_per_frame}, 2]")
            if len(t.present) != len(m):
                raise A2PError(f"take {k} ({t.name}): {len(t.present)} presence flags for {len(m)} frames")
        self.plan = chunk_plan([t.frames for t in takes], self.T, seed)
        if not len(self.plan):
            raise A2PError(f"the split is empty: none of its {len(takes)} take(s) is longer than T = {self.T} frames "
                           f"(lengths {[t.frames for t in takes]})")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise A2PError(f"CaptureBatches runs on the MI355X (got device {self.device}); there is no CPU implementation")
        from ..sample.generate import make_inv_transform
        self.inv_transform = make_inv_transform(stats)
        # ---- upload, once
        self._lib = _lib.load()
        dev = self.device
        self._motion = [torch.from_numpy(np.ascontiguousarray(t.face if self.face else t.pose)).to(dev) for t in takes]
        self._present = [torch.from_numpy(np.ascontiguousarray(t.present, np.uint8)).to(dev) for t in takes] if self.face else None
        self._audio = [torch.from_numpy(np.ascontiguousarray(t.audio)).to(dev) for t in takes]
        self._mean, self._std = torch.from_numpy(self.mean_h).to(dev), torch.from_numpy(self.std_h).to(dev)
        self._takes = (_lib.A2PDatasetTake * len(takes))()
        for k, t in enumerate(takes):
            self._takes[k].motion = self._motion[k].data_ptr()
            self._takes[k].present = self._present[k].data_ptr() if self.face else None
            self._takes[k].audio = self._audio[k].data_ptr()
            self._takes[k].frames = t.frames
            self._takes[k].motion_f64 = int(self._motion[k].dtype == torch.float64)
        self.resident_bytes = sum(x.numel() * x.element_size() for x in self._motion + self._audio + (self._present or []))

    def __len__(self) -> int:
        return len(self.plan)

    def batch(self, indices: Sequence[int]):
        idx = [int(i) for i in indices]
        B = len(idx)
        if not 1 <= B <= _lib.DATASET_MAX_BATCH:
            raise A2PError(f"a batch holds 1 to {_lib.DATASET_MAX_BATCH} chunks (got {B})")
        if any(not 0 <= i < len(self.plan) for i in idx):
            raise A2PError(f"chunk index outside [0, {len(self.plan)}): {idx}")
        dev, T, Cn = self.device, self.T, self.C
        f32 = dict(dtype=torch.float32, device=dev)
        inp = torch.empty(B, Cn, 1, T, **f32)
        kf = torch.empty(B, self.K, Cn, **f32)
        miss = torch.empty(B, T, Cn, **f32)
        audio = torch.empty(B, T * self.audio_per_frame, 2, **f32)
        self.launch(idx, inp, kf, miss, audio)
        i64 = dict(dtype=torch.int64, device=dev)
        y = {"missing": miss, "mask": torch.ones(B, 1, 1, T, dtype=torch.bool, device=dev),
             "lengths": torch.full((B,), T, **i64), "audio": audio, "alengths": torch.full((B,), T * self.audio_per_frame, **i64),
             "keyframes": kf, "klengths": torch.full((B,), self.K, **i64)}
        return inp, {"y": y}

    def launch(self, idx: Sequence[int], inp, kf, miss, audio) -> None:
        """The one `a2p_dataset_batch` launch of `batch`, into caller-owned fp32 outputs of its shapes, on the current stream."""
        B = len(idx)
        take_of = (C.c_int32 * B)(*[int(self.plan[i, 0]) for i in idx])
        start_of = (C.c_int64 * B)(*[int(self.plan[i, 1]) for i in idx])
        dev = self.device
        with torch.cuda.device(dev):
            _lib.check(self._lib.a2p_dataset_batch(self._takes, len(self._takes), self.C, int(self.face), take_of, start_of, B, self.T,
                                                   self.step, self.audio_per_frame, _lib.ptr(self._mean), _lib.ptr(self._std),
                                                   float(self.amean[0]), float(self.amean[1]), float(self.astd[0]),
                                                   int(self.swap_channels), _lib.ptr(inp), _lib.ptr(kf), _lib.ptr(miss), _lib.ptr(audio),
                                                   _lib.current_stream(dev)), "a2p_dataset_batch")
