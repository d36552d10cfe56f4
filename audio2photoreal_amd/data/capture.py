"""A person's capture directory on the host: takes, splits and the test split's chunk plan (reference
data_loaders/get_data.py:47-129, data_loaders/data.py:52-54 and :112-144), without torchaudio, DataLoader workers or the
reference's `np.take` over ragged lists (which numpy 2 rejects): takes of different lengths load and are planned.

A capture directory holds, per take, `<name>_body_pose.npy` [L, 104], `<name>_face_expression.npy` [L, 256],
`<name>_missing_face_frames.npy` (frame indices without a face code) and `<name>_audio.wav` (48 kHz, two channels: this
person and the partner, 1600 samples per frame), next to the subject's `data_stats.pth`.

Nothing here touches the GPU or loads the HIP library: every error of a bad directory is an A2PError raised on the host.
"""
from __future__ import annotations

import os
import struct
import wave
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from .._lib import A2PError
from ..audio import read_wav

AUDIO_PER_FRAME = 1600                                  # 48 kHz / 30 fps
UNWRAPPED_SUBJECTS = ("PXB184", "RLW104")               # captures 1 and 2: pose channel 3 is unwrapped (get_data.py:74-76)
PARTNERS = (("PXB184", "RLW104"), ("RLW104", "PXB184"), ("TXB805", "GQS883"), ("GQS883", "TXB805"))   # get_data.py:113-121
_POSE, _FACE, _MISSING, _AUDIO = "_body_pose.npy", "_face_expression.npy", "_missing_face_frames.npy", "_audio.wav"


class Take(NamedTuple):
    name: str                   # path of the take without its suffix
    pose: np.ndarray            # [L, 104] in the stored dtype
    face: np.ndarray            # [L, 256] float64
    present: np.ndarray         # uint8 [L]: 0 on the missing face frames, 1 elsewhere
    audio: np.ndarray           # float32 [L * 1600, 2], torchaudio.load's scale; channels swapped when flip_person

    @property
    def frames(self) -> int:
        return len(self.pose)

    def missing(self) -> np.ndarray:
        """The reference's `missing` array: ones like the face codes with zero rows on the listed frames (get_data.py:69-70)."""
        m = np.ones_like(self.face)
        m[self.present == 0] = 0.0
        return m


# ------------------------------------------------------------------------------------------------ WAV, torchaudio.load's scale
def _riff_chunks(path: str):
    """(fmt chunk, data chunk) bytes of a RIFF/WAVE file."""
    with open(path, "rb") as f:
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"WAVE":
            raise A2PError(f"{path}: not a RIFF/WAVE file")
        fmt = data = None
        while True:
            h = f.read(8)
            if len(h) < 8:
                break
            cid, size = h[:4], struct.unpack("<I", h[4:])[0]
            if cid == b"fmt ":
                fmt = f.read(size)
            elif cid == b"data":
                data = f.read(size)
            else:
                f.seek(size, 1)
            if size & 1:
                f.seek(1, 1)                              # chunks are word aligned
            if fmt is not None and data is not None:
                break
    if fmt is None or data is None or len(fmt) < 16:
        raise A2PError(f"{path}: no fmt / data chunk")
    return fmt, data


def _read_float_wav(path: str) -> Tuple[np.ndarray, int]:
    """IEEE-float WAV (format tag 3, or WAVE_FORMAT_EXTENSIBLE with the float sub-format), which the `wave` module refuses:
    (float32 [L, C], rate).  The samples are taken as stored, as torchaudio.load does."""
    fmt, data = _riff_chunks(path)
    tag, C, sr, _, _, bits = struct.unpack("<HHIIHH", fmt[:16])
    if tag == 0xFFFE and len(fmt) >= 26:
        tag = struct.unpack("<H", fmt[24:26])[0]
    if tag != 3 or bits not in (32, 64) or C < 1:
        raise A2PError(f"{path}: WAV format tag {tag} with {bits}-bit samples is not supported (8/16/24/32-bit PCM, 32/64-bit float)")
    width = bits // 8
    n = len(data) // (width * C)
    v = np.frombuffer(data[: n * width * C], "<f4" if bits == 32 else "<f8")
    return v.astype(np.float32).reshape(n, C), sr


def load_wav_normalized(path: str) -> Tuple[np.ndarray, int]:
    """`torchaudio.load(path)` transposed: (float32 [L, C], rate).  Integer PCM is divided by 2^(bits - 1) (8-bit: (v - 128) / 128);
    float WAV is read as stored.  PCM goes through `audio.read_wav`, which returns the stored integers."""
    try:
        with wave.open(path, "rb") as w:
            width = w.getsampwidth()
    except wave.Error:
        return _read_float_wav(path)
    except (OSError, EOFError) as e:
        raise A2PError(f"{path}: cannot read the WAV file ({e})") from None
    try:
        v, sr = read_wav(path)
    except ValueError as e:
        raise A2PError(str(e)) from None
    v = v.reshape(len(v), -1)
    if width == 1:
        v = v - np.float32(128.0)
    return v * np.float32(1.0 / (1 << (8 * width - 1))), sr


# ------------------------------------------------------------------------------------------------ takes
def partner_root(data_root: str) -> str:
    """The directory `flip_person` reads (get_data.py:113-121): the first subject name found in the path is replaced by its partner."""
    for a, b in PARTNERS:
        if a in data_root:
            return data_root.replace(a, b)
    return data_root


def _load(path: str) -> np.ndarray:
    if not os.path.isfile(path):
        raise A2PError(f"{path} is missing: every take needs {_POSE}, {_FACE}, {_MISSING} and {_AUDIO}")
    try:
        return np.load(path)
    except Exception as e:
        raise A2PError(f"{path}: cannot load ({e})") from None


def load_capture(data_root: str, flip_person: bool = False, audio_per_frame: int = AUDIO_PER_FRAME) -> List[Take]:
    """The takes of a capture directory in sorted order (get_data.py:47-129).

    Per `*_body_pose.npy`: the face codes as float64, the missing-frame list, the audio.  A take whose missing list covers every
    frame is skipped.  For the subjects PXB184 / RLW104 pose channel 3 gets `(x + pi) % (2 pi)` twice, in the stored dtype, as
    the reference applies it.  `flip_person` reads the partner's directory and swaps the two audio channels.  The audio must
    hold exactly `audio_per_frame` samples per pose frame in two channels; anything else is an A2PError."""
    if flip_person:
        data_root = partner_root(data_root)
    if not os.path.isdir(data_root):
        raise A2PError(f"{data_root} is not a directory")
    takes: List[Take] = []
    for path in sorted(os.path.join(data_root, x) for x in os.listdir(data_root)):
        if not path.endswith(_POSE):
            continue
        stem = path[: -len(_POSE)]
        code = _load(stem + _FACE).astype(float)
        missing_list = _load(stem + _MISSING)
        if len(missing_list) == len(code):
            continue                                              # no frame of this take has a face code
        present = np.ones(len(code), np.uint8)
        if missing_list.size:
            if not np.issubdtype(missing_list.dtype, np.integer):
                raise A2PError(f"{stem + _MISSING}: frame indices must be integers (got {missing_list.dtype})")
            try:
                present[missing_list] = 0
            except IndexError:
                raise A2PError(f"{stem + _MISSING}: a frame index is outside the take's {len(code)} frames") from None
        pose = _load(path)
        if pose.ndim != 2 or code.ndim != 2 or len(pose) != len(code):
            raise A2PError(f"{stem}: pose {pose.shape} and face codes {code.shape} must be [L, C] with the same L")
        if pose.dtype not in (np.float32, np.float64):
            raise A2PError(f"{path}: poses must be float32 or float64 (got {pose.dtype})")
        if any(s in path for s in UNWRAPPED_SUBJECTS):
            pose[:, 3] = (pose[:, 3] + np.pi) % (2 * np.pi)
            pose[:, 3] = (pose[:, 3] + np.pi) % (2 * np.pi)
        if not os.path.isfile(stem + _AUDIO):
            raise A2PError(f"{stem + _AUDIO} is missing")
        audio, _ = load_wav_normalized(stem + _AUDIO)
        if audio.shape[1] != 2:
            raise A2PError(f"{stem + _AUDIO}: {audio.shape[1]} channel(s); a take holds this person and the partner in two")
        if len(pose) * audio_per_frame != len(audio):
            raise A2PError(f"{stem}: motion {pose.shape} vs audio {audio.shape}: {audio_per_frame} samples per frame are required")
        audio = np.ascontiguousarray(audio[:, ::-1] if flip_person else audio)
        takes.append(Take(stem, pose, code, present, audio))
    if not takes:
        raise A2PError(f"{data_root} holds no usable take (*{_POSE})")
    return takes


# ------------------------------------------------------------------------------------------------ splits and chunks
def split_indices(n: int) -> Dict[str, List[int]]:
    """data.py:52-54: the last 4 takes are the test split, the 2 before them the val split, the rest the train split."""
    if n < 4:
        raise A2PError(f"{n} take(s): the test split is the last 4 takes of a capture")
    return {"train": list(range(0, max(n - 6, 0))), "val": list(range(max(n - 6, 0), n - 4)), "test": list(range(n - 4, n))}


def test_split(takes: Sequence[Take]) -> List[Take]:
    return [takes[i] for i in split_indices(len(takes))["test"]]


test_split.__test__ = False      # not a pytest case when a test module imports it


def chunk_starts(length: int, T: int) -> List[int]:
    """`range(0, length - T, T)` (data.py:122-123)."""
    return list(range(0, int(length) - T, T))


def chunk_plan(lengths: Sequence[int], T: int = 600, seed: Optional[int] = 10) -> np.ndarray:
    """int64 [n, 2]: the (take, start frame) of every T-frame chunk, in the order `Social._chunk_data` leaves them.

    Starts are `range(0, L - T, T)`: a take of exactly k T frames yields k - 1 chunks, and so does one of k T - 1 frames --
    the last full window of a take that ends on a chunk boundary is dropped.  This is the reference's rule and is kept on
    purpose: the published numbers were made with it.  The pairs are then shuffled by
    `np.random.RandomState(seed).permutation(n)`, the draw the reference's `fixseed(seed)` followed by the dataset's
    `np.random.permutation` makes; seed None leaves them in take order."""
    if T < 1:
        raise A2PError(f"T must be positive (got {T})")
    pairs = [(k, s) for k, L in enumerate(lengths) for s in chunk_starts(L, T)]
    plan = np.asarray(pairs, np.int64).reshape(-1, 2)
    if seed is not None and len(plan):
        plan = plan[np.random.RandomState(seed).permutation(len(plan))]
    return plan
