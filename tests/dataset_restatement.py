"""Seeded synthetic capture directories and a numpy restatement of the dataset arithmetic, shared by
tests/golden/make_golden_dataset.py (which runs the reference's own loader on the directory) and tests/test_dataset_*.py
(which rebuild the same directory from the seed: the inputs are not committed)."""
import hashlib
import os
import struct
import wave

import numpy as np

SEED = 20240
T_SHORT, L_SHORT = 60, 150                 # the fixture's window and take length: 2 chunks per take, 8 in the test split
N_TAKES = 7                                # usable takes (one more take has every face frame missing and is skipped)
SUBJECT, PARTNER = "PXB184", "RLW104"
SPF = 1600
AUDIO_STRIDE = 193                         # the fixture keeps audio[:, ::193] of every chunk (and a digest of every full chunk)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "golden_dataset_v1.npz")


def write_pcm16(path, samples):
    """samples int16 [L, C] -> 16-bit PCM WAV at 48 kHz."""
    with wave.open(path, "wb") as w:
        w.setnchannels(samples.shape[1])
        w.setsampwidth(2)
        w.setframerate(48000)
        w.writeframes(np.ascontiguousarray(samples, "<i2").tobytes())


def write_float32_wav(path, samples, sr=48000):
    """samples float32 [L, C] -> IEEE-float WAV (format tag 3) with an odd-sized LIST chunk in front of the data."""
    L, C = samples.shape
    data = np.ascontiguousarray(samples, "<f4").tobytes()
    fmt = struct.pack("<HHIIHH", 3, C, sr, sr * C * 4, C * 4, 32)
    junk = b"LIST" + struct.pack("<I", 5) + b"hello" + b"\0"
    body = b"WAVE" + b"fmt " + struct.pack("<I", len(fmt)) + fmt + junk + b"data" + struct.pack("<I", len(data)) + data
    with open(path, "wb") as f:
        f.write(b"RIFF" + struct.pack("<I", len(body)) + body)


def take_arrays(rs, L, pose_dtype=np.float32, n_missing=9):
    pose = (rs.standard_normal((L, 104)) * 0.7).astype(pose_dtype)
    pose[:, 3] = rs.uniform(-np.pi, 3 * np.pi, L).astype(pose_dtype)          # the unwrap of channel 3 has something to do
    face = rs.standard_normal((L, 256)) * 1.5
    face[rs.randint(0, L, 5), rs.randint(0, 256, 5)] *= -1.0                   # negative values on frames that may be missing: -0.0
    missing = np.sort(rs.choice(L, n_missing, replace=False)).astype(np.int64)
    audio = rs.randint(-6000, 6000, (L * SPF, 2)).astype(np.int16)
    return pose, face, missing, audio


def write_capture(root, subject=SUBJECT, lengths=(L_SHORT,) * N_TAKES, seed=SEED, pose_dtype=np.float32, skipped_take=2,
                  float_wav_take=None):
    """`root/subject/` with len(lengths) usable takes `scene{k:02d}_*` (+ one whose missing list covers every frame, in
    position `skipped_take` of the sorted listing; None: no such take), an unrelated file, and no data_stats.pth.
    Take 1 has an empty missing list.  `float_wav_take`: that take's audio is written as float32 WAV holding the PCM values
    / 32768.  Returns the directory."""
    d = os.path.join(root, subject)
    os.makedirs(d, exist_ok=True)
    rs = np.random.RandomState(seed + sum(ord(c) for c in subject))
    names = [f"scene{k:02d}" for k in range(len(lengths) + (skipped_take is not None))]
    usable = 0
    for k, name in enumerate(names):
        if skipped_take is not None and k == skipped_take:
            L = 40
            pose, face, missing, audio = take_arrays(rs, L, pose_dtype)
            missing = np.arange(L, dtype=np.int64)
        else:
            L = lengths[usable]
            pose, face, missing, audio = take_arrays(rs, L, pose_dtype if np.isscalar(pose_dtype) or isinstance(pose_dtype, type)
                                                     else pose_dtype[usable], n_missing=0 if usable == 1 else 9)
            if float_wav_take is not None and usable == float_wav_take:
                audio = audio.astype(np.float32) / np.float32(32768.0)
            usable += 1
        np.save(os.path.join(d, name + "_body_pose.npy"), pose)
        np.save(os.path.join(d, name + "_face_expression.npy"), face)
        np.save(os.path.join(d, name + "_missing_face_frames.npy"), missing)
        (write_float32_wav if audio.dtype == np.float32 else write_pcm16)(os.path.join(d, name + "_audio.wav"), audio)
    with open(os.path.join(d, "notes.txt"), "w") as f:
        f.write("not a take\n")
    return d


def golden_stats():
    """PXB184's statistics as the reference reads them (tests/golden/golden_stats_v1.npz, made from its data_stats.pth)."""
    g = np.load(os.path.join(os.path.dirname(GOLDEN), "golden_stats_v1.npz"))
    return {k[len("stats/"):]: g[k] for k in g.files if k.startswith("stats/")}


def digest_rows(x):
    """uint8 [B, 32]: SHA-256 of the bytes of every row x[b] (a bit-for-bit comparison of tensors too large to commit)."""
    x = np.ascontiguousarray(x)
    return np.stack([np.frombuffer(hashlib.sha256(x[b].tobytes()).digest(), np.uint8) for b in range(len(x))])


def numpy_batch(takes, stats, data_format, rows, T, swap=False):
    """The expressions of data_loaders/data.py:232-253 + tensors.py:19-29, 74-82 on chunks `rows` = [(take, start)] of `takes`
    (objects with .pose/.face/.present/.audio): dict of inp [B, C, 1, T], keyframes, missing, audio as float32."""
    step = 30 if data_format == "pose" else 1
    mean = stats["pose_mean"].reshape(-1) if data_format == "pose" else stats["code_mean"]
    std = stats["pose_std"].reshape(-1) if data_format == "pose" else stats["code_std"]
    out = {"inp": [], "keyframes": [], "missing": [], "audio": []}
    for k, s in rows:
        t = takes[k]
        motion = (t.pose if data_format == "pose" else t.face)[s:s + T]
        audio = t.audio[s * SPF:(s + T) * SPF]
        if swap:
            audio = audio[:, ::-1]
        if data_format == "pose":
            missing = np.ones_like(motion)
        else:
            missing = np.ones_like(motion)
            missing[t.present[s:s + T] == 0] = 0.0
        motion = (motion - mean) / std
        audio = (audio - stats["audio_mean"]) / stats["audio_std_flat"]
        keyframes = motion[::step]
        if data_format == "face":
            motion *= missing
        assert audio.dtype == np.float32 and motion.dtype == np.float64
        out["inp"].append(motion.T.astype(np.float32)[:, None, :])
        out["keyframes"].append(keyframes.astype(np.float32))
        out["missing"].append(missing.astype(np.float32))
        out["audio"].append(np.ascontiguousarray(audio))
    # collate_tensors (tensors.py:23-28) adds every sample into a zeroed canvas: -0.0 becomes +0.0
    return {k: np.zeros((len(v),) + v[0].shape, np.float32) + np.stack(v) for k, v in out.items()}
