"""Fixture for the capture dataset (audio2photoreal_amd/data/): the reference's own `load_local_data` ->
`Social(split="test", chunk=True)` -> `social_collate` on the seeded synthetic capture directory of tests/dataset_restatement.py
(7 usable takes of 150 frames and one skipped take per subject, window 60), for pose and face, with and without flip_person.
Build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dataset.py

torchaudio is absent: `torchaudio.load` is a stub that reads the 16-bit PCM files with the `wave` module and divides by 32768.
`torch.load` gets weights_only=False (the reference predates that default).  np.random.seed(SEED) stands for `fixseed`.

Only data is stored.  Per configuration `{fmt}/flip{0|1}/`: the shuffle permutation, lengths, mask, one frame column of
`missing`, and SHA-256 digests of every chunk row of inp / keyframes / missing / audio -- the claim under test is bit identity, so
a digest of the bytes checks a tensor in full at 32 bytes per row.  In full: pose inp and keyframes (both flips), face inp
(flip 0).  Audio does not depend on the format: `audio/flip{f}/sample` keeps audio[:, ::193] of every chunk.  The take order,
the channel-3 bits of every loaded pose and the split indices are stored for the host tests."""
import argparse
import os
import shutil
import sys
import tempfile
import types
import wave

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_import as ri  # noqa: E402
import dataset_restatement as R  # noqa: E402


def _stub_load(path):
    with wave.open(path, "rb") as w:
        assert w.getsampwidth() == 2
        C, sr, raw = w.getnchannels(), w.getframerate(), w.readframes(w.getnframes())
    v = np.frombuffer(raw, "<i2").reshape(-1, C).astype(np.float32) / np.float32(32768.0)
    return torch.from_numpy(np.ascontiguousarray(v.T)), sr


def main():
    sys.dont_write_bytecode = True
    ri.install_stubs()
    sys.modules["torchaudio"].load = _stub_load
    sys.path.insert(0, ri.REF)
    import data_loaders.data as rd
    import data_loaders.get_data as rg
    from data_loaders.tensors import social_collate
    orig_load = torch.load
    torch.load = lambda *a, **k: orig_load(*a, **{**k, "weights_only": False})
    tmp = tempfile.mkdtemp()
    out = {"seed": np.int64(R.SEED), "T": np.int64(R.T_SHORT)}
    try:
        for subject in (R.SUBJECT, R.PARTNER):
            R.write_capture(tmp, subject)
        root = os.path.join(tmp, R.SUBJECT)
        shutil.copy(os.path.join(ri.REF, "dataset", R.SUBJECT, "data_stats.pth"), os.path.join(root, "data_stats.pth"))
        audio_of = {}
        for flip in (0, 1):
            for fmt in ("pose", "face"):
                data = rg.load_local_data(root, audio_per_frame=R.SPF, flip_person=bool(flip))
                key = f"{fmt}/flip{flip}"
                if fmt == "pose":
                    out[f"load/flip{flip}/lengths"] = np.asarray(data["lengths"], np.int64)
                    out[f"load/flip{flip}/pose_ch3"] = np.stack([p[:, 3] for p in data["data"]])
                    out[f"load/flip{flip}/pose_sum"] = np.asarray([np.float64(p.astype(np.float64).sum()) for p in data["data"]])
                    out[f"load/flip{flip}/missing_rows"] = np.stack([m[:, 0] for m in data["missing"]]).astype(np.uint8)
                    out[f"load/flip{flip}/audio_head"] = np.stack([a[:64].numpy() for a in data["audio"]])
                args = argparse.Namespace(data_format=fmt, add_frame_cond=1 if fmt == "pose" else None, data_root=root,
                                          max_seq_length=R.T_SHORT, curr_seq_length=None)
                perms = []
                permutation = np.random.permutation

                def recording(n):
                    p = permutation(n)
                    perms.append(np.array(p))
                    return p
                np.random.seed(R.SEED)
                np.random.permutation = recording
                try:
                    ds = rd.Social(args=args, data_dict=data, split="test", chunk=True)
                finally:
                    np.random.permutation = permutation
                motion, cond = social_collate([ds[i] for i in range(len(ds))])
                y = cond["y"]
                assert motion.dtype == torch.float32 and y["audio"].dtype == torch.float32 and len(perms) == 1
                out[f"{key}/perm"] = perms[0].astype(np.int64)
                out[f"{key}/lengths"] = y["lengths"].numpy()
                out[f"{key}/alengths"] = y["alengths"].numpy()
                out[f"{key}/klengths"] = y["klengths"].numpy()
                out[f"{key}/mask"] = y["mask"].numpy()
                miss = y["missing"].numpy()
                assert (miss == miss[:, :, :1]).all()
                out[f"{key}/missing_col"] = miss[:, :, 0].astype(np.uint8)
                tensors = {"inp": motion.numpy(), "keyframes": y["keyframes"].numpy(), "missing": miss, "audio": y["audio"].numpy()}
                for name, v in tensors.items():
                    out[f"{key}/sha256/{name}"] = R.digest_rows(v)
                    out[f"{key}/shape/{name}"] = np.asarray(v.shape, np.int64)
                if fmt == "pose" or flip == 0:
                    out[f"{key}/inp"] = tensors["inp"]
                if fmt == "pose":
                    out[f"{key}/keyframes"] = tensors["keyframes"]
                else:   # the face keyframes are inp's values, frame-major
                    assert np.array_equal(tensors["keyframes"].view(np.uint32), tensors["inp"][:, :, 0].transpose(0, 2, 1).view(np.uint32))
                if flip in audio_of:
                    assert np.array_equal(audio_of[flip].view(np.uint32), tensors["audio"].view(np.uint32))
                else:
                    audio_of[flip] = tensors["audio"]
                    out[f"audio/flip{flip}/sample"] = np.ascontiguousarray(tensors["audio"][:, ::R.AUDIO_STRIDE])
        n = len(out["load/flip0/lengths"])
        out["split/train"] = np.asarray(list(range(0, n - 6)), np.int64)
        out["split/val"] = np.asarray(list(range(n - 6, n - 4)), np.int64)
        out["split/test"] = np.asarray(list(range(n - 4, n)), np.int64)
    finally:
        torch.load = orig_load
        shutil.rmtree(tmp)
    np.savez_compressed(R.GOLDEN, **out)
    size = os.path.getsize(R.GOLDEN)
    print(R.GOLDEN, size, "bytes")
    assert size <= 1 << 20, "a committed file stays within 1 MiB"
    print({k: (v.dtype, v.shape) for k, v in out.items() if "sha256" not in k and "shape" not in k})


if __name__ == "__main__":
    main()
