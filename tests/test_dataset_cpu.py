"""Host side of the capture dataset (audio2photoreal_amd/data/capture.py, the argument checks of data/batches.py and
sample/dataset.py) against tests/golden/golden_dataset_v1.npz, which the reference's own loader wrote for the seeded directory
of tests/dataset_restatement.py.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

import dataset_restatement as R
from audio2photoreal_amd import _lib
from audio2photoreal_amd._lib import A2PError
from audio2photoreal_amd.data import capture as cap


@pytest.fixture(scope="module")
def gold():
    return np.load(R.GOLDEN)


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("capture"))
    for subject in (R.SUBJECT, R.PARTNER):
        R.write_capture(tmp, subject)
    return os.path.join(tmp, R.SUBJECT)


@pytest.fixture()
def no_library(monkeypatch):
    """Any attempt to load the HIP library (or to touch the GPU through torch) fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the HIP library was loaded before the arguments were checked")
    monkeypatch.setattr(_lib, "load", refuse)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


# ---------------------------------------------------------------------------------------------- takes
@pytest.mark.parametrize("flip", [0, 1])
def test_take_order_skip_rule_unwrap_bits_and_split(gold, root, flip):
    takes = cap.load_capture(root, flip_person=bool(flip))
    subject = R.PARTNER if flip else R.SUBJECT
    assert [os.path.basename(t.name) for t in takes] == [f"scene{k:02d}" for k in (0, 1, 3, 4, 5, 6, 7)]   # scene02: every frame missing
    assert all(os.path.basename(os.path.dirname(t.name)) == subject for t in takes)
    assert [t.frames for t in takes] == list(gold[f"load/flip{flip}/lengths"])
    ch3 = np.stack([t.pose[:, 3] for t in takes])
    assert ch3.dtype == np.float32 and np.array_equal(_bits(ch3), _bits(gold[f"load/flip{flip}/pose_ch3"]))
    assert np.array_equal(np.asarray([t.pose.astype(np.float64).sum() for t in takes]), gold[f"load/flip{flip}/pose_sum"])
    assert np.array_equal(np.stack([t.present for t in takes]), gold[f"load/flip{flip}/missing_rows"])
    assert all(t.face.dtype == np.float64 and t.missing().shape == t.face.shape for t in takes)
    assert np.array_equal(takes[0].missing()[:, 7], takes[0].present.astype(np.float64))
    assert takes[1].present.all()                                                     # its missing list is empty
    head = np.stack([t.audio[:64] for t in takes])
    assert head.dtype == np.float32 and np.array_equal(_bits(head), _bits(gold[f"load/flip{flip}/audio_head"]))
    idx = cap.split_indices(len(takes))
    for name in ("train", "val", "test"):
        assert idx[name] == list(gold[f"split/{name}"])
    assert [t.name for t in cap.test_split(takes)] == [takes[i].name for i in idx["test"]]


def test_flip_swaps_the_audio_channels(root):
    partner = cap.load_capture(os.path.join(os.path.dirname(root), R.PARTNER))
    flipped = cap.load_capture(root, flip_person=True)
    for a, b in zip(partner, flipped):
        assert np.array_equal(a.audio[:, ::-1], b.audio) and np.array_equal(a.pose, b.pose)


@pytest.mark.parametrize("fmt", ["pose", "face"])
@pytest.mark.parametrize("flip", [0, 1])
def test_chunk_plan_and_permutation_match_the_reference(gold, root, fmt, flip):
    takes = cap.test_split(cap.load_capture(root, flip_person=bool(flip)))
    lengths = [t.frames for t in takes]
    ordered = cap.chunk_plan(lengths, R.T_SHORT, seed=None)
    assert ordered.tolist() == [[k, s] for k in range(4) for s in (0, 60)]
    plan = cap.chunk_plan(lengths, R.T_SHORT, seed=int(gold["seed"]))
    perm = gold[f"{fmt}/flip{flip}/perm"]
    assert np.array_equal(plan, ordered[perm])
    # ... and the reference's tensors are those chunks: the numpy restatement of its arithmetic reproduces them bit for bit
    got = R.numpy_batch(takes, R.golden_stats(), fmt, plan.tolist(), R.T_SHORT)
    for name in ("inp", "keyframes", "missing", "audio"):
        assert list(got[name].shape) == list(gold[f"{fmt}/flip{flip}/shape/{name}"])
        assert np.array_equal(R.digest_rows(got[name]), gold[f"{fmt}/flip{flip}/sha256/{name}"]), name
    assert np.array_equal(_bits(got["audio"][:, ::R.AUDIO_STRIDE]), _bits(gold[f"audio/flip{flip}/sample"]))
    if f"{fmt}/flip{flip}/inp" in gold.files:
        assert np.array_equal(_bits(got["inp"]), _bits(gold[f"{fmt}/flip{flip}/inp"]))


@pytest.mark.parametrize("T", [600, 60, 7])
def test_chunk_starts_follow_the_reference_range(T):
    for L in (T, T + 1, 2 * T, 2 * T + 1, (5 * T) // 2):
        assert cap.chunk_starts(L, T) == list(range(0, L - T, T))
    assert cap.chunk_starts(T, T) == [] and cap.chunk_starts(2 * T, T) == [0] and cap.chunk_starts(2 * T + 1, T) == [0, T]
    assert cap.chunk_starts(T - 5, T) == []
    assert "k - 1 chunks" in cap.chunk_plan.__doc__


def test_ragged_takes_load_and_are_planned(tmp_path):
    lengths = (70, 130, 61, 200, 60, 181, 125)
    d = R.write_capture(str(tmp_path), "GQS883", lengths=lengths, seed=5, pose_dtype=np.float64, skipped_take=None)
    takes = cap.load_capture(d)
    assert [t.frames for t in takes] == list(lengths) and takes[0].pose.dtype == np.float64
    raw = np.load(takes[0].name + "_body_pose.npy")
    assert np.array_equal(raw, takes[0].pose)                                        # GQS883: channel 3 is not unwrapped
    test = cap.test_split(takes)
    assert [t.frames for t in test] == [200, 60, 181, 125]
    plan = cap.chunk_plan([t.frames for t in test], 60, seed=None)
    assert plan.tolist() == [[0, 0], [0, 60], [0, 120], [2, 0], [2, 60], [2, 120], [3, 0], [3, 60]]
    shuffled = cap.chunk_plan([t.frames for t in test], 60, seed=3)
    assert np.array_equal(shuffled, plan[np.random.RandomState(3).permutation(8)])
    np.random.seed(3)                                                                # fixseed(3), then the dataset's draw
    assert np.array_equal(shuffled, plan[np.random.permutation(8)])


# ---------------------------------------------------------------------------------------------- WAV
def test_wav_reading_matches_hand_built_files(tmp_path):
    rs = np.random.RandomState(0)
    pcm = rs.randint(-32768, 32768, (500, 2)).astype(np.int16)
    pcm[0] = (-32768, 32767)
    p16 = str(tmp_path / "a.wav")
    R.write_pcm16(p16, pcm)
    got, sr = cap.load_wav_normalized(p16)
    assert sr == 48000 and got.dtype == np.float32 and got.shape == (500, 2)
    assert np.array_equal(got, pcm.astype(np.float32) / np.float32(32768.0))
    assert got[0, 0] == -1.0 and got[0, 1] == np.float32(32767 / 32768)
    flt = rs.standard_normal((333, 2)).astype(np.float32)
    pf = str(tmp_path / "f.wav")
    R.write_float32_wav(pf, flt, sr=16000)
    got, sr = cap.load_wav_normalized(pf)
    assert sr == 16000 and got.dtype == np.float32 and np.array_equal(_bits(got), _bits(flt))
    with open(str(tmp_path / "bad.wav"), "wb") as f:
        f.write(b"RIFFxxxxWAVEjunk")
    with pytest.raises(A2PError):
        cap.load_wav_normalized(str(tmp_path / "bad.wav"))


def test_float_wav_take_equals_the_pcm_take(tmp_path):
    a = cap.load_capture(R.write_capture(str(tmp_path / "a"), "TXB805", lengths=(20,) * 4, seed=9, skipped_take=None))
    b = cap.load_capture(R.write_capture(str(tmp_path / "b"), "TXB805", lengths=(20,) * 4, seed=9, skipped_take=None, float_wav_take=2))
    assert np.array_equal(_bits(a[2].audio), _bits(b[2].audio))


# ---------------------------------------------------------------------------------------------- errors, all on the host
def test_capture_errors(tmp_path, no_library):
    with pytest.raises(A2PError, match="not a directory"):
        cap.load_capture(str(tmp_path / "nowhere"))
    os.makedirs(str(tmp_path / "empty"))
    with pytest.raises(A2PError, match="no usable take"):
        cap.load_capture(str(tmp_path / "empty"))
    d = R.write_capture(str(tmp_path), "TXB805", lengths=(20,) * 4, seed=1, skipped_take=None)
    pcm = np.zeros((20 * R.SPF - 2, 2), np.int16)
    R.write_pcm16(os.path.join(d, "scene01_audio.wav"), pcm)
    with pytest.raises(A2PError, match="vs audio"):
        cap.load_capture(d)
    R.write_pcm16(os.path.join(d, "scene01_audio.wav"), np.zeros((20 * R.SPF, 1), np.int16))
    with pytest.raises(A2PError, match="channel"):
        cap.load_capture(d)
    os.remove(os.path.join(d, "scene01_audio.wav"))
    with pytest.raises(A2PError, match="missing"):
        cap.load_capture(d)
    with pytest.raises(A2PError, match="last 4 takes"):
        cap.split_indices(3)


def test_batches_reject_bad_arguments_before_the_library_loads(root, no_library):
    from audio2photoreal_amd.data.batches import CaptureBatches
    takes = cap.test_split(cap.load_capture(root))
    stats = R.golden_stats()
    with pytest.raises(A2PError, match="data_format"):
        CaptureBatches(takes, stats, "hands", T=60)
    with pytest.raises(A2PError, match="lack"):
        CaptureBatches(takes, {k: v for k, v in stats.items() if k != "audio_std_flat"}, "pose", T=60)
    with pytest.raises(A2PError, match="empty"):
        CaptureBatches(takes, stats, "pose", T=150)                      # range(0, 150 - 150, 150) is empty
    with pytest.raises(A2PError, match="no take"):
        CaptureBatches([], stats, "pose", T=60)
    with pytest.raises(A2PError, match="positive"):
        CaptureBatches(takes, stats, "pose", T=0)
    with pytest.raises(A2PError, match="MI355X"):
        CaptureBatches(takes, stats, "pose", T=60, device="cpu")
    bad = [takes[0]._replace(audio=takes[0].audio[:-2])] + takes[1:]
    with pytest.raises(A2PError, match="audio"):
        CaptureBatches(bad, stats, "pose", T=60)
    with pytest.raises(A2PError, match="channels"):
        CaptureBatches(takes, {**stats, "pose_mean": stats["pose_mean"][:100], "pose_std": stats["pose_std"][:100]}, "pose", T=60)


def test_command_errors_come_before_any_gpu_work(root, tmp_path, no_library):
    from audio2photoreal_amd.sample import dataset as cmd
    ckpt = tmp_path / "run" / "model000001.pt"
    os.makedirs(str(ckpt.parent))
    torch.save({}, str(ckpt))
    base = ["--model_path", str(ckpt), "--data_root", root, "--num_samples", "2", "--num_repetitions", "1"]
    with pytest.raises(A2PError, match="args.json"):
        cmd.main(base)
    with open(str(ckpt.parent / "args.json"), "w") as f:
        json.dump({"data_format": "pose", "layers": 2, "heads": 8, "max_seq_length": 60}, f)
    with pytest.raises(A2PError, match="data_stats.pth"):
        cmd.main(base)
    torch.save(R.golden_stats(), os.path.join(root, "data_stats.pth"))
    try:
        with pytest.raises(A2PError, match="renderer"):
            cmd.main(base + ["--plot"])
        with pytest.raises(A2PError, match="sampler"):
            cmd.main(base + ["--sampler", "euler"])
        with pytest.raises(A2PError, match="not found"):
            cmd.main(["--model_path", str(tmp_path / "none.pt"), "--data_root", root])
        with pytest.raises(A2PError, match="empty"):
            cmd.main(base + ["--max_seq_length", "150"])
        with pytest.raises(A2PError, match="num_samples"):
            cmd.main(base[:4] + ["--num_samples", "9"])               # the split has 8 chunks
    finally:
        os.remove(os.path.join(root, "data_stats.pth"))
