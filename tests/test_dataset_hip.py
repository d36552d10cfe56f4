"""GPU side of the capture dataset: `CaptureBatches.batch` (a2p_dataset_batch, csrc/kernels_dataset.h) against the reference's
own loader (tests/golden/golden_dataset_v1.npz) bit for bit, against the numpy restatement at the real window, and the command
`python -m audio2photoreal_amd.sample.dataset` end to end on synthetic weights.  Both sides perform the same correctly rounded
operations, so every comparison of batch tensors is on the raw bits: no tolerance applies."""
import json
import os

import numpy as np
import pytest
import torch

import dataset_restatement as R
from audio2photoreal_amd.data import capture as cap

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gold():
    return np.load(R.GOLDEN)


@pytest.fixture(scope="module")
def root(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("capture"))
    for subject in (R.SUBJECT, R.PARTNER):
        R.write_capture(tmp, subject)
    return os.path.join(tmp, R.SUBJECT)


def _same_bits(t, want):
    """torch.equal on the raw bytes of a device tensor and a numpy array."""
    w = torch.from_numpy(np.ascontiguousarray(want))
    t = t.detach().cpu().contiguous()
    return t.dtype == w.dtype and t.shape == w.shape and torch.equal(t.reshape(-1).view(torch.uint8), w.reshape(-1).view(torch.uint8))


def _batches(takes, fmt, T, seed, **kw):
    from audio2photoreal_amd.data.batches import CaptureBatches
    return CaptureBatches(takes, R.golden_stats(), fmt, T=T, seed=seed, device="cuda", **kw)


@pytest.mark.parametrize("flip", [0, 1])
@pytest.mark.parametrize("B", [1, 3, 8])
@pytest.mark.parametrize("fmt", ["pose", "face"])
def test_batch_matches_the_reference_bit_for_bit(gold, root, fmt, B, flip):
    takes = cap.test_split(cap.load_capture(root, flip_person=bool(flip)))
    data = _batches(takes, fmt, R.T_SHORT, int(gold["seed"]))
    key = f"{fmt}/flip{flip}"
    assert len(data) == 8
    idx = {1: [5], 3: [6, 0, 3], 8: list(range(8))}[B]
    gt, kw = data.batch(idx)
    y = kw["y"]
    got = {"inp": gt, "keyframes": y["keyframes"], "missing": y["missing"], "audio": y["audio"]}
    for name, t in got.items():
        assert t.is_cuda and t.dtype == torch.float32
        assert list(t.shape) == [B] + list(gold[f"{key}/shape/{name}"][1:])
        assert np.array_equal(R.digest_rows(t.cpu().numpy()), gold[f"{key}/sha256/{name}"][idx]), name     # every byte of every row
    if f"{key}/inp" in gold.files:
        assert _same_bits(gt, gold[f"{key}/inp"][idx])
    if f"{key}/keyframes" in gold.files:
        assert _same_bits(y["keyframes"], gold[f"{key}/keyframes"][idx])
    else:
        assert _same_bits(y["keyframes"], gt[:, :, 0].permute(0, 2, 1).contiguous().cpu().numpy())   # the generator checked this identity
    assert _same_bits(y["missing"][:, :, 0].to(torch.uint8), gold[f"{key}/missing_col"][idx])
    assert _same_bits(y["audio"][:, ::R.AUDIO_STRIDE].contiguous(), gold[f"audio/flip{flip}/sample"][idx])
    assert _same_bits(y["mask"], gold[f"{key}/mask"][idx])
    for name in ("lengths", "alengths", "klengths"):
        assert _same_bits(y[name], gold[f"{key}/{name}"][idx])


def test_kernel_channel_swap_equals_the_flipped_load(root):
    partner = cap.test_split(cap.load_capture(os.path.join(os.path.dirname(root), R.PARTNER)))
    flipped = cap.test_split(cap.load_capture(root, flip_person=True))
    a = _batches(partner, "pose", R.T_SHORT, 3, swap_channels=True).batch(range(8))[1]["y"]["audio"]
    b = _batches(flipped, "pose", R.T_SHORT, 3).batch(range(8))[1]["y"]["audio"]
    assert _same_bits(a, b.cpu().numpy())


@pytest.fixture(scope="module")
def ragged(tmp_path_factory):
    """T = 600: takes of unequal lengths, fp64 and fp32 pose files in one directory."""
    tmp = str(tmp_path_factory.mktemp("ragged"))
    lengths = (610, 700, 1300, 1201, 1850, 601)
    d = R.write_capture(tmp, "RLW104", lengths=lengths, seed=77, skipped_take=None,
                        pose_dtype=(np.float32, np.float32, np.float64, np.float32, np.float64, np.float32))
    return cap.test_split(cap.load_capture(d))


@pytest.mark.parametrize("fmt", ["pose", "face"])
def test_real_window_matches_the_numpy_restatement(ragged, fmt):
    assert [t.pose.dtype for t in ragged] == [np.float64, np.float32, np.float64, np.float32]
    data = _batches(ragged, fmt, 600, 10)
    assert len(data) == 2 + 2 + 3 + 1 and sorted(map(tuple, data.plan.tolist())) == sorted(
        [(0, 0), (0, 600), (1, 0), (1, 600), (2, 0), (2, 600), (2, 1200), (3, 0)])
    idx = list(range(8))
    gt, kw = data.batch(idx)
    want = R.numpy_batch(ragged, R.golden_stats(), fmt, data.plan[idx].tolist(), 600)
    y = kw["y"]
    assert gt.shape == (8, 104 if fmt == "pose" else 256, 1, 600) and y["keyframes"].shape[1] == (20 if fmt == "pose" else 600)
    assert _same_bits(gt, want["inp"])
    assert _same_bits(y["keyframes"], want["keyframes"])
    assert _same_bits(y["missing"], want["missing"])
    assert _same_bits(y["audio"], want["audio"])
    if fmt == "face":
        assert (want["missing"] == 0).any() and (np.signbit(want["inp"]) & (want["inp"] == 0)).sum() == 0


@pytest.mark.parametrize("fmt", ["pose", "face"])
def test_a_chunk_does_not_depend_on_its_batch(ragged, fmt):
    data = _batches(ragged, fmt, 600, 10)
    gt8, kw8 = data.batch(range(8))
    for i in (0, 3, 7):
        gt1, kw1 = data.batch([i])
        assert _same_bits(gt1, gt8[i:i + 1].cpu().numpy())
        for name in ("keyframes", "missing", "audio"):
            assert _same_bits(kw1["y"][name], kw8["y"][name][i:i + 1].cpu().numpy()), name


# ---------------------------------------------------------------------------------------------- the command, end to end
def _checkpoint(tmp_path, fmt):
    from audio2photoreal_amd.spec import face_spec, pose_spec
    from audio2photoreal_amd.synthetic import synthetic_frontend_state_dict, synthetic_state_dict
    spec = face_spec(num_layers=2) if fmt == "face" else pose_spec(num_layers=2)
    run = tmp_path / f"c1_{fmt}"
    os.makedirs(str(run), exist_ok=True)
    torch.save({**synthetic_state_dict(spec, 10), **synthetic_frontend_state_dict(10, lip=fmt == "face")}, str(run / "model000000010.pt"))
    with open(str(run / "args.json"), "w") as f:
        json.dump({"data_format": fmt, "layers": 2, "heads": spec.num_heads, "max_seq_length": 600}, f)
    return str(run / "model000000010.pt")


@pytest.fixture(scope="module")
def ragged_root(tmp_path_factory):
    tmp = str(tmp_path_factory.mktemp("e2e"))
    d = R.write_capture(tmp, "PXB184", lengths=(610, 700, 1300, 1201, 1850, 601), seed=78, skipped_take=None)
    torch.save(R.golden_stats(), os.path.join(d, "data_stats.pth"))
    return d


@pytest.mark.parametrize("fmt", ["pose", "face"])
def test_command_end_to_end(tmp_path, ragged_root, fmt):
    from audio2photoreal_amd.evaluate import METRICS, evaluate_motion
    from audio2photoreal_amd.sample import dataset as cmd
    from audio2photoreal_amd.sample.generate import load_results
    ckpt = _checkpoint(tmp_path, fmt)
    Rn, B, T, C = 2, 3, 600, (104 if fmt == "pose" else 256)
    common = ["--model_path", ckpt, "--data_root", ragged_root, "--num_samples", str(B), "--num_repetitions", str(Rn),
              "--timestep_respacing", "ddim10", "--seed", "10"]
    out1, out2, js = str(tmp_path / "o1"), str(tmp_path / "o2"), str(tmp_path / "m.json")
    res = cmd.run(cmd.build_parser().parse_args(common + ["--output_dir", out1, "--evaluate", "--json", js, "--diversity_times", "1000"]))
    block = load_results(res["results"])
    assert sorted(block) == ["audio", "gt", "keyframes", "lengths", "motions"]
    assert block["motions"].shape == (Rn * B, C, 1, T) and block["gt"].shape == (Rn * B, C, 1, T)
    assert block["audio"].shape == (Rn * B, T * 1600, 2) and block["lengths"].tolist() == [T] * (Rn * B)
    assert block["keyframes"].shape == (Rn * B, 20 if fmt == "pose" else T, C)
    assert np.isfinite(block["motions"]).all()

    # gt un-normalises back to the stored takes: one fp32 rounding of the normalised value carried through * std + mean in fp64
    takes = cap.test_split(cap.load_capture(ragged_root))
    plan = cap.chunk_plan([t.frames for t in takes], T, 10)
    stats = R.golden_stats()
    mean = stats["pose_mean"].reshape(-1) if fmt == "pose" else stats["code_mean"]
    std = stats["pose_std"].reshape(-1) if fmt == "pose" else stats["code_std"]
    for r in range(Rn):
        for b in range(B):
            k, s = plan[b]
            x = (takes[k].pose if fmt == "pose" else takes[k].face)[s:s + T].astype(np.float64)
            got = block["gt"][r * B + b, :, 0].T
            present = np.ones(T, bool) if fmt == "pose" else takes[k].present[s:s + T] == 1
            bound = 2.0 ** -23 * (np.abs(x - mean) + std)
            assert (np.abs(got - x)[present] <= bound[present]).all()
            if fmt == "face":
                assert np.array_equal(got[~present], np.broadcast_to(mean, got.shape)[~present])   # face gt = code_mean on missing frames

    # --evaluate: five finite metrics, equal to evaluate_motion on the loaded block
    saved = json.load(open(js))
    want = evaluate_motion(block["motions"], block["gt"], num_samples=Rn, diversity_times=1000, seed=0)
    for m in METRICS:
        assert np.isfinite(saved[m]) and saved[m] == want[m] == res["metrics"][m], m
    assert {"load_s", "upload_s", "batch_s", "sample_s", "evaluate_s"} <= set(saved["timing"])

    # the same seed gives the same file twice
    res2 = cmd.run(cmd.build_parser().parse_args(common + ["--output_dir", out2]))
    block2 = load_results(res2["results"])
    for key in block:
        assert np.array_equal(block[key], block2[key]), key


def test_all_visits_every_chunk_once(tmp_path, ragged_root):
    from audio2photoreal_amd.sample import dataset as cmd
    from audio2photoreal_amd.sample.generate import load_results
    ckpt = _checkpoint(tmp_path, "pose")
    Rn, B, T = 2, 3, 600
    res = cmd.run(cmd.build_parser().parse_args(
        ["--model_path", ckpt, "--data_root", ragged_root, "--num_samples", str(B), "--num_repetitions", str(Rn),
         "--timestep_respacing", "ddim10", "--sampler", "dpm++2m", "--all", "--output_dir", str(tmp_path / "all")]))
    block = load_results(res["results"])
    takes = cap.test_split(cap.load_capture(ragged_root))
    plan = cap.chunk_plan([t.frames for t in takes], T, 10)
    n = len(plan)
    assert n == 8 and res["chunks"] == n and block["motions"].shape == (Rn * n, 104, 1, T)       # batches of 3, 3 and a short one of 2
    stats = R.golden_stats()
    inv_audio = lambda a: a * stats["audio_std_flat"] + stats["audio_mean"]                        # noqa: E731
    for r in range(Rn):
        for i, (k, s) in enumerate(plan):                                                           # repetition-major over the whole plan
            want = inv_audio((takes[k].audio[s * 1600:(s + T) * 1600] - stats["audio_mean"]) / stats["audio_std_flat"])
            assert np.array_equal(block["audio"][r * n + i], want), (r, i)
    assert not np.array_equal(block["motions"][:n], block["motions"][n:])                          # repetitions draw fresh noise
