"""Motion evaluation, host side (no GPU): the fixture of the reference's utils/eval.py against the float64 restatement
(tests/eval_restatement.py), the diversity draw against the reference's indices, the host validation (every error before any
GPU work), the command line and the results-key fallback of audio2photoreal_amd/evaluate.py."""
import os

import numpy as np
import pytest
import torch

import eval_restatement as R
from audio2photoreal_amd import _lib, evaluate as E
from audio2photoreal_amd._lib import A2PError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_eval_v1.npz"))


@pytest.fixture(scope="module")
def case_a():
    return R.make_case("a")


def test_fixture_seeds_regenerate_the_inputs(gold):
    for name, spec in R.CASES.items():
        assert int(gold[f"{name}/seed"]) == spec["seed"]
        pred, gt, ns = R.make_case(name)
        assert pred.dtype == np.float32 and pred.shape == (spec["num_samples"] * spec["B"], spec["C"], spec["T"])
        assert np.array_equal(pred * R.Q, np.round(pred * R.Q))                    # on the 2^-12 grid: exact float32 deltas
        # the means of the regenerated inputs are the reference's (float64 statistics of the same frames)
        assert np.allclose(R.frames(pred).mean(0), gold[f"{name}/pred_mu_g"], rtol=0, atol=1e-12)
        assert np.allclose(R.velocities(gt).mean(0), gold[f"{name}/gt_mu_k"], rtol=0, atol=1e-12)


def test_fixture_covariances_match_the_restatement(gold, case_a):
    pred, gt, _ = case_a
    iu = np.triu_indices(pred.shape[1])
    for key, rows in (("a/pred_cov_g_triu", R.frames(pred)), ("a/gt_cov_k_triu", R.velocities(gt))):
        want = R.stats(rows)[1][iu]
        assert np.abs(gold[key] - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_fixture_metrics_match_the_restatement(gold, name):
    pred, gt, ns = R.make_case(name)
    i1, i2 = E.diversity_indices(pred.shape[0] * pred.shape[2], R.DIVERSITY_TIMES, R.DIVERSITY_SEED)
    want = R.evaluate(pred, gt, ns, i1, i2)
    # the reference takes np.var / linalg.norm of float32 arrays: agreement within float32 rounding
    for k in ("cross_var", "var_k", "var_g"):
        assert abs(float(gold[f"{name}/{k}"]) - want[k]) <= 1e-5 * abs(want[k]), k
    for k in ("fid_g", "fid_k"):
        tr = np.trace(R.stats(R.frames(gt) if k == "fid_g" else R.velocities(gt))[1]) * 2
        got = float(gold[f"{name}/{k}64"])
        if name == "d":
            assert abs(got) <= 1e-9 * tr and abs(want[k]) <= 1e-9 * tr
        elif name == "c":   # singular gt covariance: scipy's sqrtm of the singular product carries O(sqrt(eps)) terms
            assert abs(got - want[k]) <= 1e-6 * tr, (k, got, want[k])
        else:
            assert abs(got - want[k]) <= 1e-9 * tr, (k, got, want[k])
        # main's own number (float32 means: |dmu|^2 in float32) stays within float32 rounding of the float64 one
        assert abs(float(gold[f"{name}/{k}"]) - got) <= 1e-6 * (abs(got) + tr)


def test_host_draw_equals_the_reference_indices(gold, case_a):
    pred = case_a[0]
    i1, i2 = E.diversity_indices(pred.shape[0] * pred.shape[2], int(gold["diversity_times"]), int(gold["diversity_seed"]))
    assert i1.dtype == np.int64 and np.array_equal(i1, gold["a/idx1"]) and np.array_equal(i2, gold["a/idx2"])
    assert np.allclose(R.pair_distances(pred, i1, i2), gold["a/dist"], rtol=1e-6, atol=0)
    with pytest.raises(A2PError, match="more frames than draws"):
        E.diversity_indices(10_000, 10_000, 0)                                      # the reference asserts N > times


@pytest.fixture
def no_gpu(monkeypatch):
    """Any attempt to reach the library or a device fails the test."""
    def boom(*a, **k):
        raise AssertionError("GPU work before the host validation finished")
    monkeypatch.setattr(_lib, "load", boom)
    monkeypatch.setattr(E, "moments", boom)
    monkeypatch.setattr(E, "_to_device", boom)


@pytest.mark.parametrize("case,match", [
    ("batch", "multiple of num_samples"),
    ("c_mismatch", "C and T must match"),
    ("t_mismatch", "C and T must match"),
    ("t1", "T >= 2"),
    ("c257", "at most 256"),
    ("int", "floating point"),
    ("gt_int", "floating point"),
    ("shape", r"\[S, C, T\]"),
    ("frames", "more frames than draws"),
    ("num_samples", "positive integer"),
])
def test_validation_errors_before_any_gpu_work(no_gpu, case, match):
    x = torch.zeros(20, 104, 1, 600)                                               # 12 000 frames > 10 000 draws
    gt, ns = None, 5
    if case == "batch":
        x = torch.zeros(22, 104, 1, 600)
    elif case == "c_mismatch":
        gt = torch.zeros(10, 105, 600)
    elif case == "t_mismatch":
        gt = torch.zeros(10, 104, 599)
    elif case == "t1":
        x = torch.zeros(10, 104, 1)
    elif case == "c257":
        x = torch.zeros(10, 257, 600)
    elif case == "int":
        x = torch.zeros(10, 104, 600, dtype=torch.int32)
    elif case == "gt_int":
        gt = np.zeros((10, 104, 600), np.int64)
    elif case == "shape":
        x = torch.zeros(10, 104, 2, 600)
    elif case == "frames":
        x = torch.zeros(5, 104, 2000)
    elif case == "num_samples":
        ns = 0
    with pytest.raises(A2PError, match=match):
        E.evaluate_motion(x, gt, num_samples=ns)


def test_missing_keys_raise_before_any_gpu_work(no_gpu, tmp_path):
    with pytest.raises(A2PError, match="neither 'motions'"):
        E.evaluate_results({"gt": np.zeros((5, 104, 600), np.float32)})
    with pytest.raises(A2PError, match="neither 'motions'"):
        E.evaluate_results({"motions": None, "gt": None})
    p = str(tmp_path / "not_a_dict.npy")
    np.save(p, np.zeros(3))
    with pytest.raises(A2PError, match="does not hold a results dict"):
        E.evaluate_results(p)


def test_results_key_fallback(tmp_path):
    a, b = np.ones((5, 4, 1, 8), np.float32), np.zeros((5, 4, 1, 8), np.float32)
    assert E.pick_motion({"motions": a, "gt": b})[0] is a                 # what sample.generate writes
    assert E.pick_motion({"motion": a, "gt": b})[1] is b                  # what eval.py reads
    assert E.pick_motion({"motions": a, "motion": b})[0] is a             # both: the generator's key first
    assert E.pick_motion({"motions": None, "motion": b, "gt": None}) == (b, None)
    from audio2photoreal_amd.sample.generate import save_results
    path = save_results(str(tmp_path), {"motions": a, "audio": None, "gt": None, "lengths": None, "keyframes": None})
    pred, gt = E.pick_motion(E.load_results(path))
    assert np.array_equal(pred, a) and gt is None


def test_cli_arguments():
    args = E.parse_args(["--results", "r.npy"])
    assert (args.results, args.num_samples, args.seed, args.diversity_times, args.json) == ("r.npy", 5, 0, 10_000, None)
    args = E.parse_args(["--results", "r.npy", "--num-samples", "3", "--seed", "7", "--json", "o.json", "--diversity-times", "50"])
    assert (args.num_samples, args.seed, args.json, args.diversity_times) == (3, 7, "o.json", 50)
    for bad in ([], ["--results", "r.npy", "--num-samples", "0"], ["--results", "r.npy", "--seed", "x"],
                ["--results", "r.npy", "--diversity-times", "0"]):
        with pytest.raises(SystemExit):
            E.parse_args(bad)


def test_printed_lines_follow_the_reference_order():
    res = {"cross_var": 0.5, "var_g": 1.25, "var_k": 0.1, "fid_g": 3.0, "fid_k": 4.0}
    assert E.format_lines(res) == ["cross var 0.5", "var_g 1.25", "var_k 0.1", "fid_g 3.0", "fid_k 4.0"]
    assert E.format_lines({**res, "fid_g": None, "fid_k": None}) == ["cross var 0.5", "var_g 1.25", "var_k 0.1"]
    v = 0.1 + 0.2
    assert float(E.format_lines({**res, "var_k": v})[2].split()[-1]) == v     # repr round-trips


def test_exports_are_bound():
    assert {"a2p_eval_moments", "a2p_eval_pair_dist", "a2p_eval_gemm_f64", "a2p_eval_eigh"} <= set(_lib.EXPORTS)
