"""Motion evaluation on the MI355X (csrc/kernels_eval.h, audio2photoreal_amd/evaluate.py): the fp64 moments against numpy
float64, the Jacobi eigensolver against numpy.linalg.eigvalsh, the Frechet distance, diversity, var_k and cross var against the
reference's fixture (tests/golden/golden_eval_v1.npz) and the float64 restatement (tests/eval_restatement.py), determinism,
non-finite input, and the command line end to end on a generated results.npy.  Measured errors go to record(...).

Gates are min(bar of the issue, a few x the measured error); the measured numbers are in the comments."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import eval_restatement as R
from audio2photoreal_amd import evaluate as E
from audio2photoreal_amd._lib import A2PError
from conftest import record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_eval_v1.npz"))


def _rel(got, want):
    return float(np.abs(np.asarray(got) - np.asarray(want)).max() / max(np.abs(np.asarray(want)).max(), 1e-300))


# ------------------------------------------------------------------------------------------------ moments
@pytest.mark.parametrize("C", [104, 256])
@pytest.mark.parametrize("T", [2, 600])
@pytest.mark.parametrize("S", [1, 40])
def test_moments_match_numpy_float64(dev, C, T, S):
    rs = np.random.RandomState(C * 1000 + T + S)
    x = (rs.randn(S, C, T) * rs.uniform(0.1, 3.0, (1, C, 1)) + rs.randn(1, C, 1) * 5).astype(np.float32)
    reps = 5 if S % 5 == 0 else 1
    m = E.moments(torch.from_numpy(x).to(dev), reps=reps)
    mu, cov = R.stats(R.frames(x))
    errs = {"mu": _rel(m["mu"].cpu().numpy(), mu), "cov": _rel(m["cov"].cpu().numpy(), cov)}
    assert torch.equal(m["cov"], m["cov"].T)                                        # symmetric to the bit
    if S * (T - 1) >= 2:
        mu_v, cov_v = R.stats(R.velocities(x))
        errs["mu_v"] = float(np.abs(m["mu_v"].cpu().numpy() - mu_v).max() / np.abs(R.velocities(x)).max())
        errs["cov_v"] = _rel(m["cov_v"].cpu().numpy(), cov_v)
    else:                                                                           # one velocity frame: np.cov's 0 / 0
        assert torch.isnan(m["cov_v"]).all()
    errs["var_k"] = abs(m["var_k"] - R.var_k(x)) / R.var_k(x)
    errs["cross_var"] = abs(m["cross_var"] - R.cross_var(x, reps)) / max(R.cross_var(x, reps), 1e-300) if reps > 1 else 0.0
    if reps == 1:
        assert m["cross_var"] == 0.0
    record(f"eval_moments_C{C}_T{T}_S{S}", **errs)
    assert max(errs.values()) <= 1e-14, errs                                        # bar 1e-12; measured <= 1.2e-15


def test_velocities_never_cross_sequences(dev):
    """Large per-sequence offsets: a delta taken across the boundary of s and s + 1 would be ~1000 and swamp mu_v / cov_v."""
    rs = np.random.RandomState(5)
    S, C, T = 8, 104, 50
    x = (rs.randn(S, C, T) * 0.1 + np.arange(S)[:, None, None] * 1000.0).astype(np.float32)
    m = E.moments(torch.from_numpy(x).to(dev))
    mu_v, cov_v = R.stats(R.velocities(x))
    assert np.abs(m["mu_v"].cpu().numpy()).max() < 0.1
    assert _rel(m["cov_v"].cpu().numpy(), cov_v) <= 1e-12
    assert np.abs(m["mu_v"].cpu().numpy() - mu_v).max() <= 1e-12


def test_fp64_input_gives_the_fp32_bits(dev):
    pred, gt, ns = R.make_case("a")
    a = E.moments(torch.from_numpy(pred).to(dev), reps=ns)
    b = E.moments(torch.from_numpy(pred.astype(np.float64)).to(dev), reps=ns)
    for k in ("mu", "cov", "mu_v", "cov_v"):
        assert torch.equal(a[k], b[k]), k
    assert (a["var_k"], a["cross_var"]) == (b["var_k"], b["cross_var"])


# ------------------------------------------------------------------------------------------------ eigensolver
def _matrix(kind, n, rs):
    x = rs.randn(n, n)
    if kind == "spd":
        return x @ x.T / n + 0.1 * np.eye(n)
    if kind == "rank":
        y = rs.randn(n, max(1, n // 3))
        return y @ y.T
    q, _ = np.linalg.qr(x)                                                          # repeated eigenvalues 1, 2, 3
    return (q * np.tile([1.0, 2.0, 3.0], n)[:n]) @ q.T


@pytest.mark.parametrize("n", [1, 2, 17, 104, 128, 129, 256])
@pytest.mark.parametrize("kind", ["spd", "rank", "repeated"])
def test_jacobi_eigensolver(dev, n, kind):
    a = _matrix(kind, n, np.random.RandomState(n))
    a = 0.5 * (a + a.T)
    w, q, sweeps, off = E.eigh(torch.from_numpy(a).to(dev))
    norm2 = max(np.linalg.norm(a, 2), 1e-300)
    dl = float(np.abs(np.sort(w.cpu().numpy()) - np.linalg.eigvalsh(a)).max() / norm2)
    qh = q.cpu().numpy()
    orth = float(np.abs(qh.T @ qh - np.eye(n)).max())
    recon = float(np.abs((qh * w.cpu().numpy()) @ qh.T - a).max() / norm2)
    record(f"eval_eigh_{kind}_n{n}", sweeps=sweeps, off=off, dlambda=dl, orth=orth, recon=recon)
    # bars 1e-12 (dlambda, orth); measured <= 8.3e-15 / 1.7e-13 / 1.1e-13 (recon), <= 23 sweeps (repeated, n = 256)
    assert sweeps < 40 and dl <= 5e-14 and orth <= 1e-12 and recon <= 1e-12, (sweeps, dl, orth, recon)
    w2, q2, sweeps2, _ = E.eigh(torch.from_numpy(a).to(dev), vectors=False)
    assert q2 is None and sweeps2 == sweeps and torch.equal(w2, w)                 # the vectors do not change the values


def test_eigensolver_refuses_nonfinite_input(dev):
    a = torch.eye(8, dtype=torch.float64, device=dev)
    a[2, 3] = float("nan")
    with pytest.raises(A2PError, match="non-finite"):
        E.eigh(a)


# ------------------------------------------------------------------------------------------------ against the fixture
@pytest.mark.parametrize("name", sorted(R.CASES))
def test_metrics_against_the_reference_fixture(dev, gold, name):
    pred, gt, ns = R.make_case(name)
    res = E.evaluate_motion(torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev), num_samples=ns,
                            diversity_times=R.DIVERSITY_TIMES, seed=R.DIVERSITY_SEED)
    i1, i2 = E.diversity_indices(pred.shape[0] * pred.shape[2], R.DIVERSITY_TIMES, R.DIVERSITY_SEED)
    want = R.evaluate(pred, gt, ns, i1, i2)
    errs = {}
    for k in ("cross_var", "var_k", "var_g"):
        errs[f"{k}_vs_ref"] = abs(res[k] - float(gold[f"{name}/{k}"])) / abs(want[k])
        errs[f"{k}_vs_f64"] = abs(res[k] - want[k]) / abs(want[k])
    for k in ("fid_g", "fid_k"):
        tr = 2.0 * np.trace(R.stats(R.frames(gt) if k == "fid_g" else R.velocities(gt))[1])
        errs[f"{k}_vs_ref"] = abs(res[k] - float(gold[f"{name}/{k}64"])) / tr
        errs[f"{k}_vs_f64"] = abs(res[k] - want[k]) / tr
        errs[f"{k}_abs"] = abs(res[k]) / tr
    record(f"eval_fixture_{name}", **errs, **{k: res[k] for k in E.METRICS})
    for k in ("cross_var", "var_k", "var_g"):
        # bars 1e-5 / 1e-12; measured <= 9.2e-8 (the reference's float32 rounding) / 6.7e-16
        assert errs[f"{k}_vs_ref"] <= 5e-7 and errs[f"{k}_vs_f64"] <= 1e-14, (k, errs)
    for k in ("fid_g", "fid_k"):
        if name in ("a", "b"):
            # bar 1e-9 (trS1 + trS2); measured <= 1.8e-12
            assert errs[f"{k}_vs_ref"] <= 1e-11 and errs[f"{k}_vs_f64"] <= 1e-11, (k, errs)
        elif name == "c":
            # singular gt covariance: its zero eigenvalues come back as +-rounding (~eps ||S||), and their square roots
            # enter tr sqrtm as O(sqrt(eps) ||S||) ~ 1e-8 relative terms at worst, in ours, scipy's and numpy's alike;
            # measured <= 1.8e-10
            assert errs[f"{k}_vs_ref"] <= 1e-9 and errs[f"{k}_vs_f64"] <= 1e-9, (k, errs)
        else:                                                                       # pred == gt
            assert errs[f"{k}_abs"] <= 1e-10, (k, errs)                         # measured <= 6.2e-12


def test_diversity_against_the_fixture(dev, gold):
    pred = R.make_case("a")[0]
    i1, i2 = E.diversity_indices(pred.shape[0] * pred.shape[2], int(gold["diversity_times"]), int(gold["diversity_seed"]))
    assert np.array_equal(i1, gold["a/idx1"]) and np.array_equal(i2, gold["a/idx2"])
    d = E.diversity(torch.from_numpy(pred).to(dev), int(gold["diversity_times"]), int(gold["diversity_seed"])).cpu().numpy()
    err_ref = float(np.abs(d - gold["a/dist"]).max() / np.abs(gold["a/dist"]).max())
    err_f64 = _rel(d, R.pair_distances(pred, i1, i2))
    record("eval_diversity_a", vs_ref_float32=err_ref, vs_f64=err_f64)
    assert err_ref <= 5e-7 and err_f64 <= 1e-13                                     # bar 1e-6; measured 9.0e-8 / 0


def test_two_calls_return_identical_floats(dev):
    pred, gt, ns = R.make_case("b")
    p, g = torch.from_numpy(pred).to(dev), torch.from_numpy(gt).to(dev)
    assert E.evaluate_motion(p, g, num_samples=ns) == E.evaluate_motion(p, g, num_samples=ns)


def test_nonfinite_prediction_raises(dev):
    pred, gt, ns = R.make_case("a")
    p = torch.from_numpy(pred).to(dev)
    p[3, 17, 250] = float("nan")
    with pytest.raises(A2PError, match="pred holds non-finite"):
        E.evaluate_motion(p, torch.from_numpy(gt).to(dev), num_samples=ns)


# ------------------------------------------------------------------------------------------------ end to end
def test_generated_results_through_the_command_line(dev, tmp_path):
    """A synthetic body model, ddim10, 5 repetitions x B=4 x T=600 with a synthetic gt, through _generate_sequences and
    save_results; the command line's five printed numbers equal evaluate_results on the same file and the restatement."""
    from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from audio2photoreal_amd.model_util import create_model_and_diffusion, default_args, load_model
    from audio2photoreal_amd.sample.generate import _generate_sequences, make_inv_transform, save_results
    from audio2photoreal_amd.spec import pose_spec
    from audio2photoreal_amd.synthetic import synthetic_inputs, synthetic_state_dict, synthetic_tensor
    spec = pose_spec()
    B, T, reps = 4, 600, 5
    model, diffusion = create_model_and_diffusion(default_args("pose", timestep_respacing="ddim10"), "test", precision="fp32",
                                                  max_batch=2 * B)
    load_model(model, synthetic_state_dict(spec, 10))
    cfg = ClassifierFreeSampleModel(model.to(dev).eval())
    inp = synthetic_inputs(spec, B, T, 10)
    y = {"cond_embed": inp["cond_embed"], "keyframes": inp["keyframes"], "mask": inp["mask"], "lengths": torch.full((B,), T)}
    stats = {"pose_mean": np.zeros(104), "pose_std": np.ones(104), "code_mean": np.zeros(256), "code_std": np.ones(256),
             "audio_mean": np.zeros(2, np.float32), "audio_std": np.ones(2, np.float32), "audio_std_flat": np.ones(1, np.float32)}
    gt = synthetic_tensor(11, "gt", (B, 104, 1, T))
    args = argparse.Namespace(batch_size=B, curr_seq_length=T, data_format="pose", num_repetitions=reps, guidance_param=2.0,
                              device=dev)
    torch.manual_seed(0)
    res = _generate_sequences(args, {"y": y}, diffusion, cfg, make_inv_transform(stats), gt=gt)
    assert res["motions"].shape == (reps * B, 104, 1, T) and res["gt"].shape == (reps * B, 104, 1, T)
    path = save_results(str(tmp_path), res)
    out = subprocess.run(["timeout", "-k", "10", "300", sys.executable, "-m", "audio2photoreal_amd.evaluate", "--results", path,
                          "--json", str(tmp_path / "m.json")], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stdout.strip().splitlines()
    assert [ln.rsplit(" ", 1)[0] for ln in lines] == ["cross var", "var_g", "var_k", "fid_g", "fid_k"]
    printed = [float(ln.rsplit(" ", 1)[1]) for ln in lines]
    direct = E.evaluate_results(path)
    assert printed == [direct[k] for k in E.METRICS]
    pred = np.asarray(res["motions"])[:, :, 0]
    g = np.asarray(res["gt"])[:, :, 0]
    i1, i2 = E.diversity_indices(pred.shape[0] * T, 10_000, 0)
    want = R.evaluate(pred, g, reps, i1, i2)
    errs = {k: abs(direct[k] - want[k]) / max(abs(want[k]), 1e-300) for k in ("cross_var", "var_g", "var_k")}
    for k in ("fid_g", "fid_k"):
        tr = 2.0 * np.trace(R.stats(R.frames(g) if k == "fid_g" else R.velocities(g))[1])
        errs[k] = abs(direct[k] - want[k]) / tr
    record("eval_end_to_end_pose_ddim10", **{f"err_{k}": v for k, v in errs.items()}, **direct)
    assert max(errs.values()) <= 1e-9, errs
