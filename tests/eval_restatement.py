"""Inputs and a float64 numpy restatement of the motion-evaluation formulas (audio2photoreal_amd/evaluate.py, the reference's
utils/eval.py).  Test infrastructure: shared by tests/golden/make_golden_eval.py, tests/test_evaluate_cpu.py and
tests/test_evaluate_hip.py.  The inputs are regenerated from np.random.RandomState streams, so the fixture stores only seeds.

Every input value is a multiple of 2^-12 below 2^8 in magnitude: float32 holds it, and the frame-to-frame differences the
reference takes in float32 are exact, so the velocity statistics of reference and product see the same numbers."""
import numpy as np

# name: (seed, C, T, num_samples, B); (c) has constant gt channels (singular gt covariances), (d) pred == gt
CASES = {
    "a": dict(seed=101, C=104, T=600, num_samples=5, B=4),
    "b": dict(seed=202, C=256, T=600, num_samples=5, B=4),
    "c": dict(seed=303, C=104, T=600, num_samples=5, B=4, const_channels=(3, 17, 40, 41, 99)),
    "d": dict(seed=404, C=104, T=600, num_samples=5, B=4, same=True),
}
DIVERSITY_SEED = 0
DIVERSITY_TIMES = 10_000
Q = 4096.0


def _motion(rs, S, C, T, scale):
    """Correlated, temporally smooth [S, C, T] float32 on the 2^-12 grid: per-channel offsets, a random walk and white noise
    through a random channel mixing."""
    mix = rs.randn(C, C) / np.sqrt(C)
    walk = np.cumsum(rs.randn(S, C, T) * 0.05, axis=-1)
    noise = rs.randn(S, C, T) * 0.3
    x = np.einsum("dc,sct->sdt", mix, walk + noise) * scale + rs.randn(1, C, 1) * 2.0
    return (np.round(np.clip(x, -200, 200) * Q) / Q).astype(np.float32)


def make_case(name):
    """(pred, gt, num_samples) of a fixture case: rep-major [num_samples * B, C, T] float32."""
    c = CASES[name]
    rs = np.random.RandomState(c["seed"])
    S = c["num_samples"] * c["B"]
    pred = _motion(rs, S, c["C"], c["T"], 1.0)
    gt = pred.copy() if c.get("same") else _motion(rs, S, c["C"], c["T"], 0.8)
    for ch in c.get("const_channels", ()):
        gt[:, ch, :] = np.float32(round(1.5 + 0.25 * ch, 2))
    return pred, gt, c["num_samples"]


# ------------------------------------------------------------------------------------------------ float64 restatement
def frames(x):
    """[S, C, T] -> [S T, C] float64 (frame s T + t)."""
    x = np.asarray(x, np.float64)
    return x.transpose(0, 2, 1).reshape(-1, x.shape[1])


def velocities(x):
    """[S, C, T] -> [S (T - 1), C] float64 in-sequence differences."""
    x = np.asarray(x, np.float64)
    d = x[..., 1:] - x[..., :-1]
    return d.transpose(0, 2, 1).reshape(-1, x.shape[1])


def stats(rows):
    """(mean, centred covariance / (N - 1)) of [N, C] float64 rows."""
    mu = rows.mean(axis=0)
    d = rows - mu
    return mu, d.T @ d / (rows.shape[0] - 1)


def sqrt_trace(cov1, cov2):
    """tr sqrtm(cov1 cov2) for PSD matrices as sum sqrt(lambda(A cov2 A)), A = cov1^(1/2)."""
    w, q = np.linalg.eigh(cov1)
    a = (q * np.sqrt(np.maximum(w, 0.0))) @ q.T
    lam = np.linalg.eigvalsh(a @ cov2 @ a)
    return float(np.sum(np.sqrt(np.maximum(lam, 0.0))))


def frechet(mu1, cov1, mu2, cov2):
    d = mu1 - mu2
    return float(d @ d + np.trace(cov1) + np.trace(cov2) - 2.0 * sqrt_trace(cov1, cov2))


def cross_var(pred, num_samples):
    x = np.asarray(pred, np.float64).reshape(num_samples, -1)
    return float(x.var(axis=0).mean())


def var_k(pred):
    return float(np.asarray(pred, np.float64).var(axis=-1).mean())


def pair_distances(pred, i1, i2):
    f = frames(pred)
    return np.sqrt(((f[i1] - f[i2]) ** 2).sum(axis=1))


def evaluate(pred, gt, num_samples, i1, i2):
    """The five metrics in float64, with the diversity pairs given."""
    pm, pc = stats(frames(pred))
    gm, gc = stats(frames(gt))
    pmv, pcv = stats(velocities(pred))
    gmv, gcv = stats(velocities(gt))
    return {"cross_var": cross_var(pred, num_samples), "var_g": float(pair_distances(pred, i1, i2).mean()), "var_k": var_k(pred),
            "fid_g": frechet(gm, gc, pm, pc), "fid_k": frechet(gmv, gcv, pmv, pcv)}
