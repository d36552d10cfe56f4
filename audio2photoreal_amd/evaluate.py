"""Motion evaluation on the MI355X: the reference's quality yardstick (utils/eval.py) -- cross-repetition variance, static and
kinematic diversity, static and kinematic Frechet distance -- computed in fp64 HIP kernels (csrc/kernels_eval.h) straight from
the tensors the samplers return, or from a saved results.npy.

    python -m audio2photoreal_amd.evaluate --results results.npy [--num-samples 5] [--seed 0] [--json out.json]

Differences from the reference script (INTEGRATION.md "Evaluating samples"):
  - C and T come from the input (eval.py hard-codes 104 x 600); C <= 256, T >= 2;
  - every statistic is fp64; the reference takes np.var / linalg.norm of float32 arrays, so the two agree within float32 rounding;
  - the diversity draw uses np.random.RandomState(seed), equal to the reference's after np.random.seed(seed);
  - the Frechet distance takes tr sqrtm(S1 S2) as sum sqrt(max(lambda, 0)) of A S2 A with A = S1^(1/2) from a symmetric
    eigensolver: always finite for covariances, so the reference's eps-on-the-diagonal retry never applies;
  - results.npy may hold the key "motions" (what sample.generate writes) or "motion" (what eval.py reads).
"""
from __future__ import annotations

import argparse
import ctypes
import json
import sys
from typing import Optional

import numpy as np
import torch

from . import _lib
from ._lib import A2PError

METRICS = ("cross_var", "var_g", "var_k", "fid_g", "fid_k")
_LABELS = {"cross_var": "cross var", "var_g": "var_g", "var_k": "var_k", "fid_g": "fid_g", "fid_k": "fid_k"}


# ------------------------------------------------------------------------------------------------ host validation
def _check_motion(x, name: str):
    """Shape / dtype checks of a motion batch on the host: returns (S, C, T).  [S, C, T] or [S, C, 1, T], floating point."""
    if not (torch.is_tensor(x) or isinstance(x, np.ndarray)):
        raise A2PError(f"{name} must be a tensor or an ndarray (got {type(x).__name__})")
    floating = x.is_floating_point() if torch.is_tensor(x) else np.issubdtype(x.dtype, np.floating)
    if not floating:
        raise A2PError(f"{name} must be floating point (got {x.dtype})")
    shape = tuple(x.shape)
    if len(shape) == 4:
        if shape[2] != 1:
            raise A2PError(f"{name} must be [S, C, T] or [S, C, 1, T] (got {list(shape)})")
        shape = (shape[0], shape[1], shape[3])
    if len(shape) != 3:
        raise A2PError(f"{name} must be [S, C, T] or [S, C, 1, T] (got {list(shape)})")
    S, C, T = shape
    if S < 1 or C < 1:
        raise A2PError(f"{name} is empty ({list(x.shape)})")
    if T < 2:
        raise A2PError(f"{name} needs T >= 2 frames for velocities (got T={T})")
    if C > _lib.EVAL_MAX_CHANNELS:
        raise A2PError(f"{name} has C={C} channels; the evaluation kernels take at most {_lib.EVAL_MAX_CHANNELS}")
    return S, C, T


def _to_device(x, name: str):
    """(device tensor [S, C, T] fp32 or fp64 contiguous, S, C, T).  fp64 stays fp64 (un-normalised results are float64);
    16-bit inputs are widened to fp32."""
    S, C, T = _check_motion(x, name)
    t = x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    if t.dtype not in (torch.float32, torch.float64):
        t = t.to(torch.float32)
    if not t.is_cuda:
        if not torch.cuda.is_available():
            raise A2PError(f"{name}: evaluation runs on the MI355X; there is no CPU implementation")
        t = t.to("cuda")
    return t.reshape(S, C, T).contiguous(), S, C, T


def _raise_nonfinite(flag, name: str):
    v = int(flag.item())
    if v & 1:
        raise A2PError(f"{name} holds non-finite values (nan / inf): its statistics are undefined")
    if v & 2:
        raise A2PError(f"{name}: a diversity index is outside the frames")


# ------------------------------------------------------------------------------------------------ device statistics
def moments(x, name: str = "motion", reps: int = 0) -> dict:
    """Every statistic of one batch [S, C(, 1), T]: fp64 device tensors mu, cov (over the S T frames) and mu_v, cov_v (over the
    S (T - 1) in-sequence velocities), and the host floats var_k (mean over (s, c) of the variance along T) and cross_var
    (reps > 0: mean over the elements of one repetition of the variance across the reps repetitions; else None)."""
    xt, S, C, T = _to_device(x, name)
    if reps and S % reps:
        raise A2PError(f"{name}: {S} sequences are not a multiple of {reps} repetitions")
    dev = xt.device
    f64 = dict(dtype=torch.float64, device=dev)
    out = {"mu": torch.empty(C, **f64), "cov": torch.empty(C, C, **f64), "mu_v": torch.empty(C, **f64), "cov_v": torch.empty(C, C, **f64)}
    sums = torch.empty(2, **f64)
    ws = torch.empty(_lib.EVAL_NSPLIT * C * C + C + _lib.EVAL_XV_PARTIALS, **f64)   # A2P_EVAL_MOMENTS_WS_DOUBLES(C)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    lib = _lib.load()
    with _lib.on_device_of(xt):
        _lib.check(lib.a2p_eval_moments(_lib.ptr(xt), int(xt.dtype == torch.float64), S, C, T, reps, _lib.ptr(out["mu"]),
                                        _lib.ptr(out["cov"]), _lib.ptr(out["mu_v"]), _lib.ptr(out["cov_v"]), _lib.ptr(sums),
                                        _lib.ptr(ws), _lib.ptr(flag), _lib.current_stream(dev)), "a2p_eval_moments")
    _raise_nonfinite(flag, name)
    s = sums.cpu().numpy()
    out["var_k"] = float(s[0] / (S * C))
    out["cross_var"] = float(s[1] / ((S // reps) * C * T)) if reps else None
    return out


def activation_statistics(motion):
    """(mu [C], cov [C, C]) fp64 device tensors over the frames of `motion` [S, C(, 1), T]: eval.py's
    calculate_activation_statistics on transpose(0, 1, 3, 2).reshape(-1, C) (np.cov's N - 1 normalisation)."""
    m = moments(motion, "motion")
    return m["mu"], m["cov"]


def eigh(a, vectors: bool = True):
    """Symmetric eigendecomposition of an fp64 device matrix [n, n] (n <= 256) by the HIP Jacobi solver:
    (w [n] unsorted, q [n, n] or None, sweeps, final off-diagonal norm).  A2PError when it does not converge or a is not finite."""
    if not torch.is_tensor(a) or a.dim() != 2 or a.shape[0] != a.shape[1] or a.dtype != torch.float64:
        raise A2PError("eigh takes a square fp64 tensor")
    n = int(a.shape[0])
    if not 1 <= n <= _lib.EVAL_MAX_CHANNELS:
        raise A2PError(f"eigh: n={n} outside [1, {_lib.EVAL_MAX_CHANNELS}]")
    _lib.require_gpu_tensor(a, "a")
    a = a.contiguous()
    f64 = dict(dtype=torch.float64, device=a.device)
    w = torch.empty(n, **f64)
    q = torch.empty(n, n, **f64) if vectors else None
    m = n + (n & 1)
    ws = torch.empty(m * m + 2, **f64)                                              # A2P_EVAL_EIGH_WS_DOUBLES(n)
    sweeps, off = ctypes.c_int32(0), ctypes.c_double(0.0)
    with _lib.on_device_of(a):
        _lib.check(_lib.load().a2p_eval_eigh(_lib.ptr(a), n, _lib.ptr(w), _lib.ptr(q), _lib.ptr(ws), ctypes.byref(sweeps),
                                             ctypes.byref(off), _lib.current_stream(a.device)), "a2p_eval_eigh")
    return w, q, int(sweeps.value), float(off.value)


def _gemm(a, b, d=None, b_t: bool = False):
    """c = a diag(d) op(b) for n x n fp64 device matrices (op = transpose when b_t)."""
    n = int(a.shape[0])
    c = torch.empty(n, n, dtype=torch.float64, device=a.device)
    brs, bcs = (1, n) if b_t else (n, 1)
    with _lib.on_device_of(a):
        _lib.check(_lib.load().a2p_eval_gemm_f64(n, _lib.ptr(a), n, 1, _lib.ptr(d), _lib.ptr(b), brs, bcs, _lib.ptr(c),
                                                 _lib.current_stream(a.device)), "a2p_eval_gemm_f64")
    return c


def sqrt_trace_product(cov1, cov2):
    """tr sqrtm(cov1 cov2) for positive semi-definite fp64 device matrices: sum sqrt(max(lambda, 0)) over the eigenvalues of
    A cov2 A, A = cov1^(1/2) = Q diag(sqrt(max(lambda1, 0))) Q^T.  Returns (value, {"sweeps": (..), "off": (..)})."""
    w1, q1, sw1, off1 = eigh(cov1, vectors=True)
    root = torch.sqrt(torch.clamp(w1, min=0.0))
    a = _gemm(q1, q1, d=root, b_t=True)
    m = _gemm(_gemm(a, cov2), a)
    w2, _, sw2, off2 = eigh(m, vectors=False)
    lam = w2.cpu().numpy()
    return float(np.sum(np.sqrt(np.maximum(lam, 0.0)))), {"sweeps": (sw1, sw2), "off": (off1, off2)}


def frechet_distance(mu1, cov1, mu2, cov2) -> float:
    """|mu1 - mu2|^2 + tr cov1 + tr cov2 - 2 tr sqrtm(cov1 cov2) (eval.py calculate_frechet_distance) on fp64 device tensors.
    The matrix work runs in HIP; the final handful of scalars (|dmu|^2, the traces) are combined on the host."""
    if tuple(mu1.shape) != tuple(mu2.shape):
        raise A2PError("Training and test mean vectors have different lengths")
    if tuple(cov1.shape) != tuple(cov2.shape) or cov1.dim() != 2 or cov1.shape[0] != mu1.shape[0]:
        raise A2PError("Training and test covariances have different dimensions")
    cov1, cov2 = cov1.to(torch.float64), cov2.to(torch.float64)
    tr_covmean, _ = sqrt_trace_product(cov1, cov2)
    d = mu1.double().cpu().numpy() - mu2.double().cpu().numpy()
    tr1 = float(np.sum(np.diag(cov1.cpu().numpy())))
    tr2 = float(np.sum(np.diag(cov2.cpu().numpy())))
    return float(d.dot(d)) + tr1 + tr2 - 2.0 * tr_covmean


def diversity_indices(num_frames: int, diversity_times: int = 10_000, seed: Optional[int] = None):
    """The two index draws of eval.py calculate_diversity, in its order, from np.random.RandomState(seed): with seed=s they
    equal the reference's after np.random.seed(s).  Needs num_frames > diversity_times, as the reference asserts."""
    if not num_frames > diversity_times:
        raise A2PError(f"diversity needs more frames than draws (frames={num_frames}, diversity_times={diversity_times})")
    rs = np.random.RandomState(seed)
    first = rs.choice(num_frames, diversity_times, replace=False)
    second = rs.choice(num_frames, diversity_times, replace=False)
    return first.astype(np.int64), second.astype(np.int64)


def diversity(motion, diversity_times: int = 10_000, seed: Optional[int] = None):
    """fp64 device tensor [diversity_times]: L2 distances of random frame pairs of `motion` [S, C(, 1), T] (eval.py
    calculate_diversity; frame f = motion[f // T, :, f % T]).  Its mean is var_g."""
    S, C, T = _check_motion(motion, "motion")
    i1, i2 = diversity_indices(S * T, diversity_times, seed)
    xt, S, C, T = _to_device(motion, "motion")
    dev = xt.device
    d1, d2 = torch.from_numpy(i1).to(dev), torch.from_numpy(i2).to(dev)
    out = torch.empty(diversity_times, dtype=torch.float64, device=dev)
    flag = torch.zeros(1, dtype=torch.int32, device=dev)
    with _lib.on_device_of(xt):
        _lib.check(_lib.load().a2p_eval_pair_dist(_lib.ptr(xt), int(xt.dtype == torch.float64), S, C, T, _lib.ptr(d1), _lib.ptr(d2),
                                                  diversity_times, _lib.ptr(out), _lib.ptr(flag), _lib.current_stream(dev)),
                   "a2p_eval_pair_dist")
    _raise_nonfinite(flag, "motion")
    return out


# ------------------------------------------------------------------------------------------------ the five metrics
def _validate(pred, gt, num_samples, diversity_times):
    if isinstance(num_samples, bool) or not isinstance(num_samples, (int, np.integer)) or num_samples < 1:
        raise A2PError(f"num_samples must be a positive integer (got {num_samples!r})")
    S, C, T = _check_motion(pred, "pred")
    if S % num_samples:
        raise A2PError(f"pred holds {S} sequences, not a multiple of num_samples={num_samples} (rep-major [num_samples * B, C, T])")
    if not S * T > diversity_times:
        raise A2PError(f"diversity needs more frames than draws (frames={S * T}, diversity_times={diversity_times})")
    if gt is not None:
        Sg, Cg, Tg = _check_motion(gt, "gt")
        if (Cg, Tg) != (C, T):
            raise A2PError(f"gt is [{Sg}, {Cg}, {Tg}] but pred is [{S}, {C}, {T}]: C and T must match")
        if S * (T - 1) < 2 or Sg * (Tg - 1) < 2:
            raise A2PError("fid_k needs at least two velocity frames in pred and in gt")


def evaluate_motion(pred, gt=None, num_samples: int = 5, diversity_times: int = 10_000, seed: Optional[int] = 0) -> dict:
    """eval.py main on tensors: pred is rep-major [num_samples * B, C, (1,) T] as _generate_sequences concatenates it.
    Returns {"cross_var", "var_g", "var_k", "fid_g", "fid_k"} as Python floats (fid_* None without gt).  Every input check
    happens on the host before any GPU work."""
    _validate(pred, gt, num_samples, diversity_times)
    p = moments(pred, "pred", reps=num_samples)
    res = {"cross_var": p["cross_var"], "var_k": p["var_k"], "fid_g": None, "fid_k": None}
    res["var_g"] = float(diversity(pred, diversity_times, seed).mean().item())
    if gt is not None:
        g = moments(gt, "gt")
        res["fid_g"] = frechet_distance(g["mu"], g["cov"], p["mu"], p["cov"])       # eval.py's (gt, pred) order
        res["fid_k"] = frechet_distance(g["mu_v"], g["cov_v"], p["mu_v"], p["cov_v"])
    return {k: res[k] for k in METRICS}


def load_results(path_or_dict) -> dict:
    """The results dict of a results.npy path (np.save of a dict, as sample.generate.save_results writes it), or the dict."""
    if isinstance(path_or_dict, dict):
        return path_or_dict
    obj = np.load(path_or_dict, allow_pickle=True)
    if obj.shape != () or not isinstance(obj.item(), dict):
        raise A2PError(f"{path_or_dict} does not hold a results dict")
    return obj.item()


def pick_motion(results: dict):
    """(pred, gt or None) of a results dict: the prediction under "motions" (sample.generate) or "motion" (eval.py)."""
    for key in ("motions", "motion"):
        if results.get(key) is not None:
            return results[key], results.get("gt")
    raise A2PError(f"the results hold neither 'motions' (sample.generate) nor 'motion' (eval.py); keys: {sorted(results)}")


def evaluate_results(path_or_dict, num_samples: int = 5, diversity_times: int = 10_000, seed: Optional[int] = 0) -> dict:
    """evaluate_motion on a results.npy (or its dict): the prediction under "motions" or "motion", the ground truth under "gt"
    (absent or None: no fid_g / fid_k)."""
    pred, gt = pick_motion(load_results(path_or_dict))
    return evaluate_motion(pred, gt, num_samples=num_samples, diversity_times=diversity_times, seed=seed)


def format_lines(res: dict):
    """The reference's printed lines in its order (cross var, var_g, var_k, fid_g, fid_k), for the metrics computed;
    repr() round-trips every float."""
    return [f"{_LABELS[k]} {res[k]!r}" for k in METRICS if res[k] is not None]


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m audio2photoreal_amd.evaluate",
                                 description="Quality metrics of generated motion (the reference's utils/eval.py) on the MI355X.")
    ap.add_argument("--results", required=True, help="results.npy written by sample.generate (keys motions|motion, gt)")
    ap.add_argument("--num-samples", type=int, default=5, help="repetitions in the rep-major batch (default 5)")
    ap.add_argument("--seed", type=int, default=0, help="seed of the diversity draw (default 0)")
    ap.add_argument("--diversity-times", type=int, default=10_000, help="frame pairs of the diversity draw (default 10000)")
    ap.add_argument("--json", default=None, help="also write the metrics to this JSON file")
    return ap


def parse_args(argv=None):
    ap = build_parser()
    args = ap.parse_args(argv)
    if args.num_samples < 1:
        ap.error("--num-samples must be >= 1")
    if args.diversity_times < 1:
        ap.error("--diversity-times must be >= 1")
    return args


def main(argv=None) -> int:
    args = parse_args(argv)
    res = evaluate_results(args.results, num_samples=args.num_samples, diversity_times=args.diversity_times, seed=args.seed)
    for line in format_lines(res):
        print(line)
    if res["fid_g"] is None:
        print("no gt in the results: fid_g and fid_k skipped", file=sys.stderr)
    if args.json:
        with open(args.json, "w") as f:
            json.dump({"results": args.results, "num_samples": args.num_samples, "seed": args.seed,
                       "diversity_times": args.diversity_times, **res}, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
