"""First use of the motion evaluation (audio2photoreal_amd/evaluate.py): how far the fast samplers land from ddim100
(profiles/sampler_quality.json).

Face and body models (trained_like_state_dict: synthetic weights pushed towards trained statistics), fp16, B = 8, T = 600, the
body on fixed keyframes.  A reference set is drawn with ddim100 DDIM (5 repetitions x B = 8: 24 000 frames) and each candidate
set -- ddim100 on a disjoint seed set (the noise floor), ddim20 DDIM, ddim20 dpm++2m, ddim10 DDIM -- is scored against it with
evaluate_motion (the reference set as gt).  The wall time of evaluate_motion is compared with the float64 numpy restatement
(tests/eval_restatement.py) on the same data.

The weights are synthetic: the numbers show that the tool works and give a first ordering of the samplers.  They say nothing
about the quality a trained checkpoint keeps.

    python tests/tools/sampler_quality.py --out profiles/sampler_quality.json
"""
import argparse
import json
import os
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import eval_restatement as R                                                              # noqa: E402
from audio2photoreal_amd import evaluate as E                                            # noqa: E402
from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel              # noqa: E402
from audio2photoreal_amd.model_util import create_gaussian_diffusion, create_model_and_diffusion, default_args, load_model   # noqa: E402
from audio2photoreal_amd.spec import face_spec, pose_spec                                # noqa: E402
from audio2photoreal_amd.synthetic import synthetic_inputs, trained_like_state_dict      # noqa: E402

B, T, REPS = 8, 600, 5
CONFIGS = (("ddim100_floor", "ddim100", "ddim", 1000), ("ddim20", "ddim20", "ddim", 2000), ("ddim20_dpm++2m", "ddim20", "dpm++2m", 2000),
           ("ddim10", "ddim10", "ddim", 3000))


def _model(fmt, dev):
    spec = face_spec() if fmt == "face" else pose_spec()
    m, _ = create_model_and_diffusion(default_args(fmt, timestep_respacing="ddim100"), "test", precision="fp16", max_batch=2 * B)
    load_model(m, trained_like_state_dict(spec, 10))
    inp = synthetic_inputs(spec, B, T, 10)
    y = {"cond_embed": inp["cond_embed"].to(dev), "scale": torch.full((B,), 2.0, device=dev)}
    if spec.is_pose:
        y["keyframes"] = inp["keyframes"].to(dev)                                       # fixed keyframes
        y["mask"] = inp["mask"].to(dev)
    return spec, ClassifierFreeSampleModel(m.to(dev).eval()), y


def _draw(fmt, model, spec, y, respacing, sampler, seed0, dev):
    """[REPS * B, C, T] fp32 on the device: REPS batches, noise from seeds seed0 + r."""
    d = create_gaussian_diffusion(default_args(fmt, timestep_respacing=respacing))
    loop = d.dpm_solver_sample_loop if sampler == "dpm++2m" else d.ddim_sample_loop
    out = []
    for r in range(REPS):
        noise = torch.randn(B, spec.nfeats, 1, T, generator=torch.Generator().manual_seed(seed0 + r)).to(dev)
        with torch.no_grad():
            out.append(loop(model, (B, spec.nfeats, 1, T), noise=noise, clip_denoised=False, model_kwargs={"y": y})[:, :, 0])
    return torch.cat(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    record = {"weights": "SYNTHETIC (audio2photoreal_amd.synthetic.trained_like_state_dict): this shows that the tool "
                         "works and a first ordering; it says nothing about trained checkpoints",
              "shape": {"B": B, "T": T, "repetitions": REPS, "precision": "fp16", "guidance": 2.0, "body": "fixed synthetic keyframes"},
              "reference_set": "ddim100 DDIM, seeds 0..4", "metrics": {}, "eval_wall_s": {}}
    for fmt in ("face", "body"):
        spec, model, y = _model("face" if fmt == "face" else "pose", dev)
        f = "face" if fmt == "face" else "pose"
        ref = _draw(f, model, spec, y, "ddim100", "ddim", 0, dev)
        record["reference_max_abs_sample"] = {**record.get("reference_max_abs_sample", {}), fmt: float(ref.abs().max())}
        rows = {}
        for name, respacing, sampler, seed0 in CONFIGS:
            pred = _draw(f, model, spec, y, respacing, sampler, seed0, dev)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = E.evaluate_motion(pred, ref, num_samples=REPS)
            torch.cuda.synchronize()
            t_gpu = time.perf_counter() - t0
            ph, rh = pred.cpu().numpy(), ref.cpu().numpy()
            t0 = time.perf_counter()
            i1, i2 = E.diversity_indices(ph.shape[0] * T, 10_000, 0)
            cpu = R.evaluate(ph, rh, REPS, i1, i2)
            t_cpu = time.perf_counter() - t0
            diff = max(abs(res[k] - cpu[k]) / max(abs(cpu[k]), 1e-12) for k in E.METRICS)
            rows[name] = {**res, "max_abs_sample": float(pred.abs().max()), "max_rel_diff_vs_cpu_restatement": diff}
            record["eval_wall_s"][f"{fmt}/{name}"] = {"evaluate_motion_gpu": round(t_gpu, 4), "numpy_restatement_cpu": round(t_cpu, 4)}
            print(fmt, name, rows[name], record["eval_wall_s"][f"{fmt}/{name}"], flush=True)
        record["metrics"][fmt] = rows
    print(json.dumps(record, indent=1))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            json.dump(record, fh, indent=1)


if __name__ == "__main__":
    main()
