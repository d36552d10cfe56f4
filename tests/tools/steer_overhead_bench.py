"""What steering costs on the MI355X (profiles/steer_overhead.json).

Body model, 6 layers (synthetic weights), fp16, B = 8, T = 600, a 100-step DDIM loop: `ddim_sample_loop` and
`steered_sample_loop` (2 iterations per step, three constraints with weight on every frame: the most a step can cost) are timed
in alternating rounds, each round one whole loop inside device events, after a warm-up loop of both.  The steer kernel's own
time is that of `a2p_skin_steer` on the same 4800 frames, constraints and iterations -- the launch the step makes, reading its
rows from a buffer instead of the model output -- over `--kernel-calls` back-to-back calls inside device events.  The skeleton
is a synthetic one of the body model's size (160 joints, 104 + 12 parameters).  Prints one JSON object and writes it to `--out`.

    python tests/tools/steer_overhead_bench.py --rounds 3 --out steer_overhead.json
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import skinning_restatement as R                                                         # noqa: E402
from audio2photoreal_amd import skinning as S                                            # noqa: E402
from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel              # noqa: E402
from audio2photoreal_amd.model_util import create_model_and_diffusion, default_args, load_model   # noqa: E402
from audio2photoreal_amd.sample.steer import JointTargets, steered_sample_loop           # noqa: E402
from audio2photoreal_amd.spec import pose_spec                                           # noqa: E402
from audio2photoreal_amd.synthetic import cond_tokens_for_frames, synthetic_state_dict   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-calls", type=int, default=200)
    ap.add_argument("--iterations", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("steer_overhead_bench measures on the MI355X: no GPU found")
    dev = torch.device("cuda:0")
    B, T, layers, J = 8, 600, 6, 160
    m, diff = create_model_and_diffusion(default_args("pose", layers=layers, timestep_respacing="ddim100"), "test", precision="fp16",
                                         max_batch=B)
    load_model(m, synthetic_state_dict(pose_spec(num_layers=layers), 10))
    model = ClassifierFreeSampleModel(m.to(dev).eval())
    g = torch.Generator().manual_seed(10)
    y = {"cond_embed": torch.randn(B, cond_tokens_for_frames(T), m.cond_feature_dim, generator=g).to(dev),
         "scale": torch.full((B,), 2.0, device=dev), "keyframes": torch.randn(B, len(range(T)[::30]), 104, generator=g).to(dev),
         "mask": torch.ones(B, 1, 1, T, dtype=torch.bool, device=dev)}
    noise = torch.randn(B, 104, 1, T, generator=g).to(dev)

    skel = R.make_skeleton(7, J, 16, 4)
    _, scales = R.make_inputs(11, 1)
    sk = S.BodySkeleton.from_arrays(skel["parents"], skel["pre_rotation"], skel["joint_offset"], skel["transform"], skel["transform_offsets"],
                                    104, 12, skel["rest_vertices"], skel["skin_indices"], skel["skin_weights"], lbs_scale=scales[0])
    rs = np.random.RandomState(5)
    mean, std = (rs.randn(104) * 0.1).astype(np.float32), rs.uniform(0.3, 1.5, 104).astype(np.float32)
    other = R.joint_positions(skel, (rs.randn(B * T, 104) * 0.6).astype(np.float32), scales).reshape(B, T, J, 3)
    jt = JointTargets(sk, B, T)
    jt.aim(J // 3, slice(0, T), other[:, :, J // 3] + 1.0).reach(J - 1, slice(0, T), other[:, :, J - 1]).reach(J // 2, slice(0, T), other[:, :, J // 2])
    host = jt.constraints()
    cons = S.JointConstraints(host.joints, host.kinds, host.axes, host.targets.to(dev), host.weights.to(dev), sk.J)   # resident: no copy per call
    mean_d, std_d = torch.from_numpy(mean).to(dev), torch.from_numpy(std).to(dev)

    variants = {
        "plain": lambda: diff.ddim_sample_loop(model, (B, 104, 1, T), noise=noise, clip_denoised=False, model_kwargs={"y": y}),
        "steered": lambda: steered_sample_loop(diff, model, y, sk, mean, std, jt, noise, iterations=a.iterations),
    }
    with torch.no_grad():
        for fn in variants.values():
            fn()
        torch.cuda.synchronize(dev)
        loop_ms = {k: [] for k in variants}
        for _ in range(a.rounds):
            for name, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn()
                e1.record()
                e1.synchronize()
                loop_ms[name].append(round(e0.elapsed_time(e1), 2))
        z = variants["plain"]()[:, :, 0].permute(0, 2, 1).reshape(B * T, 104).contiguous()
        for _ in range(10):
            sk.solve_ik(z, cons, iterations=a.iterations, mean=mean_d, std=std_d)
        torch.cuda.synchronize(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.kernel_calls):
            sk.solve_ik(z, cons, iterations=a.iterations, mean=mean_d, std=std_d)
        e1.record()
        e1.synchronize()
        kernel_ms = e0.elapsed_time(e1) / a.kernel_calls
    mean_ms = {k: sum(v) / len(v) for k, v in loop_ms.items()}
    out = {"what": f"body {layers}L fp16 (synthetic weights), B={B}, T={T}, 100-step ddim loop: ddim_sample_loop vs steered_sample_loop "
                   f"({a.iterations} iterations per step, 3 constraints weighted on every frame, synthetic {J}-joint skeleton); {a.rounds} "
                   f"rounds, alternating, one loop per device-event window; steer kernel: a2p_skin_steer on the same {B * T} frames, "
                   f"{a.kernel_calls} back-to-back calls per window (includes the host's call overhead)",
           "loop_ms": loop_ms, "mean_loop_ms": {k: round(v, 2) for k, v in mean_ms.items()},
           "steered_over_plain": round(mean_ms["steered"] / mean_ms["plain"], 4),
           "steer_call_ms": round(kernel_ms, 4), "steer_calls_per_loop": 100,
           "steer_share_of_steered_loop": round(100 * kernel_ms / mean_ms["steered"], 4)}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
