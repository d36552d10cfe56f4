"""What separate guidance of audio and keyframes costs per sampling step (profiles/dual_guidance_timing.json).

Body model (pose_spec(), synthetic weights), B = 16, T = 600, fp16, one fused DDIM step (a2p_sample_step) per measurement, timed
with device events; y["guidance"] absent (joint), "audio" and "dual" ALTERNATED step by step, so that clock and load drift hit the
three alike; median, min and max of --steps measurements each after --warmup rounds.  The combine kernel's own time comes from
the library's dispatch-packet timer (a2p_kernel_timing, A2P_KERNEL_GUIDE_COMBINE) in a second pass.

    python scratch/dual_guidance_time.py [--steps 30] [--warmup 5] [--out profiles/dual_guidance_timing.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from audio2photoreal_amd import _lib  # noqa: E402
from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel  # noqa: E402
from audio2photoreal_amd.model_util import create_gaussian_diffusion, create_model_and_diffusion, default_args, load_model  # noqa: E402
from audio2photoreal_amd.spec import pose_spec  # noqa: E402
from audio2photoreal_amd.synthetic import synthetic_inputs, synthetic_state_dict  # noqa: E402

B, T, SEED = 16, 600, 10


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="fp16")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dual_guidance_timing.json"))
    a = ap.parse_args()
    assert a.steps >= 20, "median of at least 20"
    dev = torch.device("cuda:0")
    spec = pose_spec()
    model, _ = create_model_and_diffusion(default_args("pose", timestep_respacing="ddim100"), "test", precision=a.precision,
                                          max_batch=(3 * B + 1) // 2)
    load_model(model, synthetic_state_dict(spec, SEED))
    cfg = ClassifierFreeSampleModel(model.to(dev).eval())
    diff = create_gaussian_diffusion(default_args("pose", timestep_respacing="ddim100"))
    inp = synthetic_inputs(spec, B, T, SEED)
    base = {k: inp[k].to(dev) for k in ("cond_embed", "keyframes", "mask")}
    base["scale"] = torch.full((B,), 2.0, device=dev)
    ys = {"joint": dict(base), "audio": {**base, "guidance": "audio"},
          "dual": {**base, "guidance": "dual", "scale_keyframes": torch.full((B,), 1.5, device=dev)}}
    x = inp["x_T"].to(dev)
    tab, tmap = diff._tables(dev), diff._timestep_map_tensor(dev)
    t_idx = torch.full((B,), 57, dtype=torch.int64, device=dev)

    def step(mode):
        return cfg.a2p_sample_step(_lib.SAMPLER_DDIM, x, t_idx, tmap, tab, ys[mode], None, 0.0, False)

    for _ in range(a.warmup):
        for mode in ys:
            step(mode)
    torch.cuda.synchronize(dev)
    ms = {mode: [] for mode in ys}
    for _ in range(a.steps):
        for mode in ys:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            step(mode)
            e1.record()
            e1.synchronize()
            ms[mode].append(e0.elapsed_time(e1))
    model.check_finite()

    lib = model._lib()
    combine = {}
    for mode in ("audio", "dual"):
        _lib.check(lib.a2p_kernel_timing(model._ctx, _lib.KERNEL_GUIDE_COMBINE, 1), "a2p_kernel_timing")
        for _ in range(a.steps):
            step(mode)
        tot, n = C.c_double(0), C.c_int64(0)
        _lib.check(lib.a2p_kernel_time_ms(model._ctx, C.byref(tot), C.byref(n)), "a2p_kernel_time_ms")
        _lib.check(lib.a2p_kernel_timing(model._ctx, _lib.KERNEL_GUIDE_COMBINE, 0), "a2p_kernel_timing")
        combine[mode] = {"launches": int(n.value), "mean_us": 1e3 * tot.value / max(1, n.value)}

    out = {"config": {"model": "pose", "B": B, "T": T, "precision": a.precision, "sampler": "ddim", "steps": a.steps, "warmup": a.warmup,
                      "device": torch.cuda.get_device_name(dev)},
           "ms_per_step": {m: {"median": statistics.median(v), "min": min(v), "max": max(v)} for m, v in ms.items()},
           "combine_kernel": combine}
    med = out["ms_per_step"]
    out["ratio_to_joint"] = {m: med[m]["median"] / med["joint"]["median"] for m in ("audio", "dual")}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
    print(json.dumps(out, sort_keys=True))


if __name__ == "__main__":
    main()
