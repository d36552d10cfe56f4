"""Steps per second of the fused tokenizer training step (a2p_vq_train_step through TokenizerTrainer.step) and of the fp32
torch-autograd restatement of the same step (tests/vq_train_restatement.py moved to the GPU, torch.optim.AdamW, EMA in torch ops)
on the same MI355X, at the reference's settings: B = 64, T = 20, spec shapes (104 channels, latent 64, 1024 codes, depth 4).

Method: warm-up steps, then REPEATS timed regions of STEPS steps each with a stream synchronisation on both sides, median of the
repeats.  Writes profiles/vq_train_timing.json.  A record, not a gate.

    python tests/tools/vq_train_timing.py [--out profiles/vq_train_timing.json]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import vq_train_restatement as VT  # noqa: E402
from audio2photoreal_amd.spec import TokenizerSpec  # noqa: E402
from audio2photoreal_amd.synthetic import synthetic_tokenizer_encoder_state_dict, synthetic_tokenizer_state_dict  # noqa: E402
from audio2photoreal_amd.train import tokenizer as TK  # noqa: E402

B, T, WARMUP, STEPS, REPEATS = 64, 20, 20, 50, 7
HP = {"commit": 0.02, "loss_vel": 0.0, "weight_decay": 0.0, "lr": 2e-4}        # the README command's settings


def timed(fn):
    for _ in range(WARMUP):
        fn()
    out = []
    for _ in range(REPEATS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(STEPS):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / STEPS)
    return statistics.median(out), min(out), max(out)


def torch_step_fn(sd, spec, x):
    """The autograd restatement in fp32 on the device with torch's own AdamW."""
    dev = x.device
    state = VT.make_state(sd, spec.residual_depth, dtype=torch.float32)
    P = {k: v.to(dev).requires_grad_(VT.trainable(k)) for k, v in state["params"].items()}
    books = {n: [t.to(dev) for t in state[n]] for n in ("embed", "embed_avg", "cluster_size")}
    opt = torch.optim.AdamW([p for k, p in P.items() if VT.trainable(k)], lr=HP["lr"], betas=(0.9, 0.99), weight_decay=HP["weight_decay"])

    def step():
        out = VT._forward_autograd(P, books["embed"], x, HP)
        opt.zero_grad(set_to_none=True)
        out["loss"].backward()
        opt.step()
        with torch.no_grad():
            new = VT.ema(books, out["tokens"], out["residuals"], HP)
            for n in new:
                books[n] = new[n]
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(HERE)), "profiles", "vq_train_timing.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs the MI355X"
    spec = TokenizerSpec()
    sd = {**synthetic_tokenizer_state_dict(spec, 10), **synthetic_tokenizer_encoder_state_dict(spec, 10)}
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((B, T, spec.n_vertices)).astype(np.float32)).cuda()
    tr = TK.TokenizerTrainer(spec, lr=HP["lr"], weight_decay=HP["weight_decay"], commit=HP["commit"], loss_vel=HP["loss_vel"],
                             warm_up_iter=0, milestones=[10 ** 9])
    tr.load_net(sd, inited=True, strict=False)
    fused = timed(lambda: tr.step(x))
    losses = tr.losses()
    eager = timed(torch_step_fn(sd, spec, x))
    res = {"device": torch.cuda.get_device_name(0), "shape": {"B": B, "T": T, "n_vertices": spec.n_vertices, "latent": spec.latent_dim,
                                                             "categories": spec.categories, "depth": spec.residual_depth},
           "method": f"{WARMUP} warm-up steps, {REPEATS} x {STEPS} steps between stream synchronisations, median",
           "fused_step_ms": {"median": fused[0] * 1e3, "min": fused[1] * 1e3, "max": fused[2] * 1e3},
           "torch_autograd_fp32_step_ms": {"median": eager[0] * 1e3, "min": eager[1] * 1e3, "max": eager[2] * 1e3},
           "fused_steps_per_s": 1.0 / fused[0], "torch_autograd_steps_per_s": 1.0 / eager[0], "speedup": eager[0] / fused[0],
           "fused_mean_loss_over_timed_steps": losses["loss"]}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
