"""DPM-Solver++(2M) on the MI355X: one fused multistep step against one plain DDIM step, and a clip end to end
(profiles/multistep_step.json).

1. Face model, 8 layers (synthetic weights), fp16, B = 8, T = 600, ddim100 tables, the step at t = 50: `a2p_sample_step` (DDIM,
   eta = 0) and `a2p_sample_step_multistep` (with history: the second-order update) are timed in alternating rounds of `--steps`
   calls each, with device events around every round, after a warm-up of both.
2. `generate_from_recording` at the demo's shape (face and body, 8 layers each, fp16, 20 s recording, `--reps` repetitions,
   synthetic weights) with face and body diffusions at ddim100 + sampler="ddim" against ddim20 + sampler="dpm++2m", in s/clip
   (wall clock around the call, after one warm-up call of each), alternating for `--clips` clips each.

Prints one JSON object and writes it to `--out` when given.

    python tests/tools/multistep_step_bench.py --rounds 5 --steps 40 --clips 3 --out multistep_step.json
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from audio2photoreal_amd import _lib                                                    # noqa: E402
from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel              # noqa: E402
from audio2photoreal_amd.model_util import create_gaussian_diffusion, create_model_and_diffusion, default_args, load_model   # noqa: E402
from audio2photoreal_amd.spec import face_spec                                           # noqa: E402
from audio2photoreal_amd.synthetic import cond_tokens_for_frames, synthetic_state_dict   # noqa: E402


def step_timing(dev, rounds, steps, warmup):
    B, T, layers = 8, 600, 8
    spec = face_spec(num_layers=layers)
    m, diff = create_model_and_diffusion(default_args("face", layers=layers, timestep_respacing="ddim100"), "test", precision="fp16",
                                         max_batch=B)
    load_model(m, synthetic_state_dict(spec, 10))
    model = ClassifierFreeSampleModel(m.to(dev).eval())
    g = torch.Generator().manual_seed(10)
    y = {"cond_embed": torch.randn(B, cond_tokens_for_frames(T), m.cond_feature_dim, generator=g).to(dev),
         "scale": torch.full((B,), 10.0, device=dev)}
    x = torch.randn(B, m.nfeats, 1, T, generator=g).to(dev)
    prev = torch.randn(B, m.nfeats, 1, T, generator=g).to(dev)
    tab, tmap, cf = diff._tables(dev), diff._timestep_map(dev), diff._multistep_coefs(dev)
    t = torch.full((B,), 50, dtype=torch.int64, device=dev)
    variants = {
        "ddim": lambda: model.a2p_sample_step(_lib.SAMPLER_DDIM, x, t, tmap, tab, y, None, 0.0, False),
        "multistep": lambda: model.a2p_sample_step_multistep(x, t, tmap, cf, y, prev, False),
    }
    with torch.no_grad():
        for fn in variants.values():
            for _ in range(warmup):
                fn()
        torch.cuda.synchronize(dev)
        _, x0d = variants["ddim"]()
        _, x0m = variants["multistep"]()
        same_x0 = bool(torch.equal(x0d, x0m))        # same forward, same guided output
        step_ms = {k: [] for k in variants}
        for _ in range(rounds):
            for name, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(steps):
                    fn()
                e1.record()
                e1.synchronize()
                step_ms[name].append(round(e0.elapsed_time(e1) / steps, 4))
        model.model.check_finite()
    m.release()
    mean = {k: sum(v) / len(v) for k, v in step_ms.items()}
    return {"what": f"face {layers}L fp16 (synthetic weights), B={B}, T={T}, one step at t=50 of ddim100: a2p_sample_step (ddim, eta 0) vs "
                    f"a2p_sample_step_multistep (second order, with history); {rounds} rounds of {steps} steps each, alternating, device events",
            "step_ms": step_ms, "mean_ms": {k: round(v, 4) for k, v in mean.items()},
            "multistep_over_ddim": round(mean["multistep"] / mean["ddim"], 4), "pred_xstart_bit_identical": same_x0}


def _pipeline(dev, reps):
    """Face and body models at the demo's shape with native front ends and the guide (synthetic weights), fp16."""
    from audio2photoreal_amd.model.guide import GuideTransformer
    from audio2photoreal_amd.model.vqvae import TemporalVertexCodec
    from audio2photoreal_amd.spec import GuideSpec, TokenizerSpec, pose_spec
    from audio2photoreal_amd.synthetic import (synthetic_frontend_state_dict, synthetic_guide_state_dict, synthetic_tokenizer_state_dict)
    gs, ts = GuideSpec(), TokenizerSpec()
    guide = GuideTransformer(tokens=gs.tokens, num_layers=gs.num_layers, dim=gs.dim, emb_len=gs.emb_len,
                             num_audio_layers=gs.num_audio_layers, max_batch=reps)
    guide.load_state_dict(synthetic_guide_state_dict(gs, 10), strict=False)
    tok = TemporalVertexCodec(ts.n_vertices, ts.latent_dim, ts.categories, ts.residual_depth)
    tok.load_state_dict(synthetic_tokenizer_state_dict(ts, 10), strict=False)
    out = {}
    for fmt, spec in (("face", face_spec()), ("pose", pose_spec())):
        m, _ = create_model_and_diffusion(default_args(fmt), "test", precision="fp16", max_batch=reps, audio_frontend="native")
        load_model(m, {**synthetic_state_dict(spec, 10), **synthetic_frontend_state_dict(10, lip=fmt == "face")})
        if fmt == "pose":
            m.setup_guide_predictor(guide.to(dev).eval(), tok.to(dev))
        out[fmt] = ClassifierFreeSampleModel(m.to(dev).eval())
    return out


def clip_timing(dev, reps, clips):
    from audio2photoreal_amd.sample.recording import generate_from_recording
    models = _pipeline(dev, reps)
    rng = np.random.default_rng(7)
    sr, secs = 48000, 20.0
    n = int(sr * secs)
    t = np.arange(n) / sr
    wav = (0.3 * np.sin(2 * np.pi * 220 * t) * (0.6 + 0.4 * np.sin(2 * np.pi * t / 7.0)) + 0.02 * rng.standard_normal(n)).astype(np.float32)
    r = np.random.default_rng(10)
    stats = {"audio_mean": np.array([0.003, -0.001]), "audio_std_flat": np.array([0.21]),
             "code_mean": r.standard_normal(256), "code_std": 0.5 + r.random(256),
             "pose_mean": r.standard_normal(104), "pose_std": 0.5 + r.random(104)}
    configs = {"ddim100_ddim": ("ddim100", "ddim"), "ddim20_dpm++2m": ("ddim20", "dpm++2m")}

    def run(name):
        resp, sampler = configs[name]
        face = (models["face"], create_gaussian_diffusion(default_args("face", timestep_respacing=resp)))
        pose = (models["pose"], create_gaussian_diffusion(default_args("pose", timestep_respacing=resp)))
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        res = generate_from_recording(face, pose, stats, wav, sr, num_repetitions=reps, seed=10, sampler=sampler)
        torch.cuda.synchronize(dev)
        return time.perf_counter() - t0, res

    with torch.no_grad():
        for name in configs:
            run(name)                                   # warm-up: contexts, graphs, tables
        secs_per_clip = {k: [] for k in configs}
        finite = True
        for _ in range(clips):
            for name in configs:
                dt, res = run(name)
                secs_per_clip[name].append(round(dt, 4))
                finite &= bool(all(np.isfinite(res[k]).all() for k in ("face", "pose")))
    mean = {k: sum(v) / len(v) for k, v in secs_per_clip.items()}
    for m in models.values():
        m.model.release()
    return {"what": f"generate_from_recording, 20 s recording (600 frames), {reps} repetitions, face + body 8L fp16 (synthetic weights) "
                    f"with native front ends and the guide, overlap on; wall clock per call, {clips} calls each, alternating, after one warm-up",
            "s_per_clip": secs_per_clip, "mean_s_per_clip": {k: round(v, 4) for k, v in mean.items()},
            "speedup": round(mean["ddim100_ddim"] / mean["ddim20_dpm++2m"], 3), "outputs_finite": finite}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--clips", type=int, default=3)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("multistep_step_bench measures on the MI355X: no GPU found")
    dev = torch.device("cuda:0")
    out = {"step": step_timing(dev, a.rounds, a.steps, a.warmup), "clip": clip_timing(dev, a.reps, a.clips),
           "note": "synthetic weights: the timings hold for any checkpoint of these shapes; the quality of 20 dpm++2m steps on a trained "
                   "checkpoint is not measured here"}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
