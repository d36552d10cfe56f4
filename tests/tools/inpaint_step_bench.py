"""One inpaint step against one plain step on the MI355X (profiles/inpaint_step.json).

Face model, 8 layers (synthetic weights), fp16, B = 8, T = 600, ddim100 tables, the step at t = 50.  `a2p_sample_step` and
`a2p_sample_step_inpaint` (the first 120 frames held) are timed in alternating rounds of `--steps` calls each, with device events
around every round, after a warm-up of both.  Prints one JSON object and writes it to `--out` when given.

    python tests/tools/inpaint_step_bench.py --rounds 5 --steps 40 --out inpaint_step.json
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from audio2photoreal_amd import _lib                                                    # noqa: E402
from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel              # noqa: E402
from audio2photoreal_amd.model_util import create_model_and_diffusion, default_args, load_model   # noqa: E402
from audio2photoreal_amd.sample.inpaint import expand_mask                               # noqa: E402
from audio2photoreal_amd.spec import face_spec                                           # noqa: E402
from audio2photoreal_amd.synthetic import cond_tokens_for_frames, synthetic_state_dict   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("inpaint_step_bench measures on the MI355X: no GPU found")
    dev = torch.device("cuda:0")
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
    known = torch.randn(B, m.nfeats, 1, T, generator=g).to(dev)
    held = torch.zeros(B, T, dtype=torch.bool, device=dev)
    held[:, :120] = True
    mask = expand_mask(held, B, m.nfeats, T)
    tab, tmap = diff._tables(dev), diff._timestep_map_tensor(dev)
    t = torch.full((B,), 50, dtype=torch.int64, device=dev)
    variants = {
        "plain": lambda: model.a2p_sample_step(_lib.SAMPLER_DDIM, x, t, tmap, tab, y, None, 0.0, False),
        "inpaint": lambda: model.a2p_sample_step_inpaint(_lib.SAMPLER_DDIM, x, t, tmap, tab, y, None, 0.0, False, known, mask),
    }
    with torch.no_grad():
        for fn in variants.values():
            for _ in range(a.warmup):
                fn()
        torch.cuda.synchronize(dev)
        # the two steps agree on every unheld element (same forward, same tail arithmetic)
        xp, x0p = variants["plain"]()
        xi, x0i = variants["inpaint"]()
        free = ~mask.bool()
        same_unheld = bool(torch.equal(xp[free], xi[free]) and torch.equal(x0p[free], x0i[free]))
        held_exact = bool(torch.equal(x0i[~free], known[~free]))
        step_ms = {k: [] for k in variants}
        for _ in range(a.rounds):
            for name, fn in variants.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.steps):
                    fn()
                e1.record()
                e1.synchronize()
                step_ms[name].append(round(e0.elapsed_time(e1) / a.steps, 4))
        model.model.check_finite()
    mean = {k: sum(v) / len(v) for k, v in step_ms.items()}
    out = {"what": f"face {layers}L fp16 (synthetic weights), B={B}, T={T}, one ddim step at t=50: a2p_sample_step vs "
                   f"a2p_sample_step_inpaint (120 of {T} frames held); {a.rounds} rounds of {a.steps} steps each, alternating, device events",
           "step_ms": step_ms, "mean_ms": {k: round(v, 4) for k, v in mean.items()},
           "inpaint_over_plain": round(mean["inpaint"] / mean["plain"], 4),
           "unheld_elements_bit_identical": same_unheld, "held_pred_xstart_is_known": held_exact}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
