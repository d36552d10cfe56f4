"""From a capture directory to results.npy and the paper's metrics: the reference's `python -m sample.generate` on the
test split (sample/generate.py:236-292), with the batches assembled on the GPU (data/batches.py, csrc/kernels_dataset.h).

    python -m audio2photoreal_amd.sample.dataset --model_path checkpoints/diffusion/c1_pose/model000340000.pt \\
        --data_root dataset/PXB184 --num_samples 10 --num_repetitions 5 --timestep_respacing ddim20 --sampler dpm++2m \\
        --resume_trans checkpoints/guide/c1_pose/checkpoints/iter-0100000.pt --all --evaluate --json metrics.json

The model's arguments come from the `args.json` next to the checkpoint, as in the reference.  The test split is the last 4
takes, cut into `max_seq_length`-frame chunks and shuffled by the seed (data/capture.py chunk_plan).  Like the reference, the
plain command samples the first `num_samples` chunks; `--all` goes through every chunk in batches of `num_samples` (the last one
may be shorter).  results.npy keeps the reference's keys and layouts: motions / gt [R * B, C, 1, T], audio [R * B, T * 1600, 2],
lengths [R * B], keyframes -- repetition-major per batch; with `--all` the batches are interleaved so that the whole block stays
repetition-major ([R, chunks] flattened), which is what utils/eval.py and `audio2photoreal_amd.evaluate` expect.
Every error of the arguments, the directory or the statistics is an A2PError raised before any GPU work."""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from typing import Dict, List

import numpy as np
import torch

from .. import _lib
from .._lib import A2PError
from ..data import capture as cap
from .generate import _generate_sequences, _setup_model, fixseed, load_data_stats, pose_guidance_plan, save_results
from .recording import MULTISTEP, SAMPLERS

_MODEL_DEFAULTS = dict(heads=8, not_rotary=False, unconstrained=False, noise_schedule="cosine", sigma_small=True, lambda_vel=0.0,
                       max_seq_length=600, num_audio_layers=3)
_KEYS = ("motions", "audio", "gt", "lengths", "keyframes")


def build_parser() -> argparse.ArgumentParser:
    ap = argparse.ArgumentParser(prog="python -m audio2photoreal_amd.sample.dataset",
                                 description="Sample (and score) the test split of a capture directory on the MI355X.")
    ap.add_argument("--model_path", required=True, help="denoiser checkpoint (a state dict) next to its args.json")
    ap.add_argument("--data_root", required=True, help="capture directory of one person, e.g. dataset/PXB184, with data_stats.pth")
    ap.add_argument("--num_samples", type=int, default=10, help="chunks per batch (default 10)")
    ap.add_argument("--num_repetitions", type=int, default=3, help="samples per chunk (default 3)")
    ap.add_argument("--timestep_respacing", default="ddim100", help="ddimN (default ddim100)")
    ap.add_argument("--guidance_param", type=float, default=2.5, help="classifier-free guidance scale (default 2.5)")
    ap.add_argument("--pose_guidance", default="joint", help="pose checkpoints: joint (default: --guidance_param moves audio and keyframes "
                                                             "together) | audio (keyframes as they are, guidance on the audio) | dual")
    ap.add_argument("--pose_keyframe_scale", type=float, default=None, help="with --pose_guidance dual: the keyframes' guidance scale "
                                                                            "(--guidance_param is then the audio's)")
    ap.add_argument("--resume_trans", default=None, help="guide transformer checkpoint (pose): sample the keyframes instead of "
                                                         "taking the ground truth's motion[::30]")
    ap.add_argument("--seed", type=int, default=10)
    ap.add_argument("--flip_person", action="store_true", help="the partner's directory with the audio channels swapped")
    ap.add_argument("--max_seq_length", type=int, default=None, help="chunk length in frames (default: args.json's, 600)")
    ap.add_argument("--output_dir", default="", help="default: samples_<run>_<iter>_seed<seed> next to the checkpoint")
    ap.add_argument("--sampler", default="ddim", help="ddim | dpm++2m")
    ap.add_argument("--precision", default="fp32", choices=("fp32", "fp16", "bf16"))
    ap.add_argument("--all", action="store_true", help="every chunk of the split, in batches of --num_samples")
    ap.add_argument("--evaluate", action="store_true", help="run evaluate_motion on the written block")
    ap.add_argument("--json", default=None, help="with --evaluate: write the metrics (and the timing) to this file")
    ap.add_argument("--diversity_times", type=int, default=10_000, help="frame pairs of the diversity draw of --evaluate")
    ap.add_argument("--device", default="cuda")
    for flag in ("--plot", "--render_gt"):
        ap.add_argument(flag, action="store_true", help="not available: there is no renderer")
    for flag in ("--face_codes", "--pose_codes"):
        ap.add_argument(flag, default=None, help="not available: there is no renderer")
    return ap


def _model_args(cli) -> argparse.Namespace:
    """The reference's merged args: args.json next to the checkpoint for the model, the command line for the sampling."""
    if not os.path.isfile(cli.model_path):
        raise A2PError(f"checkpoint {cli.model_path} not found")
    args_path = os.path.join(os.path.dirname(cli.model_path), "args.json")
    if not os.path.isfile(args_path):
        raise A2PError(f"{args_path} not found: the checkpoint's args.json must lie next to it")
    with open(args_path) as f:
        saved = json.load(f)
    if saved.get("data_format") not in ("pose", "face"):
        raise A2PError(f"{args_path}: data_format must be 'pose' or 'face' (got {saved.get('data_format')!r})")
    fmt = saved["data_format"]
    merged = {**_MODEL_DEFAULTS, "layers": 8 if fmt == "face" else 6, "add_frame_cond": 1 if fmt == "pose" else None,
              **{k: v for k, v in saved.items() if k in _MODEL_DEFAULTS or k in ("layers", "data_format", "add_frame_cond")}}
    if cli.max_seq_length is not None:
        merged["max_seq_length"] = cli.max_seq_length
    name = os.path.basename(os.path.dirname(os.path.abspath(cli.model_path)))
    niter = os.path.basename(cli.model_path).replace("model", "").replace(".pt", "")
    out = cli.output_dir or os.path.join(os.path.dirname(cli.model_path), f"samples_{name}_{niter}_seed{cli.seed}")
    return argparse.Namespace(**merged, model_path=cli.model_path, data_root=cli.data_root, device=cli.device,
                              timestep_respacing=cli.timestep_respacing, guidance_param=cli.guidance_param,
                              num_samples=cli.num_samples, batch_size=cli.num_samples, num_repetitions=cli.num_repetitions,
                              curr_seq_length=merged["max_seq_length"], seed=cli.seed, output_dir=out,
                              resume_trans=cli.resume_trans if fmt == "pose" else None,
                              pose_guidance=cli.pose_guidance, pose_keyframe_scale=cli.pose_keyframe_scale)


def _check_cli(cli) -> None:
    if cli.plot or cli.render_gt or cli.face_codes or cli.pose_codes:
        raise A2PError("--plot / --render_gt / --face_codes / --pose_codes need the reference's renderer; there is no renderer here: "
                       "render results.npy with the reference's visualize/ tools")
    if cli.sampler not in SAMPLERS:
        raise A2PError(f"--sampler must be one of {SAMPLERS} (got {cli.sampler!r})")
    if cli.num_samples < 1 or cli.num_repetitions < 1:
        raise A2PError("--num_samples and --num_repetitions must be at least 1")
    if cli.num_samples > _lib.DATASET_MAX_BATCH:
        raise A2PError(f"--num_samples is at most {_lib.DATASET_MAX_BATCH}")
    pose_guidance_plan(cli.guidance_param, cli.pose_guidance, cli.pose_keyframe_scale)
    if cli.json and not cli.evaluate:
        raise A2PError("--json goes with --evaluate")


def _load_guide(resume_trans: str, device, max_batch: int):
    """(GuideTransformer, TemporalVertexCodec) from a guide checkpoint in the reference's layout (model/diffusion.py:244-268,
    model/vqvae.py:18-34): `<run>/checkpoints/iter-*.pt` holding "model_state_dict", `<run>/args.json` with layers / dim /
    num_audio_layers / resume_pth, and the tokenizer checkpoint `resume_pth` ("net") next to its own args.json."""
    from ..model.guide import GuideTransformer
    from ..model.vqvae import TemporalVertexCodec
    if not os.path.isfile(resume_trans):
        raise A2PError(f"guide checkpoint {resume_trans} not found")
    cp_dir = resume_trans.split("checkpoints/iter-")[0]
    try:
        with open(os.path.join(cp_dir, "args.json")) as f:
            targs = json.load(f)
        with open(os.path.join(os.path.dirname(targs["resume_pth"]), "args.json")) as f:
            vargs = json.load(f)
        tok = TemporalVertexCodec(n_vertices=vargs["nb_joints"], latent_dim=vargs["output_emb_width"], categories=vargs["code_dim"],
                                  residual_depth=vargs["depth"])
        net = torch.load(targs["resume_pth"], map_location="cpu", weights_only=False)["net"]
        own = tok.state_dict()
        tok.load_state_dict({k: v for k, v in net.items() if k in own}, strict=True)     # a decoder-only codec skips the encoder's tensors
        guide = GuideTransformer(tokens=tok.n_clusters, num_layers=targs["layers"], dim=targs["dim"], emb_len=1998,
                                 num_audio_layers=targs["num_audio_layers"], max_batch=max_batch)
        state = torch.load(resume_trans, map_location="cpu", weights_only=False)["model_state_dict"]
        missing, unexpected = guide.load_state_dict(state, strict=False)
    except (OSError, KeyError) as e:
        raise A2PError(f"--resume_trans {resume_trans}: {type(e).__name__} {e} (expected the reference's layout: <run>/checkpoints/"
                       f"iter-*.pt with <run>/args.json naming the tokenizer's resume_pth)") from None
    if unexpected or any(not k.endswith("rotary.freqs") for k in missing):
        raise A2PError(f"--resume_trans {resume_trans}: missing keys {missing}, unexpected keys {unexpected}")
    return guide.to(device).eval(), tok.to(device).eval()


class _SamplerView:
    """A SpacedDiffusion whose `ddim_sample_loop` is the loop `--sampler` names: `_run_single_diffusion` calls that attribute."""

    def __init__(self, diffusion, sampler: str):
        self._d = diffusion
        self.ddim_sample_loop = diffusion.dpm_solver_sample_loop if sampler == MULTISTEP else diffusion.ddim_sample_loop

    def __getattr__(self, name):
        return getattr(self._d, name)


def _merge(blocks: List[Dict[str, np.ndarray]], R: int) -> Dict[str, np.ndarray]:
    """Batches of [R * B_i, ...] (repetition-major each) -> one repetition-major block [R * sum B_i, ...]."""
    out = {}
    for k in _KEYS:
        if any(b[k] is None for b in blocks):
            out[k] = None
            continue
        per = [b[k].reshape((R, -1) + b[k].shape[1:]) for b in blocks]
        v = np.concatenate(per, axis=1)
        out[k] = v.reshape((-1,) + v.shape[2:])
    return out


def run(cli) -> Dict[str, object]:
    """The command on parsed arguments: {"results": path, "metrics": dict | None, "timing": seconds per phase, "chunks": n}."""
    _check_cli(cli)
    args = _model_args(cli)
    if cli.pose_guidance != "joint" and args.data_format != "pose":
        raise A2PError(f"--pose_guidance {cli.pose_guidance} separates the audio from the keyframes: a {args.data_format} checkpoint has no keyframes")
    stats_path = os.path.join(cli.data_root, "data_stats.pth")
    if not os.path.isfile(stats_path):
        raise A2PError(f"{stats_path} not found: the subject's data_stats.pth must lie in --data_root")
    if args.resume_trans is not None and not os.path.isfile(args.resume_trans):
        raise A2PError(f"guide checkpoint {args.resume_trans} not found")
    timing = {}
    t0 = time.perf_counter()
    stats = load_data_stats(stats_path)
    from ..data.batches import CaptureBatches, check_stats
    check_stats(stats, args.data_format)
    takes = cap.test_split(cap.load_capture(cli.data_root, flip_person=cli.flip_person))
    T = int(args.max_seq_length)
    plan = cap.chunk_plan([t.frames for t in takes], T, cli.seed)
    if not len(plan):
        raise A2PError(f"the test split is empty: none of its takes is longer than {T} frames (lengths {[t.frames for t in takes]})")
    if cli.num_samples > len(plan):
        raise A2PError(f"--num_samples {cli.num_samples} exceeds the {len(plan)} chunks of the test split")
    chunks = len(plan) if cli.all else cli.num_samples
    if cli.evaluate and not cli.num_repetitions * chunks * T > cli.diversity_times:
        raise A2PError(f"--evaluate draws {cli.diversity_times} frame pairs but the block will hold only "
                       f"{cli.num_repetitions * chunks * T} frames: lower --diversity_times or sample more")
    timing["load_s"] = time.perf_counter() - t0
    device = torch.device(cli.device)
    if device.type != "cuda" or not torch.cuda.is_available():
        raise A2PError(f"sampling runs on the MI355X (device {cli.device}, cuda available: {torch.cuda.is_available()}); "
                       "there is no CPU implementation")

    fixseed(cli.seed)
    t0 = time.perf_counter()
    state = torch.load(cli.model_path, map_location="cpu", weights_only=False)
    from ..model.audio_frontend import FAIRSEQ, STUB
    geometry = FAIRSEQ if "audio_model.feature_extractor.conv_layers.0.2.weight" in state else STUB
    guide = _load_guide(args.resume_trans, device, cli.num_samples) if args.resume_trans is not None else None
    model, diffusion = _setup_model(args, state, guide=guide, audio_frontend="native", audio_geometry=geometry,
                                    precision=cli.precision,   # ("dual" runs three branches: 3B sequences in a context of 2 * max_batch)
                                    max_batch=(3 * cli.num_samples + 1) // 2 if cli.pose_guidance == "dual" else cli.num_samples)
    torch.cuda.synchronize(device)
    timing["model_s"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    data = CaptureBatches(takes, stats, args.data_format, T=T, seed=cli.seed, device=device)
    torch.cuda.synchronize(device)
    timing["upload_s"] = time.perf_counter() - t0

    B = cli.num_samples
    batches = [list(range(i, min(i + B, len(data)))) for i in range(0, len(data), B)] if cli.all else [list(range(B))]
    view = _SamplerView(diffusion, cli.sampler)
    blocks = []
    timing["batch_s"] = timing["sample_s"] = 0.0
    for idx in batches:
        t0 = time.perf_counter()
        gt, model_kwargs = data.batch(idx)
        torch.cuda.synchronize(device)
        timing["batch_s"] += time.perf_counter() - t0
        t0 = time.perf_counter()
        args.batch_size = len(idx)
        blocks.append(_generate_sequences(args, model_kwargs, view, model, data.inv_transform, gt))
        torch.cuda.synchronize(device)
        timing["sample_s"] += time.perf_counter() - t0
    block = _merge(blocks, cli.num_repetitions)
    path = save_results(args.output_dir, block)
    print(f"saved {sum(len(i) for i in batches)} chunk(s) x {cli.num_repetitions} repetition(s) to [{path}]")

    metrics = None
    if cli.evaluate:
        from ..evaluate import evaluate_motion, format_lines
        t0 = time.perf_counter()
        metrics = evaluate_motion(block["motions"], block["gt"], num_samples=cli.num_repetitions,
                                  diversity_times=cli.diversity_times, seed=0)
        timing["evaluate_s"] = time.perf_counter() - t0
        for line in format_lines(metrics):
            print(line)
        if cli.json:
            with open(cli.json, "w") as f:
                json.dump({"results": path, "num_samples": cli.num_repetitions, "seed": 0, "diversity_times": cli.diversity_times,
                           "chunks": sum(len(i) for i in batches), "sampler": cli.sampler, "timing": timing, **metrics}, f, indent=1)
    return {"results": path, "metrics": metrics, "timing": timing, "chunks": sum(len(i) for i in batches)}


def main(argv=None) -> int:
    run(build_parser().parse_args(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
