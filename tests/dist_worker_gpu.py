"""Worker of tests/test_hip_round2.py::test_two_ranks_sharing_the_gpu_match_single_rank_bit_for_bit.

Launched as `python -m torch.distributed.run --nproc-per-node 2 tests/dist_worker_gpu.py`: every rank opens its own HIP
context on cuda:0 (single-GPU box), collectives go over gloo (host memory), the sampler is the product's HIP path driven
through `sample_parallel` exactly like sample/generate.py does.  Production differs only in `cuda:LOCAL_RANK` + backend
"nccl" (= RCCL over xGMI).

A2P_DIST_GEOMETRY="samples,frames,layers,respacing" (face model) selects another geometry; the default is DEFAULT_GEOMETRY
(tests/test_shard_invariance_hip.py runs the full-size face configuration over 4 ranks)."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEFAULT_GEOMETRY = "4,240,2,ddim10"


def parse_geometry(geometry=None):
    total, frames, layers, respacing = (geometry or os.environ.get("A2P_DIST_GEOMETRY") or DEFAULT_GEOMETRY).split(",")
    return int(total), int(frames), int(layers), respacing


def run_sampler(precision, dev, world, rank, geometry=None):
    from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from audio2photoreal_amd.model_util import create_model_and_diffusion, default_args, load_model
    from audio2photoreal_amd.sample_parallel import per_sample_noise, sample_parallel
    from audio2photoreal_amd.spec import face_spec
    from audio2photoreal_amd.synthetic import cond_tokens_for_frames, synthetic_state_dict, synthetic_tensor
    TOTAL, T, LAYERS, respacing = parse_geometry(geometry)
    steps = int(respacing[len("ddim"):])
    spec = face_spec(num_layers=LAYERS)
    model, diffusion = create_model_and_diffusion(default_args("face", layers=LAYERS, timestep_respacing=respacing), "test",
                                                  precision=precision, max_batch=TOTAL)
    load_model(model, synthetic_state_dict(spec, 10))
    cfg = ClassifierFreeSampleModel(model.to(dev).eval())
    S0 = cond_tokens_for_frames(T)
    # the FULL global batch on every rank (what a data loader hands over); sample_parallel slices this rank's block
    y = {"cond_embed": torch.stack([synthetic_tensor(10, f"cond_embed/{g}", (S0, spec.cond_feature_dim)) for g in range(TOTAL)]).to(dev),
         "scale": torch.full((TOTAL,), 10.0, device=dev)}
    shape = (TOTAL, spec.nfeats, 1, T)
    noise = per_sample_noise(shape, [1000 + g for g in range(TOTAL)])          # row g depends only on the global sample id
    step_noise = [per_sample_noise(shape, [77 * (n + 1) + g for g in range(TOTAL)]).to(dev) for n in range(steps)]
    with torch.no_grad():
        out = sample_parallel(diffusion.ddim_sample_loop, cfg, shape, {"y": y}, noise=noise.to(dev), step_noise=step_noise,
                              clip_denoised=False, eta=0.5)                    # eta > 0: the per-step noise path is exercised too
    return out


def main():
    import torch.distributed as dist
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    dist.init_process_group("gloo")
    # gloo gathers host tensors: route the single end-of-run collective through the host
    from audio2photoreal_amd import sample_parallel as SP
    orig = SP.gather_samples
    SP.gather_samples = lambda local, total, group=None: orig(local.cpu(), total, group)
    out = run_sampler(os.environ.get("A2P_DIST_PRECISION", "bf16"), dev, world, rank)
    torch.save(out.cpu(), os.path.join(os.environ["A2P_DIST_OUT"], f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
