"""CPU-side checks (no GPU): the C-ABI library loads and exports every symbol include/a2p_hip.h
declares, the host logic (schedule tables, respacing, state_dict contract, sharding) matches the
reference's golden vectors, and the product path fails loudly instead of falling back to a CPU path."""
import os
import re
import socket
import sys

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp

from audio2photoreal_amd import _lib
from audio2photoreal_amd.diffusion import gaussian_diffusion as gd
from audio2photoreal_amd.diffusion.respace import SpacedDiffusion, _WrappedModel, space_timesteps
from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel
from audio2photoreal_amd.model_util import create_gaussian_diffusion, create_model_and_diffusion, default_args, load_model
from audio2photoreal_amd.sample_parallel import gather_samples, per_sample_noise, sample_parallel, shard_bounds, shard_model_kwargs
from audio2photoreal_amd.spec import face_spec, param_count, param_shapes, pose_spec
from audio2photoreal_amd.synthetic import cond_tokens_for_frames, synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------- C ABI
def _declared_symbols():
    src = open(os.path.join(ROOT, "include", "a2p_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(a2p_[a-z0-9_]+)\s*\(", src)))


def test_header_symbols_are_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.load()
    declared = _declared_symbols()
    assert len(declared) >= 18
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in include/a2p_hip.h but not exported by liba2p_hip.so"
    assert sorted(_lib.EXPORTS) == declared, "ctypes binding list and header disagree"
    assert lib.a2p_version().decode().startswith("a2p_hip")


# Environment reads of csrc/ outside load_opts: read once per context or per process, so a2p_reload_env cannot see them and no test
# may toggle them on a live context.  A new name here needs a reason; a switch meant to be toggled belongs in load_opts.
STATIC_ENV_READS = {"A2P_TAIL16", "A2P_TAIL_F32", "A2P_NO_FUSED_TAIL", "A2P_NO_ARENA", "A2P_CHAIN_CLK", "A2P_STAMP_LAUNCH"}


def test_env_switch_inventory_matches_the_library():
    """Python calls a2p_reload_env only when a name of _lib.ENV_SWITCHES changes: a switch load_opts reads but the tuple lacks would
    make every test that toggles it compare a path with itself.  So: the names load_opts reads (csrc/a2p_lib.hip) are exactly
    _lib.ENV_SWITCHES, every other getenv("A2P_...") of csrc/ is in the short list above, and INTEGRATION.md names them all."""
    csrc = os.path.join(ROOT, "audio2photoreal_amd", "csrc")
    lib_src = open(os.path.join(csrc, "a2p_lib.hip")).read()
    body = re.search(r"static void load_opts\(A2POpts& o\) \{(.*?)\n\}", lib_src, flags=re.S).group(1)
    loaded = re.findall(r"\b(?:flag|num)\(\"(A2P_[A-Z0-9_]+)\"", body)
    assert len(loaded) == len(set(loaded)) and len(_lib.ENV_SWITCHES) == len(set(_lib.ENV_SWITCHES))
    assert set(loaded) == set(_lib.ENV_SWITCHES), set(loaded) ^ set(_lib.ENV_SWITCHES)
    assert "getenv(\"" not in body, "load_opts reads through flag / num only"
    static = set()
    for name in sorted(os.listdir(csrc)):
        static |= set(re.findall(r"getenv\(\"(A2P_[A-Z0-9_]+)\"\)", open(os.path.join(csrc, name)).read()))
    assert static == STATIC_ENV_READS, static ^ STATIC_ENV_READS
    assert not static & set(loaded)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    missing = [n for n in sorted(static | set(loaded)) if not re.search(r"\b" + n + r"\b", doc)]
    assert not missing, f"not in INTEGRATION.md: {missing}"


def test_abi_rejects_bad_config_without_touching_the_gpu():
    lib = _lib.load()
    import ctypes as C
    cfg = _lib.A2PConfig(data_format=0, nfeats=256, latent_dim=384, ff_size=1024, num_layers=8, num_heads=8, cond_feature_dim=2038,
                         max_frames=600, emb_len=1998, keyframe_dim=104, keyframe_step=30, precision=1, max_batch=1, reserved=0)
    ctx = C.c_void_p()
    rc = lib.a2p_ctx_create(C.byref(cfg), C.byref(ctx))
    assert rc == -1 and b"latent_dim" in lib.a2p_last_error()      # A2P_ERR_ARG, like the reference's shape asserts
    with pytest.raises(_lib.A2PError):
        _lib.check(rc, "a2p_ctx_create")


# ----------------------------------------------------------------------------- host schedule == reference
_TABLES = ("betas", "alphas_cumprod", "alphas_cumprod_prev", "sqrt_recip_alphas_cumprod", "sqrt_recipm1_alphas_cumprod",
           "posterior_variance", "posterior_log_variance_clipped", "posterior_mean_coef1", "posterior_mean_coef2",
           "sqrt_alphas_cumprod", "sqrt_one_minus_alphas_cumprod")


@pytest.mark.parametrize("name,resp", [("full", ""), ("ddim10", "ddim10"), ("ddim100", "ddim100"), ("ddim500", "ddim500")])
def test_product_schedule_bit_exact_vs_reference(golden, name, resp):
    d = create_gaussian_diffusion(default_args("face", timestep_respacing=resp))
    assert isinstance(d, SpacedDiffusion)
    for k in _TABLES:
        assert np.array_equal(getattr(d, k), golden[f"sched/{name}/{k}"]), k       # float64, bit exact
    assert d.timestep_map == list(golden[f"sched/{name}/timestep_map"])
    assert d.num_timesteps == len(d.timestep_map)


def test_space_timesteps_matches_reference(golden):
    assert sorted(space_timesteps(1000, "ddim50")) == list(golden["sched/space/ddim50"])
    assert sorted(space_timesteps(300, "10,15,20")) == list(golden["sched/space/10,15,20"])
    assert sorted(space_timesteps(300, [10, 15, 20])) == list(golden["sched/space/10,15,20"])
    assert space_timesteps(1000, [1000]) == set(range(1000))
    with pytest.raises(ValueError):
        space_timesteps(1000, "ddim999")
    with pytest.raises(ValueError):
        space_timesteps(10, "20")


def test_wrapped_model_maps_step_index_to_original_timestep():
    seen = {}

    def model(x, ts, **kw):
        seen["ts"] = ts
        return x
    w = _WrappedModel(model, [0, 100, 200, 300], False, 1000)
    w(torch.zeros(2), torch.tensor([3, 1]))
    assert seen["ts"].tolist() == [300, 100]
    w = _WrappedModel(model, [0, 100, 200, 300], True, 1000)
    w(torch.zeros(2), torch.tensor([2, 0]))
    assert seen["ts"].dtype == torch.float32 and seen["ts"].tolist() == [200.0, 0.0]


def test_fixed_large_variance_tables():
    betas = gd.get_named_beta_schedule("linear", 50)
    d = gd.GaussianDiffusion(betas=betas, model_mean_type=gd.ModelMeanType.START_X, model_var_type=gd.ModelVarType.FIXED_LARGE,
                             loss_type=gd.LossType.MSE)
    var, logvar = d._variance_tables()
    assert np.array_equal(var[1:], betas[1:]) and var[0] == d.posterior_variance[1]
    assert np.allclose(np.exp(logvar), var)
    with pytest.raises(NotImplementedError):
        gd.get_named_beta_schedule("sqrt", 10)


# ----------------------------------------------------------------------------- construction / state_dict contract
@pytest.mark.parametrize("fmt", ["face", "pose"])
def test_state_dict_keys_follow_the_reference_layout(fmt):
    spec = face_spec() if fmt == "face" else pose_spec()
    model, diffusion = create_model_and_diffusion(default_args(fmt, timestep_respacing="ddim10"), "test")
    sd = model.state_dict()
    shapes = param_shapes(spec)
    hot = {k: tuple(v.shape) for k, v in sd.items() if not k.endswith("rotary.freqs")}
    assert hot == dict(shapes)
    assert sum(v.numel() for k, v in sd.items() if not k.endswith("rotary.freqs")) == param_count(spec)
    # every attention / norm / FiLM module carries the reference's parameter names
    p = "seqTransDecoder.stack.0."
    for k in ("self_attn.in_proj_weight", "multihead_attn.out_proj.bias", "linear1.weight", "norm3.bias", "film2.block.1.weight"):
        assert p + k in sd
    assert ("seqTransDecoder.stack.0.multihead_attn2.in_proj_weight" in sd) == spec.is_pose
    assert ("cond_encoder.1.self_attn.in_proj_weight" in sd) == (not spec.is_pose)
    assert ("post_pose_layers.5.weight" in sd) == spec.is_pose
    # attributes callers read (cfg_sampler.py:20-28, respace.py:133-135, generate.py:89)
    assert model.nfeats == spec.nfeats and model.cond_mode == "audio"
    assert model.add_frame_cond == (1 if spec.is_pose else None)
    cfg = ClassifierFreeSampleModel(model)
    assert cfg.nfeats == spec.nfeats and (cfg.step == 30 if spec.is_pose else not hasattr(cfg, "step"))
    assert diffusion.num_timesteps == 10


def test_load_model_checks_like_the_reference():
    spec = face_spec(num_layers=1)
    model, _ = create_model_and_diffusion(default_args("face", layers=1), "test")
    sd = synthetic_state_dict(spec, 3)
    sd["audio_model.feature_extractor.conv_layers.0.0.weight"] = torch.zeros(4)    # front-end tensors are skipped
    sd["lip_model.cond_projection.weight"] = torch.zeros(4)
    load_model(model, sd)
    assert torch.equal(model.state_dict()["final_layer.weight"], sd["final_layer.weight"])
    with pytest.raises(AssertionError):
        load_model(model, {**sd, "not_a_parameter": torch.zeros(1)})           # unexpected key
    bad = dict(sd)
    del bad["final_layer.weight"]
    with pytest.raises(AssertionError):
        load_model(model, bad)                                                 # missing hot-path key


def test_cond_token_geometry():
    assert cond_tokens_for_frames(600) == 1998 and cond_tokens_for_frames(240) == 798   # model/diffusion.py:136, train_guide.py:316


# ----------------------------------------------------------------------------- no CPU fallback
def test_product_fails_loudly_without_the_gpu():
    model, diffusion = create_model_and_diffusion(default_args("face", layers=1, timestep_respacing="ddim10"), "test")
    x = torch.zeros(1, 256, 1, 64)
    y = {"cond_embed": torch.zeros(1, cond_tokens_for_frames(64), 2038), "scale": torch.ones(1)}
    with pytest.raises(_lib.A2PError, match="no CPU implementation"):
        model(x, torch.tensor([5]), y)
    with pytest.raises(_lib.A2PError):
        diffusion.ddim_sample_loop(ClassifierFreeSampleModel(model), (1, 256, 1, 64), noise=x, model_kwargs={"y": y},
                                   clip_denoised=False)
    with pytest.raises(_lib.A2PError):
        diffusion.q_sample(x, torch.tensor([3]))
    with pytest.raises(NotImplementedError):
        model(x, torch.tensor([5]), y, cond_drop_prob=0.3)                      # training-time dropout: out of scope


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "audio2photoreal_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                assert not re.search(r"^\s*(from|import)\s+oracle\b", src, flags=re.M), f"{f} imports the oracle"
                assert "/root/reference" not in src.replace("(/root/reference", "")  # docstrings cite it; code never opens it


# ----------------------------------------------------------------------------- sample-parallel sharding
def test_shard_bounds_cover_and_balance():
    for total in (0, 1, 7, 8, 64, 65):
        for world in (1, 2, 3, 8):
            blocks = [shard_bounds(total, world, r) for r in range(world)]
            assert blocks[0][0] == 0 and blocks[-1][1] == total
            assert all(blocks[i][1] == blocks[i + 1][0] for i in range(world - 1))
            sizes = [hi - lo for lo, hi in blocks]
            assert max(sizes) - min(sizes) <= 1


def test_per_sample_noise_depends_only_on_the_global_sample_id():
    a = per_sample_noise((4, 3, 1, 5), [10, 11, 12, 13])
    b = per_sample_noise((2, 3, 1, 5), [12, 13])
    assert torch.equal(a[2:], b) and not torch.equal(a[0], a[1])


def test_shard_model_kwargs_slices_batch_tensors_only():
    y = {"cond_embed": torch.arange(12.).view(4, 3), "scale": torch.arange(4.), "mask": torch.ones(4, 1, 1, 6, dtype=torch.bool),
         "tag": "x", "table": torch.arange(5.)}
    out = shard_model_kwargs({"y": y, "other": 1}, 1, 3)
    assert out["other"] == 1 and out["y"]["tag"] == "x"
    assert out["y"]["cond_embed"].shape == (2, 3) and out["y"]["scale"].tolist() == [1.0, 2.0]
    assert out["y"]["table"].shape == (5,)                                      # not a per-sample tensor: untouched


def _fake_loop(model, shape, noise=None, model_kwargs=None, step_noise=None, **kw):
    """Stand-in for diffusion.*_sample_loop with the same per-sample independence: CPU arithmetic only."""
    y = model_kwargs["y"]
    x = noise.clone()
    for n in range(3):
        x = 0.5 * x + y["scale"].view(-1, 1, 1, 1) * y["cond_embed"].mean(dim=(1, 2)).view(-1, 1, 1, 1)
        if step_noise is not None:
            x = x + 0.1 * (step_noise(n) if callable(step_noise) else step_noise[n])
    return x


def _worker(rank, world, port, total, out_dir):
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    shape = (total, 4, 1, 6)
    seeds = list(range(100, 100 + total))
    noise = per_sample_noise(shape, seeds)
    steps = [per_sample_noise(shape, [s * 7 + n for s in seeds]) for n in range(3)]
    y = {"cond_embed": torch.arange(total * 6, dtype=torch.float32).view(total, 3, 2), "scale": torch.linspace(1, 2, total)}
    res = sample_parallel(_fake_loop, None, shape, {"y": y}, noise=noise, step_noise=steps)
    torch.save(res, os.path.join(out_dir, f"r{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.parametrize("total", [5, 8])
def test_world_size_2_gloo_matches_single_process(tmp_path, total):
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_worker, args=(2, port, total, str(tmp_path)), nprocs=2, join=True)
    shape = (total, 4, 1, 6)
    seeds = list(range(100, 100 + total))
    noise = per_sample_noise(shape, seeds)
    steps = [per_sample_noise(shape, [s * 7 + n for s in seeds]) for n in range(3)]
    y = {"cond_embed": torch.arange(total * 6, dtype=torch.float32).view(total, 3, 2), "scale": torch.linspace(1, 2, total)}
    want = sample_parallel(_fake_loop, None, shape, {"y": y}, noise=noise, step_noise=steps)   # world size 1: no collective
    r0, r1 = torch.load(tmp_path / "r0.pt"), torch.load(tmp_path / "r1.pt")
    assert torch.equal(r0, r1), "all ranks must hold all samples after the single all_gather"
    assert torch.equal(r0, want), "sharded result must be identical to the single-process result"


def test_gather_is_identity_without_a_process_group():
    t = torch.randn(3, 2)
    assert gather_samples(t, 3) is t


# ----------------------------------------------------------------------------- results format / un-normalisation
def test_inv_transform_matches_the_reference_on_its_own_statistics(tmp_path):
    """`make_inv_transform` against `Social.inv_transform` run by the reference on PXB184's data_stats.pth
    (tests/golden/make_golden_stats.py): same values, same dtype promotion (fp32 pose/face data -> float64)."""
    import os
    from audio2photoreal_amd.sample import generate as G
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_stats_v1.npz"))
    stats = {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith("stats/")}
    path = tmp_path / "data_stats.pth"
    torch.save(stats, path)
    inv = G.make_inv_transform(G.load_data_stats(str(path)))
    for kind in ("pose", "face"):
        got = inv(torch.from_numpy(z[f"in/{kind}"]), kind)
        assert got.dtype == torch.float64 and np.array_equal(got.numpy(), z[f"out/{kind}"]), kind
    got = inv(z["in/audio"], "audio")
    assert got.dtype == np.float32 and np.array_equal(got, z["out/audio"])     # the FLAT audio std, per-channel mean
    with pytest.raises(AssertionError):
        inv(z["in/audio"], "lips")


def test_results_file_round_trip_and_fixseed(tmp_path):
    from audio2photoreal_amd.sample import generate as G
    block = {"motions": np.arange(24, dtype=np.float32).reshape(2, 3, 1, 4), "audio": np.zeros((2, 8, 2), np.float32),
             "gt": np.ones((2, 3, 1, 4), np.float32), "lengths": np.array([4, 3]), "keyframes": np.zeros((2, 1, 3), np.float32)}
    path = G.save_results(str(tmp_path / "out"), block)
    assert path.endswith("results.npy")
    back = G.load_results(path)
    assert set(back) == {"motions", "audio", "gt", "lengths", "keyframes"}      # reference sample/generate.py:146-152
    assert all(np.array_equal(back[k], block[k]) for k in block)
    G.fixseed(10)
    a = (torch.rand(3), np.random.rand(3))
    G.fixseed(10)
    b = (torch.rand(3), np.random.rand(3))
    assert torch.equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ----------------------------------------------------------------------------- SURVEY §8 f2 / f4 host contracts (no GPU needed)
def test_guide_and_tokenizer_state_dict_contract_and_no_cpu_path():
    """Key names / shapes of the GuideTransformer and TemporalVertexCodec mirrors equal the spec that was checked against the
    reference modules (tests/golden/make_golden_guide.py loads the same dictionaries into the reference with strict key checks);
    like the denoiser they refuse to compute on CPU tensors."""
    from audio2photoreal_amd.model.guide import GuideTransformer
    from audio2photoreal_amd.model.vqvae import TemporalVertexCodec
    from audio2photoreal_amd.spec import GuideSpec, TokenizerSpec, guide_param_shapes, tokenizer_param_shapes
    from audio2photoreal_amd.synthetic import synthetic_guide_state_dict, synthetic_tokenizer_state_dict
    gs, ts = GuideSpec(), TokenizerSpec()
    g = GuideTransformer(tokens=gs.tokens, num_layers=gs.num_layers, dim=gs.dim, emb_len=gs.emb_len, num_audio_layers=gs.num_audio_layers)
    got = {k: tuple(v.shape) for k, v in g.state_dict().items() if not k.endswith("rotary.freqs")}
    assert got == dict(guide_param_shapes(gs))
    res = g.load_state_dict(synthetic_guide_state_dict(gs), strict=False)
    assert not res.unexpected_keys and all(k.endswith("rotary.freqs") for k in res.missing_keys)
    assert gs.cond_tokens_after_conv(1998) == 1950 and gs.cond_tokens_after_conv(798) == 750
    t = TemporalVertexCodec(ts.n_vertices, ts.latent_dim, ts.categories, ts.residual_depth)
    assert {k: tuple(v.shape) for k, v in t.state_dict().items()} == dict(tokenizer_param_shapes(ts))
    assert t.residual_depth == 4 and t.n_clusters == 1024
    t.load_state_dict(synthetic_tokenizer_state_dict(ts))
    with pytest.raises(_lib.A2PError):
        g(torch.zeros(1, 3, dtype=torch.int64), torch.zeros(1, 798, 1024))
    with pytest.raises(_lib.A2PError):
        t.decode(torch.zeros(1, 8, 4, dtype=torch.int64))
    with pytest.raises(_lib.A2PError):
        g.encode_audio(torch.zeros(1, 16000, 2))            # no audio front end attached
    with pytest.raises(NotImplementedError):
        GuideTransformer(tokens=8, use_rotary=False)


def test_setup_guide_predictor_keeps_the_denoiser_weight_set_separate():
    from audio2photoreal_amd.model.guide import GuideTransformer
    from audio2photoreal_amd.model.vqvae import TemporalVertexCodec
    model, _ = create_model_and_diffusion(default_args("pose", layers=1), "test", precision="fp32", max_batch=1)
    before = set(model._hot_state())
    sig = model._weights_signature()
    model.setup_guide_predictor(GuideTransformer(tokens=16, num_layers=1, dim=64, emb_len=64, num_audio_layers=1), TemporalVertexCodec(104, 64, 16, 4))
    assert set(model._hot_state()) == before and model._weights_signature()[0] == sig[0]
    assert any(k.startswith("transformer.") for k in model.state_dict()) and any(k.startswith("tokenizer.") for k in model.state_dict())
    assert model.resume_trans is not None and ClassifierFreeSampleModel(model).tokenizer is model.tokenizer
    face, _ = create_model_and_diffusion(default_args("face", layers=1), "test", precision="fp32", max_batch=1)
    with pytest.raises(AssertionError):
        face.setup_guide_predictor(model.transformer, model.tokenizer)


def test_plms_argument_checks_need_no_gpu():
    d = create_gaussian_diffusion(default_args("face", timestep_respacing="ddim10"))
    x = torch.zeros(1, 256, 1, 8)
    for bad in (0, 5, -1):
        with pytest.raises(ValueError):
            d.plms_sample(lambda *a, **k: None, x, torch.tensor([3]), order=bad)
    with pytest.raises(NotImplementedError):
        d.plms_sample(lambda *a, **k: None, x, torch.tensor([3]), cond_fn=lambda *a: None)
    with pytest.raises(AssertionError):
        d.ddim_reverse_sample(lambda *a, **k: None, x, torch.tensor([3]), eta=0.1)
    for name in ("plms_sample", "plms_sample_loop", "plms_sample_loop_progressive", "ddim_reverse_sample"):
        assert callable(getattr(d, name))
    with pytest.raises(NotImplementedError):
        d.training_losses(None, None, None)


# ----------------------------------------------------------------------------- round 3: repetition seeding under dist (ADVICE medium)
def test_derive_seed_separates_neighbouring_runs_repetitions_and_samples():
    from audio2photoreal_amd.sample_parallel import derive_seed
    seen = {derive_seed(b, r, g) for b in (10, 11, 12) for r in range(3) for g in range(8)}
    assert len(seen) == 3 * 3 * 8                                  # base + g collided: (10, 1) == (11, 0)
    assert derive_seed(10, 0, 1) != derive_seed(11, 0, 0)
    assert all(0 <= s < 2 ** 63 for s in seen)
    assert derive_seed(10, 2, 5) == derive_seed(10, 2, 5)


class _EchoDiffusion:
    """ddim_sample_loop that returns its initial noise: what _generate_sequences gathers IS the noise each sample started from."""

    def ddim_sample_loop(self, model, shape, noise=None, model_kwargs=None, **kw):
        assert noise is not None and tuple(noise.shape) == tuple(shape)
        return noise.clone()


def _rep_worker(rank, world, port, out_dir):
    import argparse
    import torch.distributed as dist
    from audio2photoreal_amd.sample import generate as G
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(1234)
    args = argparse.Namespace(num_repetitions=2, guidance_param=2.0, batch_size=5, device="cpu", data_format="face",
                              curr_seq_length=6, resume_trans=None)
    model = argparse.Namespace(nfeats=4)
    y = {"cond_embed": torch.zeros(5, 3, 2)}
    out = G._generate_sequences(args, {"y": y}, _EchoDiffusion(), model, lambda d, kind: d)
    np.save(os.path.join(out_dir, f"r{rank}.npy"), out["motions"])
    again = G._generate_sequences(args, {"y": y}, _EchoDiffusion(), model, lambda d, kind: d)    # the same clip a second time
    np.save(os.path.join(out_dir, f"again{rank}.npy"), again["motions"])
    dist.destroy_process_group()


def test_sharded_repetitions_draw_fresh_noise(tmp_path):
    """under torch.distributed every repetition of _generate_sequences started from the SAME noise (the shared
    base seed does not advance).  Now seed = derive_seed(base, sampling call of this process, repetition, global sample id):
    ADVICE round 3 -- two _generate_sequences calls of one process must not reuse each other's noise either."""
    from audio2photoreal_amd.sample_parallel import derive_seed
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_rep_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0, r1 = np.load(tmp_path / "r0.npy"), np.load(tmp_path / "r1.npy")
    assert np.array_equal(r0, r1) and r0.shape == (10, 4, 1, 6)
    rep0, rep1 = r0[:5], r0[5:]
    assert not np.array_equal(rep0, rep1), "repetition 1 repeated repetition 0's samples"
    want = per_sample_noise((5, 4, 1, 6), [derive_seed(1234, 0, 1, g) for g in range(5)]).numpy()
    assert np.array_equal(rep1, want)                                # a function of (base seed, call, repetition, global id) only
    a0, a1 = np.load(tmp_path / "again0.npy"), np.load(tmp_path / "again1.npy")
    assert np.array_equal(a0, a1) and not np.array_equal(a0, r0), "the second sampling call repeated the first one's noise"
    assert np.array_equal(a0[5:], per_sample_noise((5, 4, 1, 6), [derive_seed(1234, 1, 1, g) for g in range(5)]).numpy())


def _blocks_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from audio2photoreal_amd.sample_parallel import gather_blocks, gather_samples, shard_bounds
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sizes = [3, 0, 2][:world]
    mine = torch.full((sizes[rank], 2, 1, 4), float(rank)) + torch.arange(sizes[rank]).view(-1, 1, 1, 1) * 0.25
    allx = gather_blocks(mine, sizes)
    lo, hi = shard_bounds(2, world, rank)                    # 2 samples over 3 ranks: the last rank holds none
    few = gather_samples(torch.arange(lo, hi, dtype=torch.float32).view(-1, 1), 2)
    torch.save((allx, few), os.path.join(out_dir, f"b{rank}.pt"))
    dist.destroy_process_group()


def test_gather_blocks_with_a_rank_that_holds_nothing(tmp_path):
    """Strong scaling (a fixed number of samples over more ranks than samples, or an uneven subject placement) leaves ranks
    without rows: the one collective must still run on every rank and return the true blocks in rank order."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_blocks_worker, args=(3, port, str(tmp_path)), nprocs=3, join=True)
    outs = [torch.load(tmp_path / f"b{r}.pt") for r in range(3)]
    for allx, few in outs:
        assert allx.shape == (5, 2, 1, 4) and torch.equal(allx[:, 0, 0, 0], torch.tensor([0.0, 0.25, 0.5, 2.0, 2.25]))
        assert torch.equal(few, torch.tensor([[0.0], [1.0]]))


# ----------------------------------------------------------------------------- round 3: f1 honesty (ADVICE high)
def test_native_front_end_refuses_on_path_tensors_it_does_not_implement():
    """A real fairseq (vq-)wav2vec checkpoint carries GroupNorm affine terms per conv layer and, for the lip encoder, a 12-layer
    feature aggregator -- both ON the reference's conditioning path (model/diffusion.py:290-291, audio_encoder.py:43-44).  The stub
    geometry does not implement them: loading must fail loudly, not skip them.  Off-path tensors (quantiser, prediction heads,
    the vq-wav2vec aggregator encode_audio never calls) are still skipped."""
    from audio2photoreal_amd import _lib
    from audio2photoreal_amd.model_util import create_model_and_diffusion, default_args, load_model
    from audio2photoreal_amd.synthetic import synthetic_frontend_state_dict
    spec = face_spec(num_layers=1)
    model, _ = create_model_and_diffusion(default_args("face", layers=1), "test", audio_frontend="native")
    sd = {**synthetic_state_dict(spec, 10), **synthetic_frontend_state_dict(10, lip=True)}
    load_model(model, sd)                                                                     # stub-geometry weights: fine
    off_path = {"audio_model.vector_quantizer.vars": torch.zeros(1, 640, 128), "audio_model.feature_aggregator.conv_layers.0.1.weight": torch.zeros(512, 512, 2),
                "audio_model.wav2vec_predictions.project_to_steps.weight": torch.zeros(512, 512, 1, 12),
                "lip_model.audio_encoder.resampler.kernel": torch.zeros(1, 1, 41)}
    load_model(model, {**sd, **off_path})                                                     # not read by the reference on this path
    for bad in ("audio_model.feature_extractor.conv_layers.0.2.weight", "audio_model.feature_extractor.conv_layers.3.2.bias",
                "lip_model.audio_encoder.wav2vec_model.feature_extractor.conv_layers.1.2.weight",
                "lip_model.audio_encoder.wav2vec_model.feature_aggregator.conv_layers.0.1.weight"):
        with pytest.raises(_lib.A2PError, match="conditioning path"):
            load_model(model, {**sd, bad: torch.ones(512)})
    # round 4: a model built for fairseq's published blocks holds -- and consumes -- exactly those tensors ...
    from audio2photoreal_amd.model.audio_frontend import FAIRSEQ
    fq, _ = create_model_and_diffusion(default_args("face", layers=1), "test", audio_frontend="native", audio_geometry=FAIRSEQ)
    sd_fq = {**synthetic_state_dict(spec, 10), **synthetic_frontend_state_dict(10, lip=True, geometry=FAIRSEQ)}
    load_model(fq, {**sd_fq, **off_path})
    assert "lip_model.audio_encoder.wav2vec_model.feature_aggregator.conv_layers.11.3.bias" in fq.state_dict()
    assert "lip_model.audio_encoder.wav2vec_model.feature_extractor.conv_layers.7.0.weight" not in fq.state_dict()   # wav2vec-large: 7 layers
    with pytest.raises(_lib.A2PError, match="conditioning path"):        # ... and still refuses what its geometry does not have
        load_model(fq, {**sd_fq, "lip_model.audio_encoder.wav2vec_model.feature_aggregator.conv_layers.12.1.weight": torch.ones(512, 512, 14)})
    with pytest.raises(_lib.A2PError, match="conditioning path"):        # the stub model refuses the fairseq dictionary
        load_model(model, sd_fq)
    # a model WITHOUT the native front end is fed y["cond_embed"] by the caller: front-end tensors are none of its business
    plain, _ = create_model_and_diffusion(default_args("face", layers=1), "test")
    load_model(plain, {**synthetic_state_dict(spec, 10), "audio_model.feature_extractor.conv_layers.0.2.weight": torch.ones(512)})


# ----------------------------------------------------------------------------- round 5: all-pairs gather, failures reach every rank
def _p2p_worker(rank, world, port, out_dir):
    import torch.distributed as dist
    from audio2photoreal_amd.sample_parallel import gather_blocks
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    sizes = [3, 0, 2][:world] if world == 3 else [2, 3]
    mine = torch.full((sizes[rank], 2, 1, 4), float(rank)) + torch.arange(sizes[rank]).view(-1, 1, 1, 1) * 0.25
    ring = gather_blocks(mine, sizes, mode="ring")
    p2p = gather_blocks(mine, sizes, mode="p2p")
    os.environ["A2P_GATHER"] = "p2p"                          # the switch a deployment uses
    env = gather_blocks(mine, sizes)
    torch.save((ring, p2p, env), os.path.join(out_dir, f"p{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_all_pairs_gather_equals_the_ring_all_gather(tmp_path, world):
    """the end-of-run exchange as all-pairs point-to-point copies (one hop per block on xGMI's mesh) instead of
    the ring all_gather -- same bytes on every rank, including a rank that holds nothing."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_p2p_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    outs = [torch.load(tmp_path / f"p{r}.pt") for r in range(world)]
    for ring, p2p, env in outs:
        assert torch.equal(ring, outs[0][0]) and torch.equal(p2p, ring) and torch.equal(env, ring)
    assert outs[0][0].shape[0] == 5


def _failing_loop(model, shape, noise=None, model_kwargs=None, **kw):
    if float(model_kwargs["y"]["scale"][0]) > 1.5:            # only the rank that holds the last samples
        raise ValueError("non-finite values in the sampling loop (stand-in for A2PError)")
    return noise.clone()


def _fail_worker(rank, world, port, out_dir):
    import datetime
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    total = 4
    shape = (total, 4, 1, 6)
    y = {"cond_embed": torch.zeros(total, 3, 2), "scale": torch.tensor([1.0, 1.0, 2.0, 2.0])}
    t0 = __import__("time").perf_counter()
    try:
        sample_parallel(_failing_loop, None, shape, {"y": y}, noise=torch.zeros(shape))
        msg = "no exception"
    except Exception as e:   # noqa: BLE001
        msg = f"{type(e).__name__}: {e}"
    with open(os.path.join(out_dir, f"f{rank}.txt"), "w") as f:
        f.write(f"{__import__('time').perf_counter() - t0:.2f}\n{msg}")
    dist.destroy_process_group()


def test_a_failure_on_one_rank_raises_on_every_rank_before_the_gather(tmp_path):
    """check_finite() raising on one rank inside the loop left the others in the final collective until it timed out.
    Now every rank learns about it (one 4-byte all_gather in front of the data-path collective) and raises at once."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_fail_worker, args=(2, port, str(tmp_path)), nprocs=2, join=True)
    r0 = (tmp_path / "f0.txt").read_text().splitlines()
    r1 = (tmp_path / "f1.txt").read_text().splitlines()
    assert float(r0[0]) < 30 and float(r1[0]) < 30, "a rank sat in the collective until the timeout"
    assert r1[1].startswith("ValueError") and "non-finite" in r1[1]              # the failing rank re-raises its own error
    assert r0[1].startswith("RuntimeError") and "rank(s) [1] failed" in r0[1]    # the healthy rank names it


# ----------------------------------------------------------------------------- round 5: escalation control flow of the loops (no GPU)
class _EscalatingModel(torch.nn.Module):
    """Stands in for a 16-bit FiLMTransformer: `verdicts` is what its successive check_finite() calls return."""
    def __init__(self, verdicts):
        super().__init__()
        self.w = torch.nn.Parameter(torch.zeros(1))
        self.verdicts, self.checks, self.mode = list(verdicts), 0, "fp16"

    def a2p_wants_early_check(self):
        return self.mode != "fp32"

    def a2p_check_finite(self):
        self.checks += 1
        v = self.verdicts.pop(0) if self.verdicts else None
        if v == "escalated":
            self.mode = "fp32"
        return v


def _toy_step(calls):
    def step(model, img, t, model_kwargs=None, noise=None, **kw):
        calls.append((model.mode, int(t[0])))
        nz = torch.randn_like(img) if noise is None else noise          # draws from the default generator like p_sample
        bias = 0.0 if model.mode == "fp32" else 1e-2                     # "16-bit" steps are visibly different
        out = 0.5 * img + 0.1 * nz + bias
        return {"sample": out, "pred_xstart": out}
    return step


def test_loops_repeat_the_first_step_or_the_call_when_the_model_escalates():
    """A model that leaves the 16-bit envelope escalates to fp32 (FiLMTransformer.check_finite returns "escalated"): right after the
    first step -> that step is repeated, the other steps run once; at the end of the call -> the non-progressive loop repeats the whole
    call.  Either way the returned sample equals a pure-fp32 run under the same seed (same noise draws)."""
    d = create_gaussian_diffusion(default_args("face", timestep_respacing="ddim5"))
    shape = (2, 3, 1, 4)

    def run(model, calls):
        torch.manual_seed(77)
        def once():
            final = None
            for s in d._loop(_toy_step(calls), model, shape, None, {}, torch.device("cpu"), False, 0, None, False, None):
                final = s
            return final["sample"]
        return d._run_call(once, model, torch.device("cpu"))

    ref_model = _EscalatingModel([])
    ref_model.mode = "fp32"
    c0 = []
    want = run(ref_model, c0)
    assert len(c0) == 5 and ref_model.checks == 1                     # fp32: no early check, one end-of-call check

    early, c1 = _EscalatingModel(["escalated"]), []
    got = run(early, c1)
    assert torch.equal(got, want)
    assert [m for m, _ in c1] == ["fp16"] + ["fp32"] * 5 and c1[0][1] == c1[1][1]   # step 0 twice, then 4 more

    late, c2 = _EscalatingModel([None, "escalated"]), []
    got = run(late, c2)
    assert torch.equal(got, want)
    assert [m for m, _ in c2] == ["fp16"] * 5 + ["fp32"] * 5                          # the whole call repeated on fp32

    inside, c3 = _EscalatingModel([None, None]), []
    got = run(inside, c3)
    assert len(c3) == 5 and inside.checks == 2 and not torch.equal(got, want)         # stays 16-bit: one pass


# ----------------------------------------------------------------------------- round 6: precision is a property of the BATCH
class _ShardModel:
    """Stands in for a 16-bit FiLMTransformer behind sample_parallel: escalates itself when its shard holds a 'hot' sample."""
    def __init__(self):
        self.global_batch_hint, self.precision, self.escalated_from, self.runs = 0, "fp16", None, []

    def set_precision(self, p):
        self.precision = p


def _precision_loop(model, shape, noise=None, model_kwargs=None, **kw):
    hot = bool((model_kwargs["y"]["scale"] > 1.5).any()) if shape[0] else False
    if model.precision != "fp32" and hot:        # what check_finite() + _run_call do: escalate, repeat the call in fp32
        model.escalated_from, model.precision = model.precision, "fp32"
    model.runs.append(model.precision)
    return noise + (0.0 if model.precision == "fp32" else 1e-3)      # the two modes give different numbers


def _precision_worker(rank, world, port, out_dir):
    import datetime
    import warnings
    import torch.distributed as dist
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=60))
    total = 5
    shape = (total, 4, 1, 6)
    noise = per_sample_noise(shape, list(range(total)))
    y = {"cond_embed": torch.zeros(total, 3, 2), "scale": torch.tensor([1.0, 1.0, 1.0, 1.0, 2.0])}   # only the LAST rank's shard is hot
    m = _ShardModel()
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        res = sample_parallel(_precision_loop, m, shape, {"y": y}, noise=noise)
    torch.save((res, m.runs, m.precision, m.escalated_from, [str(x.message) for x in w]), os.path.join(out_dir, f"q{rank}.pt"))
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_one_escalating_shard_moves_every_rank_to_fp32(tmp_path, world):
    """each rank used to decide on escalation alone, from the logit maximum of its own shard -- some shards fp32,
    some fp16, where the 1-GPU run escalates the whole batch.  The verdict now travels with the failure flag: if any rank escalated,
    every other rank switches its replica to fp32 and repeats its shard, so the sharded result equals the single-process result."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    mp.spawn(_precision_worker, args=(world, port, str(tmp_path)), nprocs=world, join=True)
    total = 5
    shape = (total, 4, 1, 6)
    noise = per_sample_noise(shape, list(range(total)))
    y = {"cond_embed": torch.zeros(total, 3, 2), "scale": torch.tensor([1.0, 1.0, 1.0, 1.0, 2.0])}
    want = sample_parallel(_precision_loop, _ShardModel(), shape, {"y": y}, noise=noise)      # one process: the whole batch in fp32
    assert torch.equal(want, noise)
    for r in range(world):
        res, runs, prec, esc_from, warns = torch.load(tmp_path / f"q{r}.pt", weights_only=False)
        assert torch.equal(res, want), f"rank {r}: sharded result differs from the unsharded one"
        assert prec == "fp32" and esc_from == "fp16"
        if r == world - 1:
            assert runs == ["fp32"] and not warns                     # the hot shard escalated inside its own loop
        else:
            assert runs == ["fp16", "fp32"] and any("repeats its shard in fp32" in x for x in warns)


# ----------------------------------------------------------------------------- bench.py --dump-outputs
def test_bench_dump_outputs_stays_within_64_mb_with_a_fixed_sample(tmp_path):
    """`bench.py --dump-outputs DIR`: outputs that fit are written whole as float32 .npy files; larger ones as the same seeded sample of
    their elements on every run, the files together at most 64 MB."""
    import bench
    g = torch.Generator().manual_seed(0)
    small = {"sample": torch.randn(2, 4, 1, 6, generator=g, dtype=torch.float64).half(), "pred_xstart": torch.randn(2, 4, 1, 6, generator=g)}
    rec = bench.dump_outputs(str(tmp_path / "small"), small)
    for k, v in small.items():
        got = np.load(tmp_path / "small" / f"{k}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, v.float().numpy()) and "sampled_elements" not in rec[k]
    big = {"sample": torch.randn(64, 256, 1, 600, generator=g), "pred_xstart": torch.randn(64, 256, 1, 600, generator=g)}
    runs = [bench.dump_outputs(str(tmp_path / d), big) for d in ("a", "b")]
    assert runs[0] == runs[1] and runs[0]["sample"]["shape"] == [64, 256, 1, 600]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 64 * 10 ** 6
    for k, v in big.items():
        a, b = np.load(tmp_path / "a" / f"{k}.npy"), np.load(tmp_path / "b" / f"{k}.npy")
        assert np.array_equal(a, b) and a.size == runs[0][k]["sampled_elements"] > 0
        assert np.isin(a[:1000], v.numpy()).all()                  # sampled values, not recomputed ones


def test_bench_options_of_the_full_run_need_full():
    """`--write-parity` and `--cpu-all-cores` only mean something in a `--full` run: without it bench.py refuses them before it starts."""
    import subprocess
    for opt in (["--write-parity", "parity.json"], ["--cpu-all-cores"]):
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + opt, capture_output=True, text=True, timeout=120)
        assert r.returncode == 2 and "--full" in r.stderr, r.stderr[-2000:]
