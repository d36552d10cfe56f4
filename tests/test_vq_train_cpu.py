"""Tokenizer training, host side: the float64 restatement of a training step against the reference's recorded steps, its two forms
against each other, the tie rule, the learning-rate recipe, checkpoint layout, k-means, and every refusal before any GPU work."""
import ctypes
import os

import numpy as np
import pytest
import torch

import vq_train_restatement as VT
from audio2photoreal_amd import _lib
from audio2photoreal_amd._lib import A2PError
from audio2photoreal_amd.spec import TokenizerSpec
from audio2photoreal_amd.synthetic import synthetic_tokenizer_encoder_state_dict, synthetic_tokenizer_state_dict
from audio2photoreal_amd.train import tokenizer as TK

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 10
SPEC = TokenizerSpec(categories=128)
RECORD = ("loss", "loss_motion", "loss_commit", "loss_vel", "perplexity")


def load_golden():
    g = dict(np.load(os.path.join(HERE, "golden", "golden_vq_train_v1.npz")))
    g.update({"state/" + k: v for k, v in np.load(os.path.join(HERE, "golden", "golden_vq_train_state_v1.npz")).items()})
    return g


def golden_start(g, spec=SPEC, dtype=torch.float64):
    """The synthetic inited state the recorded run started from."""
    seed = int(g["weight_seed"])
    sd = {**synthetic_tokenizer_state_dict(spec, seed), **synthetic_tokenizer_encoder_state_dict(spec, seed)}
    sd["decoder.project_mean_shape.weight"] = torch.from_numpy(g["pms/weight"])
    sd["decoder.project_mean_shape.bias"] = torch.from_numpy(g["pms/bias"])
    return VT.make_state(sd, spec.residual_depth, dtype=dtype)


def golden_hyper(g, i):
    commit, loss_vel, wd = (float(v) for v in g["hyper"])
    return {"commit": commit, "loss_vel": loss_vel, "weight_decay": wd, "lr": float(g["lrs"][i])}


def run_restatement(g, manual, dtype=torch.float64):
    state, outs = golden_start(g, dtype=dtype), []
    for i in range(3):
        state, out = VT.step(state, torch.from_numpy(g["batches"][i]), golden_hyper(g, i), manual=manual)
        outs.append(out)
    return state, outs


@pytest.fixture(scope="module")
def golden():
    return load_golden()


@pytest.fixture(scope="module")
def chains(golden):
    return {m: run_restatement(golden, m) for m in (False, True)}


def rel_max(a, b):
    return float((a - b).abs().max() / b.abs().max())


def test_restatement_matches_the_recorded_steps(golden, chains):
    """Tokens exactly; losses, the first step's gradient and the state after three steps within fp32 rounding of the reference
    run (bounds: a few hundred ulp of the tensor's largest element for sums of ~2000 fp32 products; updates as (p - p0) / lr)."""
    nv, e = SPEC.n_vertices, SPEC.latent_dim
    for manual in (False, True):
        state, outs = chains[manual]
        for i, out in enumerate(outs):
            assert float(out["margins"].min()) >= 1e-3
            assert np.array_equal(out["tokens"].numpy(), golden[f"step{i}/tokens"])
            got = np.array([float(out[k]) for k in RECORD])
            assert np.abs(got - golden[f"step{i}/losses"]).max() <= 2e-6 * np.abs(got).max(), (i, got, golden[f"step{i}/losses"])
        want = VT.unflatten(torch.from_numpy(golden["step0/grads"]).double(), nv, e)
        for name, gr in outs[0]["grads"].items():
            assert rel_max(want[name], gr) < 2e-5, name
        assert not want["decoder.project_mean_shape.weight"].any() and "decoder.project_mean_shape.weight" not in outs[0]["grads"]
        start = golden_start(golden)
        lr = float(golden["lrs"].max())
        fin = VT.unflatten(torch.from_numpy(golden["state/params"]).double(), nv, e)
        m1 = VT.unflatten(torch.from_numpy(golden["state/exp_avg"]).double(), nv, e)
        m2 = VT.unflatten(torch.from_numpy(golden["state/exp_avg_sq"]).double(), nv, e)
        for name in state["exp_avg"]:
            du_want, du_got = (fin[name] - start["params"][name]) / lr, (state["params"][name] - start["params"][name]) / lr
            assert float((du_want - du_got).abs().max()) < 2e-2, name     # half an fp32 ulp of a weight of 0.5 is 3e-8 = 2e-4 lr, per step
            assert rel_max(m1[name], state["exp_avg"][name]) < 2e-5 and rel_max(m2[name], state["exp_avg_sq"][name]) < 4e-5, name
        assert torch.equal(fin["decoder.project_mean_shape.weight"], start["params"]["decoder.project_mean_shape.weight"])
        for k in range(SPEC.residual_depth):
            for n in ("embed", "embed_avg", "cluster_size"):
                assert rel_max(torch.from_numpy(golden[f"final/{n}/{k}"]).double(), state[n][k]) < 2e-6, (n, k)


def test_autograd_and_handwritten_backward_agree(chains):
    (sa, oa), (sm, om) = chains[False], chains[True]
    for a, m in zip(oa, om):
        assert torch.equal(a["tokens"], m["tokens"])
        for name in a["grads"]:
            assert rel_max(m["grads"][name], a["grads"][name]) < 1e-12, name
        for k in RECORD:
            assert abs(float(a[k]) - float(m[k])) <= 1e-12 * abs(float(a[k]))
    for name in sa["params"]:
        assert rel_max(sm["params"][name], sa["params"][name]) < 1e-12


def test_zero_velocity_weight_drops_the_term(golden):
    state = golden_start(golden)
    hp = {**golden_hyper(golden, 0), "loss_vel": 0.0}
    x = torch.from_numpy(golden["batches"][0])
    ga, oa = VT.gradients_autograd(state, x, hp)
    gm, om = VT.gradients_manual(state, x, hp)
    assert float(oa["loss_vel"]) == 0.0 and float(om["loss_vel"]) == 0.0
    assert all(rel_max(gm[n], ga[n]) < 1e-12 for n in ga)


def test_duplicate_codes_send_statistics_to_the_lowest_index(golden):
    """k-means on a first batch makes exact duplicate codes: the lowest index wins the pick and alone receives the row."""
    state = golden_start(golden)
    x = torch.from_numpy(golden["batches"][0])
    _, out = VT.step(state, x, golden_hyper(golden, 0), manual=True)
    used = int(out["tokens"][0, 0, 0])
    dup = (used + 5) % SPEC.categories
    lo, hi = min(used, dup), max(used, dup)
    for n in ("embed", "embed_avg"):
        state[n][0][hi] = state[n][0][lo] = state[n][0][used].clone()
    new, out2 = VT.step(state, x, golden_hyper(golden, 0), manual=True)
    tok = out2["tokens"][..., 0]
    assert (tok == lo).any() and not (tok == hi).any()
    assert float(new["cluster_size"][0][hi]) == pytest.approx(5 * 0.99) and float(new["cluster_size"][0][lo]) > 5 * 0.99
    assert torch.allclose(new["embed_avg"][0][hi], 0.99 * state["embed_avg"][0][hi], rtol=0, atol=1e-15)


def test_learning_rate_recipe_equals_torchs_scheduler(golden):
    lr, warm, gamma, total, *milestones = golden["sched/config"]
    want = golden["sched/lrs"]
    got = [TK.learning_rate(n, float(lr), int(warm), [int(m) for m in milestones], float(gamma)) for n in range(len(want))]
    assert len(want) == int(warm) - 1 + int(total)
    assert got == want.tolist()
    assert TK.learning_rate(0, 2e-4, 0, [5], 0.5) == 2e-4 and TK.learning_rate(5, 2e-4, 1, [5], 0.5) == 1e-4


def test_kmeans_reproduces_the_recorded_means(golden):
    for case in ("many", "few"):
        samples, start = torch.from_numpy(golden[f"kmeans/{case}/samples"]), torch.from_numpy(golden[f"kmeans/{case}/start"])
        means, bins = VT.kmeans(samples, start)
        assert np.array_equal(bins.numpy(), golden[f"kmeans/{case}/bins"])
        assert np.abs(means.numpy() - golden[f"kmeans/{case}/means"]).max() < 1e-6
        means2, bins2 = TK.kmeans(samples.double(), len(start), None, start=start.double())
        assert torch.equal(bins2, bins) and float((means2 - means).abs().max()) < 1e-12
    assert (golden["kmeans/few/bins"] == 0).any()          # empty clusters kept their starting mean
    g = torch.Generator().manual_seed(3)
    a, _ = TK.kmeans(torch.from_numpy(golden["kmeans/many/samples"]), 16, g)
    b, _ = TK.kmeans(torch.from_numpy(golden["kmeans/many/samples"]), 16, torch.Generator().manual_seed(3))
    assert torch.equal(a, b)


def test_checkpoint_keys_and_layout(golden):
    """The flat layout is parameters() order of the reference codec, and the recorded key list is what `net` must carry."""
    keys = [str(k) for k in golden["state_dict_keys"]]
    names = [n for n, _ in TK.param_shapes(SPEC.n_vertices, SPEC.latent_dim)]
    assert names == [n for n, _ in VT.param_shapes(SPEC.n_vertices, SPEC.latent_dim)]
    assert [k for k in keys if k.startswith(("encoder.", "decoder."))] == names
    books = {f"quantizer.layers.{k}._codebook.{n}" for k in range(SPEC.residual_depth) for n in ("inited", "cluster_size", "embed", "embed_avg")}
    assert set(keys) == set(names) | books
    assert sum(int(np.prod(s)) for _, s in TK.param_shapes(104, 64)) == golden["state/params"].size
    assert TK.tokenizer_args(TokenizerSpec()) == {"nb_joints": 104, "output_emb_width": 64, "code_dim": 1024, "depth": 4}


def test_refusals_need_no_gpu(tmp_path):
    with pytest.raises(A2PError, match="pose"):
        TK.TokenizerTrainer(TokenizerSpec(), data_format="face")
    with pytest.raises(A2PError, match="pose"):
        TK.train_tokenizer(str(tmp_path), str(tmp_path / "out"), data_format="face")
    with pytest.raises(A2PError, match="multiple of 4"):
        TK.TokenizerTrainer(TokenizerSpec(latent_dim=30))
    with pytest.raises(A2PError, match="depth"):
        TK.TokenizerTrainer(TokenizerSpec(residual_depth=9))
    with pytest.raises(A2PError, match="lr"):
        TK.TokenizerTrainer(TokenizerSpec(), lr=float("nan"))
    with pytest.raises(A2PError, match="milestones"):
        TK.TokenizerTrainer(TokenizerSpec(), milestones=[0])
    with pytest.raises(A2PError, match="MI355X"):
        TK.TokenizerTrainer(TokenizerSpec(), device="cpu")
    assert TK.max_rows(64) == 120
    TK.check_batch(torch.zeros(2, 120, 104), 104, 64)
    with pytest.raises(A2PError, match="at most 120"):
        TK.check_batch(torch.zeros(2, 121, 104), 104, 64)
    with pytest.raises(A2PError, match="at most 120"):
        TK.check_batch(torch.zeros(1, 600, 104), 104, 64)          # a frame-rate sequence
    for bad in (torch.zeros(2, 20, 103), torch.zeros(20, 104), torch.zeros(0, 20, 104), np.zeros((2, 20, 104)), torch.zeros(2, 20, 104, dtype=torch.int64)):
        with pytest.raises(A2PError, match="keyframes"):
            TK.check_batch(bad, 104, 64)
    x = torch.zeros(2, 20, 104)
    x[1, 3, 7] = float("inf")
    with pytest.raises(A2PError, match="non-finite"):
        TK.check_batch(x, 104, 64)
    with pytest.raises(A2PError, match="batch_size"):
        TK.train_tokenizer(str(tmp_path), str(tmp_path / "out"), batch_size=0)
    with pytest.raises(A2PError, match="data_stats"):
        TK.train_tokenizer(str(tmp_path), str(tmp_path / "out"))
    with pytest.raises(SystemExit):
        TK.main(["--data_root", "x"])                              # --out_dir is required, as in the reference's parser
    a = TK._parser().parse_args(["--out_dir", "o"])
    assert (a.code_dim, a.depth, a.output_emb_width, a.batch_size, a.total_iter, a.warm_up_iter, a.lr, a.lr_scheduler, a.gamma,
            a.commit, a.loss_vel, a.weight_decay, a.print_iter, a.eval_iter, a.seed) == (
        512, 3, 512, 64, 300000, 1000, 2e-4, [300000], 0.05, 0.02, 0.1, 0.0, 200, 1000, 123)


def test_both_libraries_export_the_training_entries():
    assert {"a2p_vq_train_step", "a2p_vq_train_workspace_bytes"} <= set(_lib.EXPORTS)
    header = open(os.path.join(os.path.dirname(HERE), "include", "a2p_hip.h")).read()
    assert "int a2p_vq_train_step(" in header and "int a2p_vq_train_workspace_bytes(" in header
    built = [p for p in (_lib.LIB_PATH, _lib.LIB_PATH_F16) if os.path.exists(p)]
    for path in built:
        lib = ctypes.CDLL(path)
        assert hasattr(lib, "a2p_vq_train_step") and hasattr(lib, "a2p_vq_train_workspace_bytes"), path
    if built:       # the plan needs no device: sizes and the LDS refusal
        lib = _lib.load()
        n = ctypes.c_int64(0)
        assert lib.a2p_vq_train_workspace_bytes(64, 20, 4, 1024, 64, 104, ctypes.byref(n)) == 0 and n.value > 0
        assert lib.a2p_vq_train_workspace_bytes(1, 121, 4, 1024, 64, 104, ctypes.byref(n)) < 0
        assert b"LDS" in lib.a2p_last_error()
        assert lib.a2p_vq_train_workspace_bytes(1, 120, 4, 1024, 64, 104, ctypes.byref(n)) == 0
        assert lib.a2p_vq_train_workspace_bytes(1, 20, 9, 1024, 64, 104, ctypes.byref(n)) < 0
        _lib._failed.clear()
