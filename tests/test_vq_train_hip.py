"""The fused tokenizer training step on the MI355X (a2p_vq_train_step, audio2photoreal_amd.train.tokenizer).

Every float gate is 4 x the distance of an fp32 CPU run from the float64 restatement (tests/vq_train_restatement.py), computed
here and never hard-coded: for the recorded steps that fp32 run is the reference's own (tests/golden/golden_vq_train_v1.npz), for
the edge shapes it is the restatement itself run in fp32 (counted as at least one fp32 ulp: test_edge_shapes_against_float64).  Gradients, moments and codebook state are compared per tensor
relative to the tensor's max |.|; parameters as updates (p - p0) / lr in absolute terms (Adam turns tiny gradients into O(lr)
moves).  Tokens are exact: every fixture's picks have a float64 top-2 margin >= 1e-3 and no LeakyReLU pre-activation within
100 fp32 errors of 0, which the tests assert.  Measured errors go to record(...) beside their gates (vq_train_* entries); on an
MI355X the recorded steps gave, worst tensor as error / gate: losses 7.8e-8 / 3.1e-7, gradient 5.7e-8 / 4.3e-7, updates 7.7e-4 /
1.8e-3, exp_avg 3.0e-7 / 6.2e-7, exp_avg_sq 5.7e-7 / 6.2e-7, embed 1.5e-7 / 5.4e-7, embed_avg 1.1e-7 / 4.5e-7, cluster_size 1.0e-7 /
1.3e-7."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

import dataset_restatement as R
import vq_train_restatement as VT
from audio2photoreal_amd import _lib
from audio2photoreal_amd.model.vqvae import TemporalVertexCodec
from audio2photoreal_amd.spec import TokenizerSpec
from audio2photoreal_amd.synthetic import synthetic_tokenizer_encoder_state_dict, synthetic_tokenizer_state_dict
from audio2photoreal_amd.train import tokenizer as TK
from conftest import record
from test_vq_train_cpu import RECORD, SPEC, golden_hyper, golden_start, load_golden, run_restatement

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD, SENTINEL = 64, 1234.5
BOOK = ("embed", "embed_avg", "cluster_size")


@pytest.fixture(scope="module")
def golden():
    return load_golden()


@pytest.fixture(scope="module")
def chain64(golden):
    return run_restatement(golden, manual=False)


class DeviceState:
    """The flat buffers of a2p_vq_train_step, each inside guard elements, filled from a restatement state."""

    def __init__(self, state, spec):
        self.spec, self.whole = spec, {}
        nv, e = spec.n_vertices, spec.latent_dim
        self.params = self._guarded("params", VT.flatten(state["params"], nv, e))
        self.m1 = self._guarded("m1", VT.flatten(state["exp_avg"], nv, e))
        self.m2 = self._guarded("m2", VT.flatten(state["exp_avg_sq"], nv, e))
        for n in BOOK:
            setattr(self, n, self._guarded(n, torch.stack(state[n])))
        self.record = self._guarded("record", torch.zeros(6))
        self.step_no = state["step"]

    def _guarded(self, name, value, dtype=torch.float32):
        sentinel = SENTINEL if dtype.is_floating_point else 165
        whole = torch.full((value.numel() + 2 * GUARD,), sentinel, dtype=dtype, device=DEV)
        view = whole[GUARD:GUARD + value.numel()].view(value.shape)
        view.copy_(value.to(dtype))
        self.whole[f"{name}{len(self.whole)}"] = (whole, sentinel)
        return view

    def guards_intact(self):
        return all(bool((w[:GUARD] == s).all()) and bool((w[-GUARD:] == s).all()) for w, s in self.whole.values())

    def step(self, x, hp, grads=False):
        """One a2p_vq_train_step; returns (tokens, the step's five loss scalars + count, the gradient or None)."""
        s, lib = self.spec, _lib.load()
        B, T, _ = x.shape
        n = C.c_int64(0)
        _lib.check(lib.a2p_vq_train_workspace_bytes(B, T, s.residual_depth, s.categories, s.latent_dim, s.n_vertices, C.byref(n)), "ws")
        ws = self._guarded("ws", torch.zeros(n.value), torch.uint8)
        tokens = self._guarded("tokens", torch.zeros(B, T, s.residual_depth), torch.int64)
        g = self._guarded("grads", torch.zeros(self.params.numel())) if grads else None
        xd = self._guarded("x", x)
        self.step_no += 1
        hyper = _lib.A2PVqTrainHyper(hp["lr"], 1 - 0.9 ** self.step_no, 1 - 0.99 ** self.step_no, hp["weight_decay"], hp["commit"],
                                     hp["loss_vel"], 0.99, 1e-5)
        ptrs = lambda t: (C.c_void_p * t.shape[0])(*[t[k].data_ptr() for k in range(t.shape[0])])       # noqa: E731
        self.record.zero_()
        _lib.check(lib.a2p_vq_train_step(xd.data_ptr(), B, T, s.residual_depth, s.categories, s.latent_dim, s.n_vertices,
                                         self.params.data_ptr(), self.m1.data_ptr(), self.m2.data_ptr(), ptrs(self.embed),
                                         ptrs(self.embed_avg), ptrs(self.cluster_size), C.byref(hyper), tokens.data_ptr(),
                                         self.record.data_ptr(), _lib.ptr(g), ws.data_ptr(), n.value,
                                         _lib.current_stream(torch.device(DEV))), "a2p_vq_train_step")
        torch.cuda.synchronize()
        assert bool((xd.cpu() == x).all())
        return tokens.cpu(), self.record.cpu().double(), None if g is None else g.cpu().double()

    def bits(self):
        return [t.cpu().clone() for t in (self.params, self.m1, self.m2, self.embed, self.embed_avg, self.cluster_size)]


def per_tensor(flat, nv, e):
    return {n: t for n, t in VT.unflatten(flat.double().cpu().reshape(-1), nv, e).items() if VT.trainable(n)}


def rel_err(a, ref):
    return float((a - ref).abs().max() / ref.abs().max())


ULP = 2.0 ** -23


def gate_all(name, got, base, ref, metric, floor=None):
    """got / base / ref: {key: tensor} of the GPU, the fp32 CPU run and float64.  Asserts metric(got) <= 4 metric(base) per key;
    every key's figures are recorded before the first assertion.  `floor` ({key: value}, edge shapes only): the fp32 run's
    distance is taken as at least that -- see test_edge_shapes_against_float64."""
    rows = {str(k): (metric(got[k], ref[k]), 4 * max(metric(base[k], ref[k]), floor[k] if floor else 0.0)) for k in ref}
    worst = max(rows, key=lambda k: rows[k][0] / rows[k][1] if rows[k][1] else (float("inf") if rows[k][0] else 0.0))
    record(f"vq_train_{name}", worst_key=worst, err=rows[worst][0], gate=rows[worst][1], max_err=max(r[0] for r in rows.values()))
    print(f"vq_train_{name}: worst {worst} err {rows[worst][0]:.3e} gate {rows[worst][1]:.3e}")
    for k, (err, allow) in rows.items():
        assert err <= allow, (name, k, err, allow)


def compare_run(tag, spec, dev_state, start, final64, final32, lr, ulp_floor=False):
    """Final state of a GPU run against float64, gated by the fp32 CPU run's distance (`ulp_floor`: at least one fp32 ulp of the
    tensor's largest element, for parameters of the largest parameter over lr)."""
    nv, e = spec.n_vertices, spec.latent_dim
    p0 = per_tensor(VT.flatten(start["params"], nv, e), nv, e)
    upd = lambda flat: {n: (t - p0[n]) / lr for n, t in per_tensor(flat, nv, e).items()}          # noqa: E731
    absmax = lambda a, b: float((a - b).abs().max())                                               # noqa: E731
    gate_all(f"{tag}_update", upd(dev_state.params), upd(VT.flatten(final32["params"], nv, e)), upd(VT.flatten(final64["params"], nv, e)), absmax,
             {n: ULP * float(t.abs().max()) / lr for n, t in p0.items()} if ulp_floor else None)
    one_ulp = lambda keys: {k: ULP for k in keys} if ulp_floor else None                           # noqa: E731
    for nm, attr in (("exp_avg", "m1"), ("exp_avg_sq", "m2")):
        gate_all(f"{tag}_{nm}", per_tensor(getattr(dev_state, attr), nv, e), per_tensor(VT.flatten(final32[nm], nv, e), nv, e),
                 per_tensor(VT.flatten(final64[nm], nv, e), nv, e), rel_err, one_ulp(p0))
    for n in BOOK:
        lv = lambda seq: {k: t.double().cpu() for k, t in enumerate(seq)}                          # noqa: E731
        gate_all(f"{tag}_{n}", lv(getattr(dev_state, n)), lv(final32[n]), lv(final64[n]), rel_err, one_ulp(range(spec.residual_depth)))


def golden_final32(golden):
    nv, e = SPEC.n_vertices, SPEC.latent_dim
    f = lambda k: VT.unflatten(torch.from_numpy(golden[k]).double(), nv, e)                        # noqa: E731
    st = {"params": f("state/params"), "exp_avg": f("state/exp_avg"), "exp_avg_sq": f("state/exp_avg_sq")}
    for n in BOOK:
        st[n] = [torch.from_numpy(golden[f"final/{n}/{k}"]).double() for k in range(SPEC.residual_depth)]
    return st


def golden_net_sd(golden):
    """The recorded run's starting state as a reference-layout `net` dictionary."""
    seed = int(golden["weight_seed"])
    sd = {**synthetic_tokenizer_state_dict(SPEC, seed), **synthetic_tokenizer_encoder_state_dict(SPEC, seed)}
    sd["decoder.project_mean_shape.weight"], sd["decoder.project_mean_shape.bias"] = torch.from_numpy(golden["pms/weight"]), torch.from_numpy(golden["pms/bias"])
    for k in range(SPEC.residual_depth):
        p = f"quantizer.layers.{k}._codebook."
        sd[p + "inited"], sd[p + "embed_avg"], sd[p + "cluster_size"] = torch.ones(1), 5 * sd[p + "embed"], torch.full((SPEC.categories,), 5.0)
    return sd


# ------------------------------------------------------------------------------------------------ 1. the recorded steps
def test_three_recorded_steps(golden, chain64):
    nv, e = SPEC.n_vertices, SPEC.latent_dim
    final64, outs64 = chain64
    start = golden_start(golden)
    ds = DeviceState(start, SPEC)
    pms0 = per_tensor_all(ds.params, nv, e)
    loss_err, loss_gate = 0.0, 0.0
    for i in range(3):
        x = torch.from_numpy(golden["batches"][i])
        tokens, rec, g = ds.step(x, golden_hyper(golden, i), grads=(i == 0))
        assert torch.equal(tokens, torch.from_numpy(golden[f"step{i}/tokens"]))                    # exact at every pick
        assert float(rec[5]) == 1.0
        want = np.array([float(outs64[i][k]) for k in RECORD])
        loss_err = max(loss_err, float(np.abs(rec[:5].numpy() - want).max() / np.abs(want).max()))
        loss_gate = max(loss_gate, 4 * float(np.abs(golden[f"step{i}/losses"].astype(np.float64) - want).max() / np.abs(want).max()))
        if i == 0:
            gate_all("golden_grad", per_tensor(g, nv, e), per_tensor(torch.from_numpy(golden["step0/grads"]), nv, e),
                     per_tensor(VT.flatten(outs64[0]["grads"], nv, e), nv, e), rel_err)
            pms = slice(*pms_range(nv, e))
            assert bool((g[pms] == 0).all())                                                        # the zero-filled buffer stays as it was
    record("vq_train_golden_losses", err=loss_err, gate=loss_gate)
    assert loss_err <= loss_gate
    compare_run("golden", SPEC, ds, start, final64, golden_final32(golden), float(golden["lrs"].max()))
    # 4. untouched memory
    assert ds.guards_intact()
    after = per_tensor_all(ds.params, nv, e)
    for n in ("decoder.project_mean_shape.weight", "decoder.project_mean_shape.bias"):
        assert torch.equal(after[n], pms0[n])
        assert not per_tensor_all(ds.m1, nv, e)[n].any() and not per_tensor_all(ds.m2, nv, e)[n].any()
    # the same run through TokenizerTrainer.step gives the C-ABI run's bits
    tr = TK.TokenizerTrainer(SPEC, lr=2e-4, weight_decay=float(golden["hyper"][2]), commit=float(golden["hyper"][0]),
                             loss_vel=float(golden["hyper"][1]), warm_up_iter=4, milestones=[100], device=DEV)
    tr.load_net(golden_net_sd(golden))
    for i in range(3):
        assert tr.current_lr() == float(golden["lrs"][i])
        tok = tr.step(torch.from_numpy(golden["batches"][i]))
        assert torch.equal(tok.cpu(), torch.from_numpy(golden[f"step{i}/tokens"]))
    for a, b in zip(ds.bits(), [tr.params, tr.exp_avg, tr.exp_avg_sq, tr.embed, tr.embed_avg, tr.cluster_size]):
        assert torch.equal(a, b.cpu())
    m = tr.losses()
    assert m["steps"] == 3 and np.isfinite(m["loss"]) and tr.losses()["steps"] == 0


def pms_range(nv, e):
    o = 0
    for n, sh in VT.param_shapes(nv, e):
        if n == "decoder.project_mean_shape.weight":
            return o, o + e * nv + e
        o += int(np.prod(sh))


def per_tensor_all(flat, nv, e):
    return {n: t.clone() for n, t in VT.unflatten(flat.detach().cpu().reshape(-1), nv, e).items()}


# ------------------------------------------------------------------------------------------------ 2. determinism
def test_same_state_same_bits(golden):
    x, hp = torch.from_numpy(golden["batches"][0]), golden_hyper(golden, 0)
    runs = []
    for grads in (False, False, True):
        ds = DeviceState(golden_start(golden), SPEC)
        tok, rec, _ = ds.step(x, hp, grads=grads)
        tok2, rec2, _ = ds.step(x, hp, grads=grads)
        runs.append(ds.bits() + [tok, tok2, rec.float(), rec2.float()])
        assert ds.guards_intact()
    for other in runs[1:]:
        assert all(torch.equal(a, b) for a, b in zip(runs[0], other))


# ------------------------------------------------------------------------------------------------ 3. edge shapes
SMALL = TokenizerSpec(n_vertices=10, latent_dim=8, categories=70, residual_depth=2)
EDGE = {       # name: (spec, T, seed of the weights, seed of each sequence): chosen on the CPU so that the conditions below hold
    "short": (SMALL, 5, 10, (0, 1, 2)),
    "one_row": (SMALL, 1, 10, (0, 1, 2)),
    "pipeline_books": (TokenizerSpec(), 20, 98, (130, 140)),
}
EDGE_HP = {"commit": 0.02, "loss_vel": 0.1, "weight_decay": 0.01, "lr": 1e-4}


def edge_fixture(name):
    spec, T, weight_seed, seeds = EDGE[name]
    sd = {**synthetic_tokenizer_state_dict(spec, weight_seed), **synthetic_tokenizer_encoder_state_dict(spec, weight_seed)}
    rng = np.random.default_rng(weight_seed)
    sd["decoder.project_mean_shape.weight"] = torch.from_numpy(rng.standard_normal((spec.latent_dim, spec.n_vertices)).astype(np.float32))
    sd["decoder.project_mean_shape.bias"] = torch.from_numpy(rng.standard_normal(spec.latent_dim).astype(np.float32))
    x = torch.from_numpy(np.stack([np.random.default_rng(s).standard_normal((T, spec.n_vertices)).astype(np.float32) for s in seeds]))
    return spec, sd, x


def edge_conditions(spec, sd, x):
    """(state64, final64, out64, final32, out32, min margin, min |pre-activation|, max fp32 - float64 pre-activation difference)."""
    s64, s32 = VT.make_state(sd, spec.residual_depth), VT.make_state(sd, spec.residual_depth, dtype=torch.float32)
    f64, o64 = VT.step(s64, x, EDGE_HP)
    f32, o32 = VT.step(s32, x, EDGE_HP)
    o64["preacts"], o32["preacts"] = [t.detach() for t in o64["preacts"]], [t.detach() for t in o32["preacts"]]
    diff = max(float((a.double() - b).abs().max()) for a, b in zip(o32["preacts"], o64["preacts"]))
    near = min(float(t.abs().min()) for t in o64["preacts"] + o32["preacts"])
    return s64, f64, o64, f32, o32, float(o64["margins"].min()), near, diff


@pytest.mark.parametrize("name", list(EDGE))
def test_edge_shapes_against_float64(name):
    """No recorded reference run exists at these shapes: the yardstick is the restatement itself run in fp32 on the CPU, with the
    recorded steps' factor 4.  One amendment, from the number format and not from the kernels: with tensors of 8 to 80 elements the
    fp32 run's largest error is sometimes under half an ulp by chance, while any fp32 value that went through two or more rounded
    operations (a gradient, then its square times 1 - beta2, then the moment) may be a whole ulp off however it is computed.  So
    the fp32 run's distance counts as at least one fp32 ulp (2^-23) of the tensor's largest element."""
    spec, sd, x = edge_fixture(name)
    nv, e = spec.n_vertices, spec.latent_dim
    s64, f64, o64, f32, o32, margin, near, diff = edge_conditions(spec, sd, x)
    assert margin >= 1e-3 and near >= 100 * diff, (margin, near, diff)       # the fixture's conditions, as the recorded run's
    assert torch.equal(o32["tokens"], o64["tokens"])
    ds = DeviceState(s64, spec)
    tokens, rec, g = ds.step(x, EDGE_HP, grads=True)
    assert torch.equal(tokens, o64["tokens"])
    want = np.array([float(o64[k]) for k in RECORD])
    base = np.array([float(o32[k]) for k in RECORD])
    err, gate = float(np.abs(rec[:5].numpy() - want).max() / np.abs(want).max()), 4 * max(float(np.abs(base - want).max() / np.abs(want).max()), ULP)
    record(f"vq_train_{name}_losses", err=err, gate=gate)
    assert err <= gate
    gate_all(f"{name}_grad", per_tensor(g, nv, e), per_tensor(VT.flatten(o32["grads"], nv, e), nv, e),
             per_tensor(VT.flatten(o64["grads"], nv, e), nv, e), rel_err, {n: ULP for n in o64["grads"]})
    compare_run(name, spec, ds, s64, f64, f32, EDGE_HP["lr"], ulp_floor=True)
    assert ds.guards_intact()
    a, b = pms_range(nv, e)
    assert torch.equal(ds.params.cpu()[a:b], VT.flatten(s64["params"], nv, e).float()[a:b])


# ------------------------------------------------------------------------------------------------ 5. overfit
OVERFIT_LR = 2e-3
OVERFIT_STEPS = 150     # chosen on the CPU: the float64 restatement (same init, lr, batch) is below a quarter of its first loss_motion from step 133 on


def overfit_batch():
    rng = np.random.default_rng(31)
    return torch.from_numpy(rng.standard_normal((4, 20, SPEC.n_vertices)).astype(np.float32))


def test_overfit_one_batch():
    tr = TK.TokenizerTrainer(SPEC, lr=OVERFIT_LR, weight_decay=0.0, commit=0.02, loss_vel=0.0, warm_up_iter=0, milestones=[10 ** 6], device=DEV)
    x = overfit_batch().to(DEV)
    tr.init_codebooks(x, seed=3)
    tr.step(x)
    first = tr.losses()["loss_motion"]
    for _ in range(OVERFIT_STEPS - 2):
        tr.step(x)
    tr.losses()
    tr.step(x)
    last = tr.losses()["loss_motion"]
    record("vq_train_overfit", first=first, last=last, steps=OVERFIT_STEPS)
    assert np.isfinite(first) and last < 0.5 * first


# ------------------------------------------------------------------------------------------------ 6. round trip
def test_checkpoint_round_trip(golden, tmp_path):
    def fresh():
        t = TK.TokenizerTrainer(SPEC, lr=2e-4, weight_decay=0.01, warm_up_iter=3, milestones=[2], device=DEV)
        t.load_net(golden_net_sd(golden))
        return t
    xs = [torch.from_numpy(golden["batches"][i]).to(DEV) for i in range(3)]
    a = fresh()
    a.step(xs[0]), a.step(xs[1])
    path = a.save(str(tmp_path), "net_last.pth")
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert set(ckpt) == {"net", "optimizer", "scheduler"} and list(ckpt["net"]) and isinstance(ckpt["scheduler"], dict)
    assert set(ckpt["net"]) == {str(k) for k in golden["state_dict_keys"]}
    args = json.load(open(tmp_path / "args.json"))
    assert (args["nb_joints"], args["output_emb_width"], args["code_dim"], args["depth"]) == (104, 64, 128, 4)
    # torch's own AdamW accepts the optimizer dictionary
    ref_params = [torch.nn.Parameter(torch.zeros(s)) for _, s in a.shapes]
    torch.optim.AdamW(ref_params, lr=1.0, betas=(0.9, 0.99)).load_state_dict(ckpt["optimizer"])
    # the inference codec reads `net` (it has no EMA statistics or project_mean_shape: those keys are the only unexpected ones)
    codec = TemporalVertexCodec(104, 64, 128, 4, with_encoder=True)
    res = codec.load_state_dict(ckpt["net"], strict=False)
    assert not res.missing_keys
    assert all("project_mean_shape" in k or k.endswith(("inited", "cluster_size", "embed_avg")) for k in res.unexpected_keys)
    codec = codec.to(DEV)
    tok = codec.encode(xs[2])
    assert torch.equal(tok, a.codec.encode(xs[2])) and torch.equal(codec.decode(tok), a.codec.decode(tok))
    assert torch.equal(a.codec.encoder(xs[2]), codec.encoder(xs[2]))
    # resume: a further step equals the uninterrupted run's
    b = fresh()
    b.load(path)
    assert b.iteration == 2 and b.current_lr() == a.current_lr()
    ta, tb = a.step(xs[2]), b.step(xs[2])
    assert torch.equal(ta, tb)
    for u, v in ((a.params, b.params), (a.exp_avg, b.exp_avg), (a.exp_avg_sq, b.exp_avg_sq), (a.embed, b.embed),
                 (a.embed_avg, b.embed_avg), (a.cluster_size, b.cluster_size)):
        assert torch.equal(u, v)
    # the codec's views follow the step: encode now differs from the saved weights' only through the new weights
    assert torch.equal(a.codec.encode(xs[2]), b.codec.encode(xs[2]))


# ------------------------------------------------------------------------------------------------ 7. the recipe
def test_train_tokenizer_on_a_tiny_capture(tmp_path):
    d = R.write_capture(str(tmp_path), "PXB184", lengths=(130, 100, 100, 100, 100, 100, 100), seed=5, skipped_take=None)
    torch.save(R.golden_stats(), os.path.join(d, "data_stats.pth"))
    out = str(tmp_path / "run")
    spec = TokenizerSpec(categories=16, residual_depth=2)
    tr = TK.train_tokenizer(d, out, spec=spec, batch_size=4, total_iter=4, warm_up_iter=3, print_iter=2, eval_iter=2, seed=7,
                            max_seq_length=90, device=DEV)
    assert tr.iteration == 6
    for f in ("net_last.pth", "net_best.pth", "args.json", "run.log"):
        assert os.path.isfile(os.path.join(out, f)), f
    log = open(os.path.join(out, "run.log")).read()
    assert "Warmup. Iter 2 :" in log and "Train. Iter 4 :" in log and "Eval. Iter 0 :" in log and "Eval. Iter 4 :" in log
    args = json.load(open(os.path.join(out, "args.json")))
    assert (args["nb_joints"], args["output_emb_width"], args["code_dim"], args["depth"]) == (104, 64, 16, 2)
    from audio2photoreal_amd.data import CaptureBatches, load_capture, split_indices
    takes = load_capture(d)
    val = CaptureBatches([takes[i] for i in split_indices(len(takes))["val"]], R.golden_stats(), "pose", T=90, seed=7, device=DEV)
    m = tr.evaluate(val.batch([i])[1]["y"]["keyframes"] for i in range(len(val)))
    assert m["sequences"] == len(val) and all(np.isfinite(m[k]) for k in ("recons", "commit", "perplexity"))
    ckpt = torch.load(os.path.join(out, "net_last.pth"), map_location="cpu", weights_only=False)
    assert ckpt["scheduler"]["iteration"] == 6 and float(ckpt["net"]["quantizer.layers.0._codebook.inited"]) == 1.0
