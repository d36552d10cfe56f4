"""Round-3 GPU tests (`pytest -m gpu`): the multi-GPU control flow of bench.py on the GPU that exists, a device-tensor all_gather
that lights up on a node with >= 2 GPUs, the small-forward kernels and the key-split attention.  (The bit-identity tests of the
generation-2 / -3 chain kernels left with those kernels in round 4: neither beat generation 1 inside the step, docs/lab_notebook_r1_r4.md 4.1c.)"""
import json
import os
import socket
import subprocess
import sys

import pytest
import torch

from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel
from audio2photoreal_amd.model_util import create_model_and_diffusion, default_args, load_model
from audio2photoreal_amd.spec import face_spec, pose_spec
from audio2photoreal_amd.synthetic import synthetic_inputs, synthetic_state_dict
from conftest import ROOT, record

pytestmark = pytest.mark.gpu
SEED = 10


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _model(fmt, precision, dev, B):
    spec = face_spec() if fmt == "face" else pose_spec()
    model, _ = create_model_and_diffusion(default_args(fmt), "test", precision=precision, max_batch=B)
    load_model(model, synthetic_state_dict(spec, SEED))
    return spec, model.to(dev).eval()


def _inputs(spec, fmt, B, T, dev):
    inp = synthetic_inputs(spec, B, T, SEED)
    y = {"cond_embed": inp["cond_embed"].to(dev), "scale": torch.full((B,), 10.0 if fmt == "face" else 2.0, device=dev)}
    if spec.is_pose:
        y["keyframes"], y["mask"] = inp["keyframes"].to(dev), inp["mask"].to(dev)
    t = torch.tensor(([901, 417, 33, 0] * 8)[:B], device=dev)
    return inp["x_T"].to(dev), t, y


# ----------------------------------------------------------------------------- multi-GPU readiness
def test_bench_two_ranks_sharing_the_gpu(tmp_path):
    """bench.py's own N > 1 branch (shard_bounds, barrier + max-over-ranks timing, the single end-of-run gather) with two ranks on
    the one GPU of the test box and gloo collectives; on a multi-GPU node the driver runs the same code with backend "nccl"."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, A2P_BENCH_SHARE_GPU="1", A2P_BENCH_BACKEND="gloo", A2P_TUNE_VERBOSE="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "1", "--repeats", "1",
           "--batch", "2", "--no-cpu-baseline", "--no-legs", "--no-kernel-timing"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["scaling"] == "weak" and line["config"]["global_batch"] == 4
    assert line["gather_ms"] is not None and line["gather_ms"] > 0.0          # the one collective of the data path ran
    assert line["value"] > 0 and line["steps"] == 4
    record("bench_2ranks_shared_gpu", value=float(line["value"]), gather_ms=float(line["gather_ms"]))


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (lights up on the driver's multi-GPU node)")
def test_device_tensor_all_gather_over_rccl(tmp_path):
    """gather_samples on DEVICE tensors with backend "nccl" (= RCCL over xGMI): the collective production runs."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    code = (
        "import os, torch, torch.distributed as dist\n"
        "from audio2photoreal_amd.sample_parallel import gather_samples, shard_bounds\n"
        "r = int(os.environ['LOCAL_RANK']); torch.cuda.set_device(r); dev = torch.device('cuda', r)\n"
        "dist.init_process_group('nccl', device_id=dev)\n"
        "lo, hi = shard_bounds(5, 2, r)\n"
        "mine = torch.arange(lo, hi, device=dev, dtype=torch.float32).view(-1, 1, 1, 1).expand(-1, 4, 1, 6).contiguous()\n"
        "allx = gather_samples(mine, 5)\n"
        "assert allx.is_cuda and allx.shape == (5, 4, 1, 6) and torch.equal(allx[:, 0, 0, 0].cpu(), torch.arange(5.))\n"
        "dist.barrier(); dist.destroy_process_group()\n")
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    script = tmp_path / "w.py"
    script.write_text(code)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(script)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]


# ----------------------------------------------------------------------------- small forwards (BASELINE configs[0] shape)
@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("B,T", [(1, 240), (1, 150), (2, 100), (1, 30)])
def test_small_forward_kernels_match_the_per_op_kernels_and_the_oracle(dev, B, T, precision, monkeypatch):
    """Forwards below 1100 rows (config 0: B=1, T=240 -> 480 rows) run the decoder layers as whole-K-resident small-tile GEMMs with the
    LayerNorm fused into the A load and [Q|K] + V^T in one launch (csrc/kernels_small.h).  Same operands, same MFMA shape and
    k-order as the per-op kernels they replace: the two paths must agree to operand rounding (they are bit-identical where the
    compiler contracts the LayerNorm arithmetic alike), and both sit at the precision's distance from the fp32 oracle.  T = 150 and
    T = 30 exercise the row-by-row V^T store and ragged row blocks."""
    from oracle import a2p_oracle as O
    spec, model = _model("face", precision, dev, B)
    cfg = ClassifierFreeSampleModel(model)
    x, t, y = _inputs(spec, "face", B, T, dev)
    assert 2 * B * T < 960
    monkeypatch.delenv("A2P_NO_SMALL", raising=False)
    small = cfg(x, t, y).cpu()
    monkeypatch.setenv("A2P_NO_SMALL", "1")
    per_op = cfg(x, t, y).cpu()
    monkeypatch.delenv("A2P_NO_SMALL")
    inp = synthetic_inputs(spec, B, T, SEED)
    den = O.OracleDenoiser(synthetic_state_dict(spec, SEED), "face", spec.num_layers, spec.num_heads)
    with torch.no_grad():
        want = den.forward_cfg(inp["x_T"], t.cpu(), inp["cond_embed"], torch.full((B,), 10.0))
    rel = lambda a, b: float((a - b).norm() / b.norm())
    e_pair, e_small, e_old = rel(small, per_op), rel(small, want), rel(per_op, want)
    record(f"small_vs_perop/{precision}/B{B}_T{T}", pair=e_pair, small_vs_oracle=e_small, perop_vs_oracle=e_old)
    k = 1.0 if precision == "bf16" else 1.0 / 6.0
    assert torch.isfinite(small).all()
    assert e_pair < k * 6.5e-3 and e_small < k * 9e-3 and e_small < 1.2 * e_old + k * 1e-3, (e_pair, e_small, e_old)
    model.release()


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
@pytest.mark.parametrize("fmt", ["face", "pose"])
def test_key_split_attention_matches_softmax_and_the_query_split_kernel(dev, fmt, precision, monkeypatch):
    """Small forwards run attention with the KEYS split over a workgroup's waves and an LDS log-sum-exp merge
    (csrc/kernels_attn.h attn_ksplit_kernel).  Through a2p_attention (A2P_ATTN_KSPLIT=1 forces it): against float64 softmax
    attention at the precision's bar, and against attn_kernel to the rounding of the softmax sums.  Sizes: fewer tiles than waves
    (20 keys), ragged last tiles (77, 150), several tiles per wave (800), a spiked key (rescale across the merge)."""
    from audio2photoreal_amd import _lib
    monkeypatch.setenv("A2P_ATTN3", "0")   # the query-split side of the comparison is attn_kernel (attn3_kernel has its own tests: test_hip_round6.py)
    spec, model = _model(fmt, precision, dev, 1)
    model._ensure_ctx(dev, 1)
    lib = model._lib()
    d, H = spec.latent_dim, spec.num_heads
    g = torch.Generator().manual_seed(5)
    rel = lambda a, b: float((a.double() - b.double()).norm() / b.double().norm())
    for (N, Tq, S) in [(2, 100, 77), (1, 240, 800), (3, 33, 20), (2, 240, 240), (1, 150, 150)]:
        q, k, v = (torch.randn(N, L, d, generator=g) for L in (Tq, S, S))
        k[0, S // 3] *= 6.0
        dh = d // H
        qh, kh, vh = (t.view(N, -1, H, dh).transpose(1, 2).double() for t in (q, k, v))
        ref = (torch.softmax(qh @ kh.transpose(-1, -2) / dh ** 0.5, -1) @ vh).transpose(1, 2).reshape(N, Tq, d)
        qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)
        outs = {}
        for name, val in (("split", "1"), ("query", None)):
            if val is None:
                monkeypatch.delenv("A2P_ATTN_KSPLIT", raising=False)
            else:
                monkeypatch.setenv("A2P_ATTN_KSPLIT", val)
            _lib.check(lib.a2p_reload_env(model._ctx), "a2p_reload_env")
            out = torch.empty(N, Tq, d, device=dev)
            _lib.check(lib.a2p_attention(model._ctx, _lib.ptr(qd), _lib.ptr(kd), _lib.ptr(vd), _lib.ptr(out), N, Tq, S,
                                         _lib.current_stream()), "a2p_attention")
            outs[name] = out.cpu()
        e_ref, e_pair = rel(outs["split"], ref), rel(outs["split"], outs["query"])
        record(f"attn_ksplit/{fmt}/{precision}/{N}x{Tq}x{S}", rel_l2=e_ref, vs_query_split=e_pair)
        assert torch.isfinite(outs["split"]).all()
        # fp16 gates = min(1e-3, 2x measured): vs the fp64 reference 4.4e-4..5.0e-4, vs the query-split kernel 0.4e-5..1.05e-4
        assert e_ref < {"bf16": 2e-2, "fp16": 1e-3}[precision], (N, Tq, S, e_ref)
        assert e_pair < {"bf16": 6e-3, "fp16": 2.2e-4}[precision], (N, Tq, S, e_pair)
    model.release()


@pytest.mark.parametrize("precision", ["bf16", "fp16"])
def test_small_forward_with_and_without_key_split_attention(dev, precision, monkeypatch):
    """The whole small forward (config 0 shape: time-token tail in the cross attention) with the key-split attention and with
    attn_kernel (A2P_NO_KSPLIT=1): the same result to the rounding of the softmax sums."""
    B, T = 1, 240
    spec, model = _model("face", precision, dev, B)
    cfg = ClassifierFreeSampleModel(model)
    x, t, y = _inputs(spec, "face", B, T, dev)
    monkeypatch.delenv("A2P_NO_KSPLIT", raising=False)
    split = cfg(x, t, y).cpu()
    monkeypatch.setenv("A2P_NO_KSPLIT", "1")
    query = cfg(x, t, y).cpu()
    monkeypatch.delenv("A2P_NO_KSPLIT")
    err = float((split - query).norm() / query.norm())
    record(f"small_ksplit_vs_query/{precision}/B{B}_T{T}", rel_l2=err)
    assert torch.isfinite(split).all() and err < {"bf16": 4e-3, "fp16": 5e-4}[precision], err
    model.release()
