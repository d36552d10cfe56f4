"""Sharded forwards reproduce the unsharded batch bit for bit (`pytest -m gpu`).

`sample_parallel` promises that a sample comes out the same whichever shard computed it: every rank tells its denoiser the size of
the unsharded batch (`global_batch_hint`, include/a2p_hip.h a2p_set_batch_hint), and every size-based kernel choice that changes
rounding must follow that count instead of the shard's.  Two such choices exist: the kernel family (row panels vs small / per-op
kernels, csrc/a2p_lib_run.h run_forward) and the attention kernel (attn3_kernel vs attn_kernel, csrc/a2p_lib.hip launch_attn, which
differ by ~4e-4 in fp16 and ~2e-3 in bf16).  Here the geometries sit on both sides of the attention rule at T = 600, the blocks come
from the product's own `shard_bounds`, and the gathered blocks must be `torch.equal` to the full forward, with the same number of
attn3_kernel launches per block as the unsharded call (the decision, read back with a2p_debug_read)."""
import ctypes as C
import os
import socket
import subprocess
import sys

import pytest
import torch

from audio2photoreal_amd import _lib
from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel
from audio2photoreal_amd.model_util import create_model_and_diffusion, default_args, load_model
from audio2photoreal_amd.sample_parallel import shard_bounds
from audio2photoreal_amd.spec import face_spec, pose_spec
from audio2photoreal_amd.synthetic import synthetic_inputs, synthetic_state_dict
from conftest import ROOT, record, rel_l2

pytestmark = pytest.mark.gpu
SEED = 10
T = 600
WORLDS = (2, 3, 4, 8)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _debug_i64(model, name):
    n = C.c_int64(0)
    _lib.check(model._lib().a2p_debug_read(model._ctx, name, C.byref(n), 8), "a2p_debug_read")
    return int(n.value)


# Where the rule (launch_attn: attn_kernel while its grid is at most one workgroup per CU, attn3_kernel beyond; face self attention
# also not once attn3's own grid passes one round) puts each geometry at T = 600, with guidance (2B sequences; layer 0's self attention
# runs on the B shared ones) -- the face model's cond encoder (2 self attentions over 1998 audio tokens, per clip) takes attn3 from 3 samples on:
#   face B = 8:  self + cross everywhere (16 per forward); a block of 4 loses layer 0's self attention, blocks of <= 3 samples
#                (6 sequences) every one, blocks of <= 2 the cond encoder's too
#   face B = 32: cross only (8); blocks of 8 take the self attentions too (16)
#   body B = 16: cross (6; the keyframe attention is fused into the chain kernel); blocks of <= 3 take none
#   body B = 64: cross (6) in every block of WORLDS -- the plan of 32 ranks (blocks of 2) is what crosses the rule there
GEOMETRIES = [("face", 8, WORLDS), ("face", 32, WORLDS), ("pose", 16, WORLDS), ("pose", 64, WORLDS + (32,))]


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("fmt,B,worlds", GEOMETRIES, ids=[f"{f}_B{b}" for f, b, _ in GEOMETRIES])
def test_sharded_guided_forward_takes_the_unsharded_kernels_and_bits(dev, fmt, B, worlds, precision):
    """Guided forward (ClassifierFreeSampleModel), synthetic weights, a distinct timestep per sample, every block a fresh clip (so its
    conditioning -- the cond encoder of the face model included -- is prepared at the block's size).  With the hint: every block's
    rows are the full forward's bits and every block launches attn3_kernel as often as the unsharded call.  Without it (the shard's
    own rule, as before the hint reached the attention kernels): at least one plan must launch a different number, or this geometry
    does not cross the rule and proves nothing."""
    spec = face_spec() if fmt == "face" else pose_spec()
    inp = synthetic_inputs(spec, B, T, SEED)
    model, _ = create_model_and_diffusion(default_args(fmt), "test", precision=precision, max_batch=B)
    load_model(model, synthetic_state_dict(spec, SEED))
    cfg = ClassifierFreeSampleModel(model.to(dev).eval())
    model._ensure_ctx(dev, B)                                   # the context the counter lives on (every block below reuses it)
    x = inp["x_T"].to(dev)
    t = ((torch.arange(B) * 997 + 13) % 1000).to(dev)          # distinct per sample
    scale = torch.full((B,), 10.0 if fmt == "face" else 2.0, device=dev)
    cond = {k: inp[k].to(dev) for k in ("cond_embed", "keyframes", "mask") if k in inp}

    def call(lo, hi, hint):
        model.global_batch_hint = hint
        y = {k: v[lo:hi].clone() for k, v in cond.items()}   # a fresh clip: its conditioning is prepared at this size
        y["scale"] = scale[lo:hi].contiguous()
        before = _debug_i64(model, b"attn3_launches")
        out = cfg(x[lo:hi].contiguous(), t[lo:hi].contiguous(), y).cpu()
        return out, _debug_i64(model, b"attn3_launches") - before

    whole, n_whole = call(0, B, 0)
    assert n_whole > 0, "the unsharded call launches attn3_kernel: nothing to follow otherwise"
    alone = {}
    for world in worlds:
        blocks = [shard_bounds(B, world, r) for r in range(world)]
        hinted = [call(lo, hi, B) for lo, hi in blocks]
        own = [call(lo, hi, 0) for lo, hi in blocks]
        got = torch.cat([o for o, _ in hinted])
        diff = float((got - whole).abs().max())
        own_diff = float((torch.cat([o for o, _ in own]) - whole).abs().max())
        alone[world] = [n for _, n in own]
        record(f"shard_invariance/{fmt}_B{B}/{precision}/world{world}", max_abs_diff=diff, unhinted_max_abs_diff=own_diff,
               attn3_unsharded=n_whole, attn3_hinted=[n for _, n in hinted], attn3_unhinted=alone[world])
        assert [n for _, n in hinted] == [n_whole] * world, (world, blocks, n_whole, [n for _, n in hinted])
        assert torch.equal(got, whole), f"{fmt} B={B} {precision} blocks {blocks}: max |diff| = {diff:.3e}"
    model.global_batch_hint = 0
    model.check_finite()
    model.release()
    assert torch.isfinite(whole).all()
    assert any(n != n_whole for ns in alone.values() for n in ns), \
        f"{fmt} B={B}: no plan without the hint takes a different attn3 count than the unsharded call ({n_whole}): {alone}"


def _attention_fp64(q, k, v, heads):
    """softmax(q k^T / sqrt(dh)) v per head in float64 (no projections)."""
    N, Tq, d = q.shape
    dh = d // heads
    qh, kh, vh = (z.double().view(N, -1, heads, dh).transpose(1, 2) for z in (q, k, v))
    w = torch.softmax(qh @ kh.transpose(-1, -2) / dh ** 0.5, dim=-1)
    return (w @ vh).transpose(1, 2).reshape(N, Tq, d)


@pytest.mark.parametrize("precision", ["fp16", "bf16"])
@pytest.mark.parametrize("fmt", ["face", "pose"])
def test_batch_hint_does_not_reach_direct_attention_calls(dev, fmt, precision):
    """a2p_attention called through the ABI decides from its own N whatever hint the context carries: N = 2 sequences of 600
    queries x 2000 keys is attn_kernel's size (one round of workgroups); a hint of 64 scaled into it would pick attn3_kernel."""
    spec = face_spec() if fmt == "face" else pose_spec()
    model, _ = create_model_and_diffusion(default_args(fmt), "test", precision=precision, max_batch=2)
    load_model(model, synthetic_state_dict(spec, SEED))
    model = model.to(dev).eval()
    model._ensure_ctx(dev, 2)
    lib = model._lib()
    d, H = spec.latent_dim, spec.num_heads
    N, Tq, S = 2, 600, 2000
    g = torch.Generator().manual_seed(23)
    q, k, v = (torch.randn(N, L, d, generator=g) for L in (Tq, S, S))
    qd, kd, vd = q.to(dev), k.to(dev), v.to(dev)

    def run(hint):
        _lib.check(lib.a2p_set_batch_hint(model._ctx, hint), "a2p_set_batch_hint")
        before = _debug_i64(model, b"attn3_launches")
        out = torch.empty(N, Tq, d, device=dev)
        _lib.check(lib.a2p_attention(model._ctx, _lib.ptr(qd), _lib.ptr(kd), _lib.ptr(vd), _lib.ptr(out), N, Tq, S, _lib.current_stream()),
                   "a2p_attention")
        return out.cpu(), _debug_i64(model, b"attn3_launches") - before
    plain, n_plain = run(0)
    hinted, n_hinted = run(64)
    _lib.check(lib.a2p_set_batch_hint(model._ctx, 0), "a2p_set_batch_hint")
    model.release()
    e = rel_l2(hinted, _attention_fp64(q, k, v, H))
    record(f"shard_invariance/direct_attention/{fmt}/{precision}", vs_fp64=e, attn3=[n_plain, n_hinted])
    assert (n_plain, n_hinted) == (0, 0), (n_plain, n_hinted)
    assert torch.equal(hinted, plain)
    assert e < (1.0e-3 if precision == "fp16" else 6.0e-3), e      # test_hip_round6.py's fp64 tolerance for the attention kernels


def test_sample_parallel_four_ranks_match_one_rank_at_full_size(dev, tmp_path):
    """sample_parallel end to end at the headline face geometry: 8 samples of 600 frames, 8 layers, DDIM 5 steps with eta > 0, IEEE
    half, over 4 ranks sharing cuda:0 (blocks of 2: without the hint reaching the attention kernels, those take attn_kernel where the
    single-rank run takes attn3_kernel).  The gathered samples must be the single-rank samples bit for bit."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    geometry = "8,600,8,ddim5"
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), A2P_DIST_OUT=str(tmp_path), A2P_DIST_PRECISION="fp16",
               A2P_DIST_GEOMETRY=geometry)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=4", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "tests", "dist_worker_gpu.py")]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import dist_worker_gpu as W
    want = W.run_sampler("fp16", dev, world=1, rank=0, geometry=geometry).cpu()
    got = [torch.load(tmp_path / f"r{i}.pt") for i in range(4)]
    assert all(torch.equal(got[0], g) for g in got[1:]), "all ranks must hold all samples after the single all_gather"
    diff = float((got[0] - want).abs().max())
    record("shard_invariance/dist4/face_B8_T600_L8_ddim5/fp16", max_abs_diff=diff)
    assert torch.isfinite(want).all()
    assert torch.equal(got[0], want), f"4 ranks != 1 rank, max |diff| = {diff:.3e}"
