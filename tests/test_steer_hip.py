"""Joint steering on the MI355X (csrc/kernels_steer.h, sample/steer.py) against the float64 restatement of
tests/steer_restatement.py: loss and gradient, the descent, determinism, one sampling step, and a ten-step loop.

The gate of every comparison is the rule of test_skinning_hip.py: 4 x the normalised error of the restatement in float32 against
itself in float64 on the same inputs (computed here, per case).  Two derived quantities add a few float32 ulp to it, each
with its reason beside it: x_next (fused multiply-adds) and the reported residual (a square root of the loss)."""
import ctypes

import numpy as np
import pytest
import torch

import skinning_restatement as R
import steer_restatement as SR
from audio2photoreal_amd import _lib
from audio2photoreal_amd import skinning as S
from audio2photoreal_amd.sample import steer
from conftest import record

pytestmark = pytest.mark.gpu
N = 7
P_POS = 104
G = np.array([1.5, 0.5, 2.0], np.float32)          # global_scaling of every test skeleton: anisotropic on purpose
PINNED_ROOT = np.array([0.5, -1.25, 2.0], np.float32)   # times G: exact in float32, so float32 and float64 agree that y = p


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def build(skel, **kw):
    return S.BodySkeleton.from_arrays(skel["parents"], skel["pre_rotation"], skel["joint_offset"], skel["transform"],
                                      skel["transform_offsets"], int(skel["nr_position_params"]), int(skel["nr_scaling_params"]),
                                      skel["rest_vertices"], skel["skin_indices"], skel["skin_weights"], **kw)


def _pinned_root(skel):
    """The skeleton with a root whose translation no parameter drives and whose offsets are zero: its position is joint_offset[0]
    in every precision, so an aim at that point coincides with the joint exactly."""
    skel = {k: np.array(v, copy=True) for k, v in skel.items()}
    skel["transform"][0:3] = 0
    skel["transform_offsets"][0:3] = 0
    skel["joint_offset"][0] = PINNED_ROOT
    return skel


SKELETONS = {
    "root_only": lambda: R.make_skeleton(1, 1, 4, 1),
    "two_children": lambda: R.make_skeleton(2, 5, 8, 2, parents=[-1, 0, 1, 1, 3]),
    "chain40": lambda: R.make_skeleton(3, 40, 8, 2, parents=[-1] + list(range(39))),
    "j23": lambda: R.make_skeleton(4, 23, 16, 4),
    "j160": lambda: R.make_skeleton(7, 160, 16, 4),
    "j300": lambda: R.make_skeleton(5, 300, 16, 4),
    "no_scale": lambda: R.make_skeleton(6, 23, 16, 4, P_scale=0),
    "j1000": lambda: R.make_skeleton(8, 1000, 16, 4),
}
_CACHE = {}


def case(name, pinned=False):
    """(skeleton dict, BodySkeleton, z [N, 104], scales [1, P_scale], mean, std) of a named skeleton, built once."""
    if pinned:
        if ("pinned", name) not in _CACHE:
            skel, _, z, scales, mean, std = case(name)
            skel = _pinned_root(skel)
            _CACHE["pinned", name] = (skel, build(skel, global_scaling=G, lbs_scale=scales[0] if scales.size else None), z, scales, mean, std)
        return _CACHE["pinned", name]
    if name not in _CACHE:
        skel = SKELETONS[name]()
        P_scale = int(skel["nr_scaling_params"])
        z, scales = R.make_inputs(11, N, P_POS, max(P_scale, 1))
        scales = scales if P_scale else np.zeros((1, 0), np.float32)
        rs = np.random.RandomState(5)
        mean, std = (rs.randn(P_POS) * 0.1).astype(np.float32), rs.uniform(0.3, 1.5, P_POS).astype(np.float32)
        _CACHE[name] = (skel, build(skel, global_scaling=G, lbs_scale=scales[0] if P_scale else None), z, scales, mean, std)
    return _CACHE[name]


def constraint_sets(skel, scales):
    """The named constraint sets of a skeleton (dicts of steer_restatement.make_constraints).  "aim_at_the_joint" is for the
    skeleton with the pinned root."""
    J = len(skel["parents"])
    leaf = J - 1
    sets = {"root_reach": [(0, SR.REACH, 1.0)], "leaf_reach": [(leaf, SR.REACH, 2.0)],
            "reach_and_aim": [(leaf, SR.REACH, 1.0), (leaf, SR.AIM, 0.7)],
            "sixteen": [((3 * k) % J, k % 2, 0.5 + 0.1 * k) for k in range(16)],
            "zero_weight": [(leaf, SR.REACH, 1.0), (J // 2, SR.AIM, 0.0), (0, SR.AIM, 1.5)],
            "aim_at_the_joint": [(0, SR.AIM, 1.0), (leaf, SR.REACH, 1.0)]}
    out = {k: SR.make_constraints(skel, scales, N, spec, 21) for k, spec in sets.items()}
    at = out["aim_at_the_joint"]
    at["targets"][:4, 0] = PINNED_ROOT * G                          # frames 0..3: the point is the (pinned) root itself
    return out


def product_constraints(cons, J):
    return S.JointConstraints(cons["joints"], cons["kinds"], cons["axes"], cons["targets"], cons["weights"], J)


def gate(name, got, want, f32):
    """Record and assert: got (device tensor) against want (float64 restatement) within 4 x nerr(float32 restatement, want).  A
    reference that is zero everywhere (a root nothing drives) must be matched exactly."""
    got, want, f32 = got.cpu().numpy(), np.asarray(want), np.asarray(f32)
    if not np.abs(want).max():
        assert not np.abs(got).max(), name
        return
    err, allowance = R.nerr(got, want), 4 * R.nerr(f32, want)
    record(name, err=err, allowance=float(allowance))
    assert np.isfinite(err) and err <= allowance, (name, err, allowance)


# ------------------------------------------------------------------------------------------------ loss and gradient
@pytest.mark.parametrize("name", [n for n in SKELETONS if n not in ("j160", "j1000")])
def test_loss_and_gradient_against_float64(dev, name):
    _, _, z, scales, mean, std = case(name)
    zt = torch.from_numpy(z).to(dev)
    for cname in constraint_sets(case(name)[0], scales):
        skel, sk = case(name, pinned=cname == "aim_at_the_joint")[:2]
        cons = constraint_sets(skel, scales)[cname]
        L64, g64 = SR.loss_grad(skel, cons, z, scales, mean, std, G)
        L32, g32 = SR.loss_grad(skel, cons, z, scales, mean, std, G, torch.float32)
        loss, grad = sk.joint_loss_grad(zt, product_constraints(cons, sk.J), mean=mean, std=std)
        assert loss.shape == (N,) and grad.shape == (N, P_POS)
        gate(f"steer_{name}_{cname}_loss", loss, L64.numpy(), L32.numpy())
        gate(f"steer_{name}_{cname}_grad", grad, g64.numpy(), g32.numpy())
        if cname == "aim_at_the_joint":
            only_aim = dict(cons, joints=cons["joints"][:1], kinds=cons["kinds"][:1], axes=cons["axes"][:1],
                            targets=cons["targets"][:, :1], weights=cons["weights"][:, :1])
            loss, grad = sk.joint_loss_grad(zt, product_constraints(only_aim, sk.J), mean=mean, std=std)
            assert not loss[:4].any() and not grad[:4].any()                  # the term and its gradient are 0 there
            assert loss[4:].gt(0).all()


def test_without_statistics_the_gradient_is_with_respect_to_the_poses(dev):
    skel, sk, z, scales, _, _ = case("j23")
    cons = constraint_sets(skel, scales)["reach_and_aim"]
    L64, g64 = SR.loss_grad(skel, cons, z, scales, None, None, G)
    L32, g32 = SR.loss_grad(skel, cons, z, scales, None, None, G, torch.float32)
    loss, grad = sk.joint_loss_grad(torch.from_numpy(z).to(dev), product_constraints(cons, sk.J))
    gate("steer_j23_plain_loss", loss, L64.numpy(), L32.numpy())
    gate("steer_j23_plain_grad", grad, g64.numpy(), g32.numpy())


def test_a_skeleton_that_needs_more_than_64_kib_of_lds(dev):
    """1000 joints: 66 KiB of dynamic LDS, beyond what a kernel gets without asking for it."""
    skel, sk, z, scales, mean, std = case("j1000")
    cons = constraint_sets(skel, scales)["sixteen"]
    L64, g64 = SR.loss_grad(skel, cons, z, scales, mean, std, G)
    L32, g32 = SR.loss_grad(skel, cons, z, scales, mean, std, G, torch.float32)
    loss, grad = sk.joint_loss_grad(torch.from_numpy(z).to(dev), product_constraints(cons, sk.J), mean=mean, std=std)
    gate("steer_j1000_sixteen_loss", loss, L64.numpy(), L32.numpy())
    gate("steer_j1000_sixteen_grad", grad, g64.numpy(), g32.numpy())


# ------------------------------------------------------------------------------------------------ descent
@pytest.mark.parametrize("iterations", [1, 2, 8])
@pytest.mark.parametrize("name", ["j23", "j160"])
def test_descent_against_float64(dev, name, iterations):
    """Three reach targets taken from another random pose, on 23 and 160 joints."""
    skel, sk, z, scales, mean, std = case(name)
    J = len(skel["parents"])
    cons = SR.make_constraints(skel, scales, N, [(J - 1, SR.REACH, 1.0), (J // 2, SR.REACH, 1.0), (J // 3, SR.REACH, 1.0)], 21)
    z64, _ = SR.descend(skel, cons, z, scales, iterations, 1.0, 0.25, mean, std, G)
    z32, _ = SR.descend(skel, cons, z, scales, iterations, 1.0, 0.25, mean, std, G, torch.float32)
    got = sk.solve_ik(torch.from_numpy(z).to(dev), product_constraints(cons, sk.J), iterations=iterations, mean=mean, std=std)
    gate(f"steer_{name}_descent_{iterations}", got, z64.numpy(), z32.numpy())


def test_a_far_target_takes_the_trust_region(dev):
    skel, sk, z, scales, mean, std = case("j23")
    cons = SR.make_constraints(skel, scales, N, [(22, SR.REACH, 1.0)], 21)
    cons["targets"][:, 0] += np.float32([100.0, 0.0, 0.0])
    z64, branches = SR.descend(skel, cons, z, scales, 2, 1.0, 0.25, mean, std, G)
    assert (branches == 2).all()                                              # the float64 run takes the trust-region branch
    z32, _ = SR.descend(skel, cons, z, scales, 2, 1.0, 0.25, mean, std, G, torch.float32)
    got = sk.solve_ik(torch.from_numpy(z).to(dev), product_constraints(cons, sk.J), iterations=2, mean=mean, std=std)
    gate("steer_j23_trust_region", got, z64.numpy(), z32.numpy())
    moved = (got.cpu() - torch.from_numpy(z)).abs().amax(dim=1)
    assert (moved <= 2 * 0.25 * (1 + 1e-6)).all() and (moved > 0.25).all()    # max_step per iteration, and it did move


def test_frames_without_weight_and_non_finite_frames_stay(dev):
    skel, sk, z, scales, mean, std = case("j23")
    cons = constraint_sets(skel, scales)["reach_and_aim"]
    cons["weights"][2] = 0
    zz = z.copy()
    zz[5] = np.inf
    zt = torch.from_numpy(zz).to(dev)
    got = sk.solve_ik(zt, product_constraints(cons, sk.J), iterations=2, mean=mean, std=std)
    assert torch.equal(got[2], zt[2]) and torch.equal(got[5], zt[5])
    assert not torch.equal(got[0], zt[0]) and torch.isfinite(got[[0, 1, 2, 3, 4, 6]]).all()
    loss, grad = sk.joint_loss_grad(zt, product_constraints(cons, sk.J), mean=mean, std=std)
    assert loss[2] == 0 and not grad[2].any()


# ------------------------------------------------------------------------------------------------ determinism
def test_same_bits_twice_and_per_frame(dev):
    skel, sk, z, scales, mean, std = case("j300")
    cons = constraint_sets(skel, scales)["sixteen"]
    zt = torch.from_numpy(z).to(dev)
    pc = product_constraints(cons, sk.J)
    a = sk.solve_ik(zt, pc, iterations=2, mean=mean, std=std)
    b = sk.solve_ik(zt, pc, iterations=2, mean=mean, std=std)
    la, ga = sk.joint_loss_grad(zt, pc, mean=mean, std=std)
    lb, gb = sk.joint_loss_grad(zt, pc, mean=mean, std=std)
    assert torch.equal(a, b) and torch.equal(la, lb) and torch.equal(ga, gb)
    for n in range(N):
        one = dict(cons, targets=cons["targets"][n:n + 1], weights=cons["weights"][n:n + 1])
        p1 = product_constraints(one, sk.J)
        assert torch.equal(sk.solve_ik(zt[n:n + 1], p1, iterations=2, mean=mean, std=std)[0], a[n]), n
        l1, g1 = sk.joint_loss_grad(zt[n:n + 1], p1, mean=mean, std=std)
        assert torch.equal(l1[0], la[n]) and torch.equal(g1[0], ga[n]), n


def test_argument_errors_come_back_before_any_launch(dev):
    skel, sk, z, scales, mean, std = case("j23")
    cons = product_constraints(constraint_sets(skel, scales)["root_reach"], sk.J)
    zt = torch.from_numpy(z).to(dev)
    with pytest.raises(_lib.A2PError, match="cover 7 frames"):
        sk.solve_ik(zt[:3], cons)
    t = sk._tables(dev)
    tg, w = cons.on(dev)
    out = torch.full_like(zt, 7.0)
    for field, value, match in (("joints_host", sk.J, "joint"), ("kinds_host", 2, "kind"), ("K", 17, "K=17"), ("iterations", -1, "iterations"),
                                ("alpha", 0.0, "alpha"), ("J", 0, "J=0")):
        d, keep = sk.steer_description(t, cons, tg, w, None, None, t["lbs_scale"], 0, 1.0, 2, 0.25)
        if field.endswith("_host"):
            getattr(d, field)[0] = value                                     # past the host checks of the Python layer
        else:
            setattr(d, field, value)
        with pytest.raises(_lib.A2PError, match=match):
            _lib.check(_lib.load().a2p_skin_steer(ctypes.byref(d), _lib.ptr(zt), P_POS, N, _lib.ptr(out), P_POS, None, None,
                                                  _lib.current_stream(dev)), "a2p_skin_steer")
    torch.cuda.synchronize(dev)
    assert (out == 7.0).all()


# ------------------------------------------------------------------------------------------------ one sampling step
B, T = 2, 40
_MODEL = {}


def _model(dev):
    """A 2-layer synthetic body model (fp32, ddim10 tables) and its diffusion."""
    if not _MODEL:
        from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel
        from audio2photoreal_amd.model_util import create_model_and_diffusion, default_args, load_model
        from audio2photoreal_amd.spec import pose_spec
        from audio2photoreal_amd.synthetic import synthetic_state_dict
        m, d = create_model_and_diffusion(default_args("pose", layers=2, timestep_respacing="ddim10"), "test", precision="fp32", max_batch=4)
        load_model(m, synthetic_state_dict(pose_spec(num_layers=2), 10))
        _MODEL["m"] = (ClassifierFreeSampleModel(m.to(dev).eval()), d)
    return _MODEL["m"]


def _y(model, dev, seed=10):
    from audio2photoreal_amd.synthetic import cond_tokens_for_frames
    g = torch.Generator().manual_seed(seed)
    return {"cond_embed": torch.randn(B, cond_tokens_for_frames(T), model.model.cond_feature_dim, generator=g).to(dev),
            "scale": torch.full((B,), 2.0, device=dev), "keyframes": torch.randn(B, len(range(T)[::30]), P_POS, generator=g).to(dev),
            "mask": torch.ones(B, 1, 1, T, dtype=torch.bool, device=dev)}


def _step_targets(sk, skel, scales, weight=1.0):
    """Reach targets for two joints and an aim, over part of the clip with a ramp: frames with and without weight."""
    other = SR.make_constraints(skel, scales, B * T, [(22, SR.REACH, 1.0), (10, SR.REACH, 1.0), (15, SR.AIM, 1.0)], 33)
    tg = other["targets"].reshape(B, T, 3, 3)
    jt = steer.JointTargets(sk, B, T)
    jt.reach(22, slice(5, 30), tg[:, 5:30, 0] * G, weight=weight, ramp=3)
    jt.reach(10, slice(0, T), tg[:, :, 1] * G, weight=0.5 * weight)
    jt.aim(15, np.arange(20, 36), tg[:, 20:36, 2] * G, axis=other["axes"][2], weight=weight)
    return jt


def _as_dict(jt):
    targets, weights = jt.dense()
    return {"joints": jt.joints, "kinds": jt.kinds, "axes": np.stack(jt.axes), "targets": targets.reshape(-1, jt.K, 3),
            "weights": weights.reshape(-1, jt.K)}


def _description(sk, jt, mean, std, dev, iterations=2):
    cons = jt.constraints()
    t = sk._tables(dev)
    tg, w = cons.on(dev)
    f = lambda a: torch.from_numpy(a).to(dev)
    return sk.steer_description(t, cons, tg, w, f(mean), f(std), t["lbs_scale"], 0, 1.0, iterations, 0.25)


STEP_CASES = [(_lib.SAMPLER_DDIM, 0.0, False), (_lib.SAMPLER_DDIM, 0.5, True), (_lib.SAMPLER_DDPM, 0.0, False), (_lib.SAMPLER_DDPM, 0.0, True)]


def test_step_with_zero_weights_is_the_plain_step(dev):
    skel, sk, _, scales, mean, std = case("j23")
    model, diff = _model(dev)
    y = _y(model, dev)
    desc = _description(sk, _step_targets(sk, skel, scales, weight=0.0), mean, std, dev)
    g = torch.Generator().manual_seed(3)
    x, noise = torch.randn(B, P_POS, 1, T, generator=g).to(dev), torch.randn(B, P_POS, 1, T, generator=g).to(dev)
    tab, tmap = diff._tables(dev), diff._timestep_map_tensor(dev)
    for step in (7, 0):
        t = torch.full((B,), step, dtype=torch.int64, device=dev)
        for sampler, eta, clip in STEP_CASES:
            nz = None if (sampler == _lib.SAMPLER_DDIM and eta == 0.0) else noise
            want = model.a2p_sample_step(sampler, x, t, tmap, tab, y, nz, eta, clip)
            got = model.a2p_sample_step_steer(sampler, x, t, tmap, tab, y, nz, eta, clip, desc)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (step, sampler, eta, clip)
    model.model.check_finite()


def test_step_against_the_restatement(dev):
    skel, sk, _, scales, mean, std = case("j23")
    model, diff = _model(dev)
    y = _y(model, dev)
    jt = _step_targets(sk, skel, scales)
    cons = _as_dict(jt)
    desc = _description(sk, jt, mean, std, dev)
    gen = torch.Generator().manual_seed(3)
    x, noise = torch.randn(B, P_POS, 1, T, generator=gen).to(dev), torch.randn(B, P_POS, 1, T, generator=gen).to(dev)
    tab, tmap = diff._tables(dev), diff._timestep_map_tensor(dev)
    tab_h = tab.cpu().numpy().astype(np.float64)
    xh, nh = x.cpu().numpy()[:, :, 0].astype(np.float64), noise.cpu().numpy()[:, :, 0].astype(np.float64)
    for step in (7, 0):
        t = torch.full((B,), step, dtype=torch.int64, device=dev)
        guided = model(x, tmap[t], y).cpu().numpy().reshape(B * T, P_POS)                    # a2p_denoise_forward: [B, T, C]
        z64, _ = SR.descend(skel, cons, guided, scales, 2, 1.0, 0.25, mean, std, G)
        z32, _ = SR.descend(skel, cons, guided, scales, 2, 1.0, 0.25, mean, std, G, torch.float32)
        moved = np.abs(z64.numpy() - guided).max(axis=1).reshape(B, T)
        assert (moved[:, 5:30] > 0).all()                                                  # the weighted frames are steered
        lay = lambda a: a.reshape(B, T, P_POS).transpose(0, 2, 1)                           # -> [B, C, T]
        tabs = {n: tab_h[i] for i, n in enumerate(_lib.TABLE_NAMES)}
        for sampler, eta, clip in STEP_CASES:
            nz = None if (sampler == _lib.SAMPLER_DDIM and eta == 0.0) else noise
            x_next, x0 = model.a2p_sample_step_steer(sampler, x, t, tmap, tab, y, nz, eta, clip, desc)
            c = (lambda a: np.clip(a, -1, 1)) if clip else (lambda a: a)
            name = f"steer_step_t{step}_s{sampler}_eta{eta}_clip{int(clip)}"
            gate(name + "_x0", x0[:, :, 0], c(lay(z64.numpy())), c(lay(z32.numpy())))
            # the update of the kernel's own pred_xstart, in float64 and (for the allowance) in float32
            upd = {}
            for dt in (np.float64, np.float32):
                tb = {k: v.astype(dt) for k, v in tabs.items()}
                x0h = x0[:, :, 0].cpu().numpy().astype(dt)
                n_ = None if nz is None else nh.astype(dt)
                upd[dt] = SR.ddim_update(x0h, xh.astype(dt), n_, tb, step, dt(eta)) if sampler == _lib.SAMPLER_DDIM else \
                    SR.ddpm_update(x0h, xh.astype(dt), n_, tb, step)
            # (+ 2^-22: where the float32 restatement happens to round like float64, the kernel's fused multiply-adds still differ)
            err, allowance = R.nerr(x_next[:, :, 0].cpu().numpy(), upd[np.float64]), 4 * R.nerr(upd[np.float32], upd[np.float64]) + 2.0 ** -22
            record(name + "_x_next", err=err, allowance=float(allowance))
            assert err <= allowance, (name, err, allowance)
    model.model.check_finite()


# ------------------------------------------------------------------------------------------------ a ten-step loop
def test_loop_reaches_reachable_targets(dev):
    skel, sk, _, scales, mean, std = case("j23")
    model, diff = _model(dev)
    y = _y(model, dev)
    other = SR.make_constraints(skel, scales, B * T, [(22, SR.REACH, 1.0), (10, SR.REACH, 1.0), (15, SR.REACH, 1.0)], 44)
    jt = steer.JointTargets(sk, B, T)
    for k, j in enumerate((22, 10, 15)):
        jt.reach(j, slice(0, T), other["targets"][:, k].reshape(B, T, 3) * G)
    cons = _as_dict(jt)
    noise = torch.randn(B, P_POS, 1, T, generator=torch.Generator().manual_seed(5)).to(dev)
    iterations = 2
    plain = diff.ddim_sample_loop(model, (B, P_POS, 1, T), noise=noise, clip_denoised=False, model_kwargs={"y": y})
    steered = steer.steered_sample_loop(diff, model, y, sk, mean, std, jt, noise, iterations=iterations)
    flat = lambda s: s[:, :, 0].permute(0, 2, 1).reshape(B * T, P_POS).cpu().numpy()
    pose = lambda zz: mean.astype(np.float64) + std.astype(np.float64) * np.asarray(zz, np.float64)
    res = lambda zz: float(SR.residual(skel, cons, pose(zz), scales, G).mean())
    r_plain, r_steered = res(flat(plain)), res(flat(steered))
    z64, _ = SR.descend(skel, cons, flat(plain), scales, iterations, 1.0, 0.25, mean, std, G)
    f64, f_loop = r_plain / res(z64.numpy()), r_plain / r_steered
    record("steer_loop", residual_plain=r_plain, residual_steered=r_steered, factor_float64_from_plain=f64, factor_loop=f_loop,
           iterations=iterations)
    assert f64 > 1.0
    # (the margin of 2: the steered trajectory is not the unsteered one)
    assert f_loop >= 0.5 * f64, (f_loop, f64)
    # the residual the package reports is the restatement's
    got = steer.steer_residual(sk, jt, torch.from_numpy(pose(flat(steered)).astype(np.float32)).to(dev).reshape(B, T, P_POS))
    p32 = pose(flat(steered)).astype(np.float32)
    want, f32 = (SR.residual(skel, cons, p32, scales, G, dt).numpy().reshape(B, T, 3) for dt in (torch.float64, torch.float32))
    # sqrt(2 (d^2 / 2)) on top of the float32 restatement's own error: the sum of squares, the halving and the root, a few ulp
    err, allowance = R.nerr(got.cpu().numpy(), want), 4 * R.nerr(f32, want) + 8 * 2.0 ** -24
    record("steer_residual", err=err, allowance=float(allowance))
    assert got.shape == (B, T, 3) and err <= allowance, (err, allowance)


# ------------------------------------------------------------------------------------------------ from a recording
def test_generate_steered_end_to_end(dev):
    """generate_from_recording's result with the body steered: same keys and the same face, keyframes and audio; a lower residual
    on the steered frames; the reported residual is that of the returned poses; overlap does not change the bits."""
    from audio2photoreal_amd.sample.long_form import recording_frames
    from audio2photoreal_amd.sample.recording import generate_from_recording
    from test_inpaint_hip import SR as RATE, _models, _recording, _stats
    models = _models(dev, "fp32")
    face, pose = models["face"], models["pose"]
    stats, wav = _stats(), _recording(4.0)
    skel, sk, _, scales, _, _ = case("j23")
    reps, frames = 2, recording_frames(wav, RATE)
    assert frames == 120
    other = SR.make_constraints(skel, scales, reps * frames, [(22, SR.REACH, 1.0)], 55)["targets"].reshape(reps, frames, 3) * G
    jt = steer.JointTargets(sk, reps, frames).reach(22, slice(30, 90), other[:, 30:90], ramp=10)
    plain = generate_from_recording(face, pose, stats, wav, RATE, num_repetitions=reps, overlap=False)
    out = steer.generate_steered(face, pose, stats, wav, RATE, sk, jt, num_repetitions=reps, overlap=False)
    assert set(out) == set(plain) | {"steer_residual"} and out["T"] == frames
    for k in ("face", "keyframes", "audio"):
        assert np.array_equal(out[k], plain[k]), k
    assert out["pose"].shape == plain["pose"].shape == (reps, frames, P_POS) and np.isfinite(out["pose"]).all()
    assert out["steer_residual"].shape == (reps, frames, 1)
    on_gpu = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    assert np.array_equal(out["steer_residual"], steer.steer_residual(sk, jt, on_gpu(out["pose"])).cpu().numpy())
    before = steer.steer_residual(sk, jt, on_gpu(plain["pose"])).cpu().numpy()
    record("steer_recording", residual_plain=float(before[:, 30:90].mean()), residual_steered=float(out["steer_residual"][:, 30:90].mean()))
    assert out["steer_residual"][:, 30:90].mean() < before[:, 30:90].mean()
    again = steer.generate_steered(face, pose, stats, wav, RATE, sk, jt, num_repetitions=reps, overlap=True)
    assert np.array_equal(again["pose"], out["pose"]) and np.array_equal(again["face"], out["face"])
    with pytest.raises(_lib.A2PError, match="JointTargets"):
        steer.generate_steered(face, pose, stats, wav, RATE, sk, steer.JointTargets(sk, reps, frames + 1).reach(0, slice(0, 1), [0.0, 0.0, 0.0]),
                               num_repetitions=reps)
    with pytest.raises(_lib.A2PError, match="windowed"):
        steer.generate_steered(face, pose, stats, _recording(24.0), RATE, sk, jt, num_repetitions=reps)
