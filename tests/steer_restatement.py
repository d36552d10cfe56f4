"""A torch restatement of joint steering (audio2photoreal_amd/sample/steer.py, csrc/kernels_steer.h), written from the formulas of
tests/skinning_restatement.py and the definitions of the loss and the update rule.  Test infrastructure: the yardstick of
tests/test_steer_hip.py and tests/test_steer_cpu.py.

The skeleton solve is skinning_restatement's, in torch so that autograd gives the gradient: nothing here is a hand-written
derivative.  Every function takes `dtype` (float64 by default): all inputs are cast to it and every operation runs in it.  The
float32 run against the float64 run is the rounding error float32 arithmetic makes: the allowance of the GPU tests.

Constraints are a dict: joints [K] ints, kinds [K] (0 reach, 1 aim), axes [K, 3], targets [N, K, 3], weights [N, K]."""
import numpy as np
import torch

REACH, AIM = 0, 1


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def qmul(q, r):
    qx, qy, qz, qw = q.unbind(-1)
    rx, ry, rz, rw = r.unbind(-1)
    return torch.stack([qw * rx + qx * rw + qy * rz - qz * ry,
                        qw * ry - qx * rz + qy * rw + qz * rx,
                        qw * rz + qx * ry - qy * rx + qz * rw,
                        qw * rw - qx * rx - qy * ry - qz * rz], dim=-1)


def qrot(q, v):
    a = q[..., :3]
    av = torch.linalg.cross(a, v)
    aav = torch.linalg.cross(a, av)
    return v + 2 * (av * q[..., 3:4] + aav)


def from_xyz(r):
    h = r * torch.tensor([-0.5, 0.5, 0.5], dtype=r.dtype)
    c, s = torch.cos(h), torch.sin(h)
    c0, c1, c2 = c.unbind(-1)
    s0, s1, s2 = s.unbind(-1)
    return torch.stack([-s0 * c1 * c2 - c0 * s1 * s2,
                        c0 * s1 * c2 - s0 * c1 * s2,
                        c0 * c1 * s2 + s0 * s1 * c2,
                        c0 * c1 * c2 - s0 * s1 * s2], dim=-1)


def joint_states(skel, poses, scales, dtype=torch.float64):
    """[N, J, 8] global states (translation, quaternion xyzw, scale) of poses [N, P_pos] (a tensor: autograd passes through) and
    scales [1 or N, P_scale]."""
    poses = poses.to(dtype)
    N = poses.shape[0]
    P_scale = np.asarray(scales).shape[-1]
    sc = _t(scales, dtype).reshape(-1, P_scale).expand(N, -1) if P_scale else poses.new_zeros(N, 0)
    x = torch.cat([poses, sc], dim=1)
    jp = (x @ _t(skel["transform"], dtype).T + _t(skel["transform_offsets"], dtype).reshape(1, -1)).reshape(N, -1, 7)
    J = jp.shape[1]
    parents = np.asarray(skel["parents"]).reshape(-1)
    lt = jp[:, :, 0:3] + _t(skel["joint_offset"], dtype)[None]
    lr = qmul(_t(skel["pre_rotation"], dtype)[None].expand(N, -1, -1), from_xyz(jp[:, :, 3:6]))
    ls = torch.exp2(jp[:, :, 6])
    t, q, s = [None] * J, [None] * J, [None] * J
    for j in range(J):
        p = int(parents[j])
        if p < 0 or p >= J:
            t[j], q[j], s[j] = lt[:, j], lr[:, j], ls[:, j]
        else:
            q[j] = qmul(q[p], lr[:, j])
            t[j] = qrot(q[p], lt[:, j] * s[p][:, None]) + t[p]
            s[j] = s[p] * ls[:, j]
    return torch.cat([torch.stack(t, 1), torch.stack(q, 1), torch.stack(s, 1)[..., None]], dim=-1)


def loss(skel, cons, poses, scales, global_scaling=1.0, dtype=torch.float64, directions=None):
    """[N]: sum over the constraints of reach w/2 |p - y|^2 and aim w (1 - rot(q, axis) . d), p = global_scaling t,
    d = (y - p) / |y - p| detached; an aim whose point is the joint contributes 0.  `directions` [N, K, 3]: the aims' d, frozen
    (what a finite difference of the loss must hold still to see the gradient the definition gives: aim_directions)."""
    st = joint_states(skel, poses, scales, dtype)
    g = _t(np.broadcast_to(np.asarray(global_scaling, np.float64), (3,)).copy(), dtype)
    y, w = _t(cons["targets"], dtype), _t(cons["weights"], dtype)
    total = torch.zeros(st.shape[0], dtype=dtype)
    for k, (j, kind) in enumerate(zip(cons["joints"], cons["kinds"])):
        p = st[:, j, 0:3] * g
        if kind == REACH:
            total = total + 0.5 * w[:, k] * ((p - y[:, k]) ** 2).sum(-1)
        else:
            e = (y[:, k] - p).detach()
            n = e.norm(dim=-1, keepdim=True)
            ok = n[:, 0] > 0
            d = torch.where(ok[:, None], e / torch.where(ok[:, None], n, torch.ones_like(n)), torch.zeros_like(e))
            if directions is not None:
                d = _t(directions, dtype)[:, k]
                ok = d.abs().sum(-1) > 0
            r = qrot(st[:, j, 3:7], _t(cons["axes"][k], dtype)[None].expand_as(e))
            total = total + torch.where(ok, w[:, k] * (1 - (r * d).sum(-1)), torch.zeros_like(n[:, 0]))
    return total


def aim_directions(skel, cons, poses, scales, global_scaling=1.0, dtype=torch.float64):
    """[N, K, 3]: d = (y - p) / |y - p| of every constraint at `poses` (0 where y = p)."""
    st = joint_states(skel, _t(poses, dtype), scales, dtype)
    g = _t(np.broadcast_to(np.asarray(global_scaling, np.float64), (3,)).copy(), dtype)
    e = _t(cons["targets"], dtype) - st[:, cons["joints"], 0:3] * g
    n = e.norm(dim=-1, keepdim=True)
    return torch.where(n > 0, e / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(e))


def loss_grad(skel, cons, z, scales, mean=None, std=None, global_scaling=1.0, dtype=torch.float64):
    """(L [N], dL/dz [N, P_pos]) with theta = mean + std z (autograd)."""
    z = _t(z, dtype).clone().requires_grad_(True)
    m = 0 if mean is None else _t(mean, dtype)
    s = 1 if std is None else _t(std, dtype)
    L = loss(skel, cons, m + s * z, scales, global_scaling, dtype)
    (g,) = torch.autograd.grad(L.sum(), z)
    return L.detach(), g


def descend(skel, cons, z, scales, iterations, alpha=1.0, max_step=0.25, mean=None, std=None, global_scaling=1.0,
            dtype=torch.float64):
    """(z after `iterations` of z <- z - min(alpha L / |g|^2, max_step / |g|inf) g, branches): branches [iterations, N] is 0 where
    the frame stayed (L = 0, g = 0 or non-finite), 1 where Polyak's step was taken, 2 where the trust region cut it."""
    z = _t(z, dtype).clone()
    branches = np.zeros((iterations, z.shape[0]), np.int64)
    for it in range(iterations):
        L, g = loss_grad(skel, cons, z, scales, mean, std, global_scaling, dtype)
        g2, gm = (g * g).sum(-1), g.abs().amax(-1)
        ok = (L > 0) & (g2 > 0) & torch.isfinite(L) & torch.isfinite(g2)
        one = torch.ones_like(g2)
        polyak = alpha * L / torch.where(ok, g2, one)
        trust = max_step / torch.where(ok, gm, one)
        step = torch.where(ok, torch.minimum(polyak, trust), torch.zeros_like(g2))
        branches[it] = np.where(ok.numpy(), np.where((trust < polyak).numpy(), 2, 1), 0)
        z = z - step[:, None] * torch.where(ok[:, None], g, torch.zeros_like(g))
    return z, branches


def residual(skel, cons, poses, scales, global_scaling=1.0, dtype=torch.float64):
    """[N, K]: the distance |p - y| of a reach, 1 - cos of an aim (0 when the point is the joint)."""
    st = joint_states(skel, _t(poses, dtype), scales, dtype)
    g = _t(np.broadcast_to(np.asarray(global_scaling, np.float64), (3,)).copy(), dtype)
    y = _t(cons["targets"], dtype)
    out = []
    for k, (j, kind) in enumerate(zip(cons["joints"], cons["kinds"])):
        e = y[:, k] - st[:, j, 0:3] * g
        n = e.norm(dim=-1)
        if kind == REACH:
            out.append(n)
        else:
            r = qrot(st[:, j, 3:7], _t(cons["axes"][k], dtype)[None].expand_as(e))
            out.append(torch.where(n > 0, 1 - (r * e).sum(-1) / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(n)))
    return torch.stack(out, dim=1)


def ddim_update(x0, x, noise, tables, t, eta, dtype=torch.float64):
    """The DDIM update of pred_xstart x0 at step index t (tables: dict of float64 rows by a2p_table_id name)."""
    sra, srm1 = tables["sqrt_recip_alphas_cumprod"][t], tables["sqrt_recipm1_alphas_cumprod"][t]
    ab, abp = tables["alphas_cumprod"][t], tables["alphas_cumprod_prev"][t]
    eps = (sra * x - x0) / srm1
    sigma = eta * np.sqrt((1 - abp) / (1 - ab)) * np.sqrt(1 - ab / abp)
    out = x0 * np.sqrt(abp) + np.sqrt(1 - abp - sigma ** 2) * eps
    return out + (sigma * noise if t != 0 and noise is not None else 0)


def ddpm_update(x0, x, noise, tables, t, dtype=torch.float64):
    mean = tables["posterior_mean_coef1"][t] * x0 + tables["posterior_mean_coef2"][t] * x
    return mean + (np.exp(0.5 * tables["posterior_log_variance_clipped"][t]) * noise if t != 0 else 0)


def make_constraints(skel, scales, N, spec, seed, dtype=np.float32):
    """Constraints for tests: `spec` is a list of (joint, kind, weight) with weight a number or [N]; reach targets are the joint's
    positions under another random pose (reachable), aim points are random points a unit or so away; axes are random unit vectors."""
    rs = np.random.RandomState(seed)
    P_pos = int(skel["nr_position_params"])
    other = (rs.randn(N, P_pos) * 0.6).astype(np.float32)
    pos = joint_states(skel, _t(other, torch.float64), scales)[:, :, 0:3].numpy()
    K = len(spec)
    targets, weights, axes = np.zeros((N, K, 3), dtype), np.zeros((N, K), dtype), np.zeros((K, 3), np.float32)
    for k, (j, kind, w) in enumerate(spec):
        targets[:, k] = pos[:, j] if kind == REACH else pos[:, j] + rs.randn(N, 3)
        weights[:, k] = w
        a = rs.randn(3)
        axes[k] = a / np.linalg.norm(a)
    return {"joints": [s[0] for s in spec], "kinds": [s[1] for s in spec], "axes": axes, "targets": targets, "weights": weights}
