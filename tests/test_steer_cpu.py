"""Joint steering, host side (no GPU): the float64 restatement (tests/steer_restatement.py) against skinning_restatement and
against central differences, JointTargets' validation and ramps, the host tables of the backward pass, every refusal, and the
exports of the built library."""
import ctypes
import os

import numpy as np
import pytest
import torch

import skinning_restatement as R
import steer_restatement as SR
from audio2photoreal_amd import _lib
from audio2photoreal_amd import skinning as S
from audio2photoreal_amd.sample import steer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(skel, **kw):
    return S.BodySkeleton.from_arrays(skel["parents"], skel["pre_rotation"], skel["joint_offset"], skel["transform"],
                                      skel["transform_offsets"], int(skel["nr_position_params"]), int(skel["nr_scaling_params"]),
                                      skel["rest_vertices"], skel["skin_indices"], skel["skin_weights"], **kw)


@pytest.fixture(scope="module")
def sk23():
    skel = R.make_skeleton(4, 23, 16, 4)
    return skel, build(skel, lbs_scale=R.make_inputs(11, 1)[1][0])


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("J,parents", [(1, None), (5, [-1, 0, 1, 1, 3]), (23, None), (160, None)])
def test_restatement_states_match_the_numpy_restatement(J, parents):
    skel = R.make_skeleton(J, J, 8, 2, parents=parents)
    poses, scales = R.make_inputs(3, 5)
    want = R.joint_states(skel, poses, scales)
    got = SR.joint_states(skel, torch.from_numpy(poses), scales).numpy()
    assert np.abs(got - want).max() <= 1e-12


def test_autograd_gradient_matches_central_differences(sk23):
    skel, _ = sk23
    N = 3
    poses, scales = R.make_inputs(5, N)
    cons = SR.make_constraints(skel, scales, N, [(22, SR.REACH, 1.0), (22, SR.AIM, 0.7), (7, SR.AIM, 2.0), (0, SR.REACH, 0.5)], 9)
    rs = np.random.RandomState(1)
    mean, std = rs.randn(104) * 0.1, rs.uniform(0.3, 1.5, 104)
    g = np.array([1.5, 0.5, 2.0])
    _, grad = SR.loss_grad(skel, cons, poses, scales, mean, std, g)
    z = torch.from_numpy(poses).double()
    d = SR.aim_directions(skel, cons, torch.from_numpy(mean) + torch.from_numpy(std) * z, scales, g)   # held constant by definition
    h = 1e-6
    num = np.zeros((N, 104))
    for i in range(104):
        e = torch.zeros(104, dtype=torch.float64)
        e[i] = h
        m, s = torch.from_numpy(mean), torch.from_numpy(std)
        num[:, i] = ((SR.loss(skel, cons, m + s * (z + e), scales, g, directions=d)
                      - SR.loss(skel, cons, m + s * (z - e), scales, g, directions=d)) / (2 * h)).numpy()
    assert R.nerr(grad.numpy(), num) <= 1e-7          # (central differences at h = 1e-6 in float64: h^2 truncation, 1e-10 / h rounding)


def test_descent_lowers_a_reachable_loss_and_records_its_branches(sk23):
    skel, _ = sk23
    poses, scales = R.make_inputs(5, 4)
    cons = SR.make_constraints(skel, scales, 4, [(22, SR.REACH, 1.0), (10, SR.REACH, 1.0), (15, SR.REACH, 1.0)], 9)
    L0 = SR.loss(skel, cons, torch.from_numpy(poses), scales)
    z, br = SR.descend(skel, cons, poses, scales, 8)
    assert br.shape == (8, 4) and set(np.unique(br)) <= {1, 2}
    assert float(SR.loss(skel, cons, z, scales).mean()) < 0.5 * float(L0.mean())
    # no element moves more than max_step per iteration
    z1, _ = SR.descend(skel, cons, poses, scales, 1, max_step=0.25)
    assert float((z1 - torch.from_numpy(poses)).abs().max()) <= 0.25 + 1e-12
    # all-zero weights: the frame stays, branch 0
    cons["weights"][:] = 0
    z0, br0 = SR.descend(skel, cons, poses, scales, 2)
    assert (br0 == 0).all() and torch.equal(z0, torch.from_numpy(poses).double())


# ------------------------------------------------------------------------------------------------ host tables
def test_child_lists_and_compressed_columns(sk23):
    skel, sk = sk23
    cp, ci = S.child_list([-1, 0, 1, 1, 3, 99])
    assert cp.tolist() == [0, 1, 3, 3, 4, 4, 4] and ci.tolist() == [1, 2, 3, 4]          # 99 >= J marks a second root
    for j in range(sk.J):
        kids = sk.child_idx[sk.child_ptr[j]:sk.child_ptr[j + 1]]
        assert kids.tolist() == sorted(np.nonzero(sk.parents == j)[0].tolist())
    dense = np.zeros((7 * sk.J, sk.P_pos), np.float32)
    for c in range(sk.P_pos):
        rows = sk.col_rows[sk.col_ptr[c]:sk.col_ptr[c + 1]]
        assert (np.diff(rows) > 0).all()
        dense[rows, c] = sk.col_vals[sk.col_ptr[c]:sk.col_ptr[c + 1]]
    assert np.array_equal(dense, skel["transform"][:, :sk.P_pos])


# ------------------------------------------------------------------------------------------------ JointTargets
def test_ramp_shape():
    idx = np.arange(10, 14)
    w = steer.ramp_weights(30, idx, 2.0, 3)
    want = np.zeros(30, np.float32)
    want[10:14] = 2.0
    want[[9, 14]], want[[8, 15]], want[[7, 16]] = 1.5, 1.0, 0.5
    assert np.allclose(w, want, atol=1e-7) and w[6] == 0 and w[17] == 0
    assert np.array_equal(steer.ramp_weights(30, idx, 2.0, 0), np.where((np.arange(30) >= 10) & (np.arange(30) < 14), 2.0, 0.0))
    # cut at the ends of the clip
    assert np.allclose(steer.ramp_weights(5, np.array([0]), 1.0, 9), 1 - np.arange(5) / 10)


def test_joint_targets_build_dense_tensors(sk23):
    _, sk = sk23
    B, T = 2, 20
    jt = steer.JointTargets(sk, B, T)
    pts = np.arange(B * 4 * 3, dtype=np.float64).reshape(B, 4, 3)
    jt.reach("joint5", slice(8, 12), pts, weight=2.0, ramp=2).aim(3, np.array([0, 19]), [1.0, 2.0, 3.0], axis=(0, 1, 0))
    targets, weights = jt.dense()
    assert targets.shape == (B, T, 2, 3) and weights.shape == (B, T, 2) and targets.dtype == weights.dtype == np.float32
    assert np.array_equal(targets[:, 8:12, 0], pts.astype(np.float32))
    assert np.array_equal(targets[:, 6, 0], pts[:, 0]) and np.array_equal(targets[:, 13, 0], pts[:, 3])      # the ramp holds the nearest target
    assert np.allclose(weights[0, :, 0], steer.ramp_weights(T, np.arange(8, 12), 2.0, 2)) and weights[1, 5, 0] == 0
    assert weights[:, :, 1].sum() == 2 * B and (targets[:, [0, 19], 1] == np.float32([1, 2, 3])).all()
    cons = jt.constraints()
    assert (cons.N, cons.K, cons.joints, cons.kinds) == (B * T, 2, [5, 3], [S.REACH, S.AIM])
    assert torch.equal(cons.targets.reshape(B, T, 2, 3), torch.from_numpy(targets))


def test_joint_targets_validation(sk23):
    _, sk = sk23
    new = lambda: steer.JointTargets(sk, 2, 20)
    ok = (0, slice(0, 5), [0.0, 0.0, 0.0])
    for bad, match in (
            (lambda: new().reach("nose", *ok[1:]), "unknown joint"),
            (lambda: new().reach(23, *ok[1:]), "unknown joint"),
            (lambda: new().reach(-1, *ok[1:]), "unknown joint"),
            (lambda: new().aim(*ok, axis=(0, 0, 0)), "unit"),
            (lambda: new().aim(*ok, axis=(0, 0, 2)), "unit"),
            (lambda: new().aim(*ok, axis=(0, np.nan, 1)), "unit"),
            (lambda: new().reach(*ok, weight=-1.0), "weight"),
            (lambda: new().reach(*ok, weight=float("inf")), "weight"),
            (lambda: new().reach(*ok, weight=float("nan")), "weight"),
            (lambda: new().reach(0, np.array([3, 20]), ok[2]), r"outside \[0, 20\)"),
            (lambda: new().reach(0, np.array([-1]), ok[2]), r"outside \[0, 20\)"),
            (lambda: new().reach(0, slice(10, 25), ok[2]), r"outside \[0, 20\)"),
            (lambda: new().reach(0, np.array([3, 3]), ok[2]), "twice"),
            (lambda: new().reach(0, slice(5, 5), ok[2]), "no frame"),
            (lambda: new().reach(0, slice(0, 5), np.zeros((4, 3))), "target must be"),
            (lambda: new().reach(0, slice(0, 5), [0.0, np.inf, 0.0]), "non-finite"),
            (lambda: new().reach(*ok, ramp=-1), "ramp"),
            (lambda: new().dense(), "no constraint"),
            (lambda: steer.JointTargets(object(), 1, 1), "BodySkeleton")):
        with pytest.raises(_lib.A2PError, match=match):
            bad()
    jt = new()
    for _ in range(_lib.STEER_MAX_CONSTRAINTS):
        jt.reach(*ok)
    with pytest.raises(_lib.A2PError, match="more than 16"):
        jt.reach(*ok)


def test_joint_constraints_validation():
    t, w = np.zeros((4, 1, 3), np.float32), np.ones((4, 1), np.float32)
    for bad, match in ((lambda: S.JointConstraints([5], [S.REACH], np.zeros((1, 3)), t, w, 5), "outside"),
                       (lambda: S.JointConstraints([0], [2], np.zeros((1, 3)), t, w, 5), "neither"),
                       (lambda: S.JointConstraints([0], [S.AIM], np.zeros((1, 3)), t, w, 5), "unit"),
                       (lambda: S.JointConstraints([0], [S.REACH], np.zeros((1, 3)), t, -w, 5), "weights"),
                       (lambda: S.JointConstraints([0], [S.REACH], np.zeros((1, 3)), t[:3], w, 5), "targets must be"),
                       (lambda: S.JointConstraints([0] * 17, [S.REACH] * 17, np.zeros((17, 3)), np.zeros((4, 17, 3)), np.ones((4, 17))), "17 constraints")):
        with pytest.raises(_lib.A2PError, match=match):
            bad()


# ------------------------------------------------------------------------------------------------ refusals before any GPU work
class _Model:
    nfeats = 104

    def a2p_sample_step_steer(self, *a, **k):
        raise AssertionError("no GPU work expected")


def test_the_loop_refuses_what_is_out_of_scope(sk23):
    _, sk = sk23
    B, T = 1, 8
    jt = steer.JointTargets(sk, B, T).reach(0, slice(0, T), [0.0, 0.0, 0.0])
    noise = torch.zeros(B, 104, 1, T)
    mean, std = np.zeros(104), np.ones(104)
    call = lambda **kw: steer.steered_sample_loop(None, kw.pop("model", _Model()), {}, sk, mean, std, kw.pop("targets", jt),
                                                  kw.pop("noise", noise), **kw)
    for kw, match in (({"sampler": "dpm++2m"}, "dpm\\+\\+2m"), ({"sampler": "plms"}, "PLMS"), ({"sampler": "euler"}, "unknown sampler"),
                      ({"known": noise, "known_mask": noise > 0}, "held elements"),
                      ({"model": object()}, "a2p_sample_step_steer"),
                      ({"targets": steer.JointTargets(sk, B, T + 1).reach(0, slice(0, 1), [0.0, 0.0, 0.0])}, "targets cover"),
                      ({"targets": steer.JointTargets(build(R.make_skeleton(4, 23, 16, 4)), B, T).reach(0, slice(0, 1), [0.0, 0.0, 0.0])},
                       "built on"),
                      ({"noise": torch.zeros(B, 50, 1, T)}, "channels"),
                      ({"noise": noise}, "MI355X")):                                        # everything valid but the device: the last check
        with pytest.raises(_lib.A2PError, match=match):
            call(**kw)
    long_model = _Model()
    long_model.seq_len = 4
    with pytest.raises(_lib.A2PError, match="windowed"):
        call(model=long_model)


def test_generate_steered_refuses_samplers_before_touching_the_models(sk23):
    _, sk = sk23
    for sampler in ("dpm++2m", "plms"):
        with pytest.raises(_lib.A2PError, match="out of scope"):
            steer.generate_steered(None, None, {}, None, 48000, sk, None, sampler=sampler)


def test_descent_arguments_are_checked_on_the_host(sk23):
    _, sk = sk23
    cons = S.JointConstraints([0], [S.REACH], np.zeros((1, 3)), np.zeros((2, 1, 3), np.float32), np.ones((2, 1), np.float32), sk.J)
    t = sk._tables("cpu")
    tg, w = cons.on("cpu")
    for kw, match in (({"iterations": -1}, "iterations"), ({"alpha": 0.0}, "alpha"), ({"max_step": float("nan")}, "max_step")):
        args = {"alpha": 1.0, "iterations": 2, "max_step": 0.25, **kw}
        with pytest.raises(_lib.A2PError, match=match):
            sk.steer_description(t, cons, tg, w, None, None, t["lbs_scale"], 0, args["alpha"], args["iterations"], args["max_step"])
    d, keep = sk.steer_description(t, cons, tg, w, None, None, t["lbs_scale"], 0, 1.0, 2, 0.25)
    assert (d.J, d.P_pos, d.P_scale, d.K, d.iterations, d.n_levels) == (sk.J, 104, 12, 1, 2, sk.level_start.size - 1)
    assert d.targets == tg.data_ptr() and d.joints_host[0] == 0 and list(d.global_scaling) == [1.0, 1.0, 1.0]


# ------------------------------------------------------------------------------------------------ the library
def test_the_new_symbols_are_exported_by_the_built_library():
    assert {"a2p_skin_steer", "a2p_sample_step_steer"} <= set(_lib.EXPORTS)
    src = open(os.path.join(ROOT, "include", "a2p_hip.h")).read()
    assert f"#define A2P_STEER_MAX_CONSTRAINTS {_lib.STEER_MAX_CONSTRAINTS}\n" in src
    assert "enum a2p_steer_kind { A2P_STEER_REACH = %d, A2P_STEER_AIM = %d };" % (_lib.STEER_REACH, _lib.STEER_AIM) in src
    for path in (_lib.LIB_PATH, _lib.LIB_PATH_F16):
        lib = ctypes.CDLL(path)
        for name in ("a2p_skin_steer", "a2p_sample_step_steer"):
            assert hasattr(lib, name), (path, name)
    # the struct the binding passes is the header's: 22 pointers, 5 floats, 7 int32 (8-byte aligned)
    assert ctypes.sizeof(_lib.A2PSteer) == 22 * 8 + 5 * 4 + 7 * 4
