"""Posed geometry, host side (no GPU): the float64 restatement (tests/skinning_restatement.py) against the reference's fixture
(tests/golden/golden_skinning_v1.npz), and what BodySkeleton prepares and rejects before anything reaches a kernel."""
import os

import numpy as np
import pytest
import torch

import skinning_restatement as R
from audio2photoreal_amd import _lib
from audio2photoreal_amd import skinning as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_skinning_v1.npz"))


def _skel(gold):
    return {k.split("/", 1)[1]: gold[k] for k in gold.files if k.startswith("skel/")}


def _build(skel, **kw):
    args = dict(parents=skel["parents"], pre_rotation=skel["pre_rotation"], joint_offset=skel["joint_offset"],
                transform=skel["transform"], transform_offsets=skel["transform_offsets"],
                nr_position_params=int(skel["nr_position_params"]), nr_scaling_params=int(skel["nr_scaling_params"]),
                rest_vertices=skel["rest_vertices"], skin_indices=skel["skin_indices"], skin_weights=skel["skin_weights"])
    args.update(kw)
    return S.BodySkeleton.from_arrays(**args)


# ------------------------------------------------------------------------------------------------ restatement == reference
def test_restatement_reproduces_the_reference(gold):
    """The float64 restatement against the reference's float32 outputs, within 4 x the error stored with them (which is this
    very difference, measured when the fixture was made): the restatement and the stored reference belong together."""
    skel = _skel(gold)
    poses, scales = gold["poses"], gold["scales"]
    got = {"states": R.joint_states(skel, poses, scales), "matrices": R.transforms(skel, poses, scales),
           "vertices": R.pose_vertices(skel, poses, scales, gold["verts_unposed"], gold["template_verts"], gold["global_scaling"])}
    for k, v in got.items():
        e = R.nerr(gold[f"ref/{k}"], v)
        assert 0 < float(gold[f"e_ref/{k}"]) < 1e-5, k                       # a float32 rounding error, not a formula error
        assert e <= 4 * float(gold[f"e_ref/{k}"]), (k, e)
    assert R.nerr(gold["ref/bind_state"], R.bind_state(skel)) <= 4 * float(gold["e_ref/states"])
    sk = _build(skel)
    assert R.nerr(sk.bind_state[None], R.bind_state(skel)) <= 1e-14           # the product's float64 bind state
    # bind o bind^-1 is the identity up to how far the float32 pre-rotations are from unit length (the formulas do not normalise)
    inv = R.states_to_matrix(R.bind_state(skel), R.bind_state(skel))
    assert np.abs(inv - np.eye(3, 4)[None, None]).max() <= 1e-5


def test_from_model_and_static_assets_match_from_arrays(gold):
    skel = _skel(gold)
    J = skel["parents"].size
    bones = [{"Name": f"b{j}", "Parent": int(skel["parents"][j]) if skel["parents"][j] >= 0 else 2 ** 31,
              "PreRotation": skel["pre_rotation"][j].tolist(), "TranslationOffset": skel["joint_offset"][j].tolist()} for j in range(J)]
    pairs = [[int(i), float(w)] for i, w in zip(gold["ragged/indices"], gold["ragged/weights"])]
    model = {"Skeleton": {"Bones": bones}, "SkinnedModel": {"RestPositions": skel["rest_vertices"].tolist(), "SkinningWeights": pairs,
                                                            "SkinningOffsets": gold["ragged/offsets"].tolist()}}
    cfg = {"transform": skel["transform"], "transform_offsets": skel["transform_offsets"].reshape(1, -1),
           "nr_scaling_params": int(skel["nr_scaling_params"]), "nr_position_params": int(skel["nr_position_params"])}
    a = S.BodySkeleton.from_static_assets({"lbs_model_json": model, "lbs_config_dict": cfg, "lbs_template_verts": torch.from_numpy(gold["template_verts"]),
                                           "lbs_scale": torch.from_numpy(gold["scales"][0]), "global_scaling": gold["global_scaling"].tolist()})
    b = _build(skel)
    for k in ("parents", "order", "level_start", "skin_indices", "skin_weights", "row_ptr", "cols", "vals", "bind_state", "inv_bind"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.joint_names[3] == "b3" and (a.J, a.V, a.K) == (40, 500, 8)
    assert np.array_equal(a.template_verts, gold["template_verts"]) and np.array_equal(a.global_scaling, gold["global_scaling"])
    assert np.array_equal(a.lbs_scale, gold["scales"][0]) and b.template_verts is None and np.array_equal(b.global_scaling, np.ones(3))
    assert np.array_equal(S.BodySkeleton.from_model(model, cfg, global_scaling=2.0).global_scaling, np.full(3, 2.0))


# ------------------------------------------------------------------------------------------------ packing, roots, levels
def test_packing_keeps_the_first_k_unrenormalised():
    idx = [3, 1, 4, 1, 5, 9, 2, 6, 5, 3]
    w = [0.1, 0.2, 0.3, 0.05, 0.05, 0.3, 1.0, 0.5, 0.25, 0.25]
    pi, pw = S.pack_skinning(idx, w, [0, 6, 7, 7, 10], num_max_skin_joints=4)
    assert pi.tolist() == [[3, 1, 4, 1], [2, 0, 0, 0], [0, 0, 0, 0], [6, 5, 3, 0]]
    assert np.array_equal(pw, np.array([[0.1, 0.2, 0.3, 0.05], [1, 0, 0, 0], [0, 0, 0, 0], [0.5, 0.25, 0.25, 0]], np.float32))
    assert abs(pw[0].sum() - 0.65) < 1e-6                                     # six influences, four kept: the weights are NOT rescaled
    with pytest.raises(ValueError, match=r"SkinningOffsets\[2\]"):
        S.pack_skinning(idx, w, [0, 6, 5, 10], 4)
    with pytest.raises(ValueError, match="SkinningOffsets"):
        S.pack_skinning(idx, w, [0, 6, 11], 4)


def test_out_of_range_parents_are_roots_and_levels_follow_parents(gold):
    assert S.normalise_parents([7, 0, -3, 1, 6, 2]).tolist() == [-1, 0, -1, 1, -1, 2]        # J = 6: negative and >= 6 are roots
    order, start, depth = S.level_schedule([-1, 0, 99, 1, 2, 0, 5])
    assert depth.tolist() == [0, 1, 0, 2, 1, 1, 2] and order.tolist() == [0, 2, 1, 4, 5, 3, 6] and start.tolist() == [0, 2, 5, 7]
    for parents in (_skel(gold)["parents"], np.arange(-1, 32), np.r_[-1, np.zeros(129, np.int64)], [-1, 0, -1, 2, 1, 3]):
        p = S.normalise_parents(parents)
        order, start, depth = S.level_schedule(parents)
        assert sorted(order.tolist()) == list(range(p.size)) and start[0] == 0 and start[-1] == p.size
        level_of = np.empty(p.size, np.int64)
        for lvl in range(start.size - 1):
            assert start[lvl + 1] > start[lvl]                                # no empty level
            level_of[order[start[lvl]:start[lvl + 1]]] = lvl
        assert np.array_equal(level_of, depth)
        assert all(level_of[j] == (0 if p[j] < 0 else level_of[p[j]] + 1) for j in range(p.size))
    assert S.level_schedule(np.arange(-1, 32))[1].size == 34                  # a chain of 33: as many levels as joints


def test_compressed_transform_equals_the_dense_one(gold):
    tr = _skel(gold)["transform"]
    row_ptr, cols, vals = S.compress_transform(tr)
    assert row_ptr[-1] == np.count_nonzero(tr) == vals.size and vals.size < tr.size // 20
    assert all(np.all(np.diff(cols[row_ptr[r]:row_ptr[r + 1]]) > 0) for r in range(tr.shape[0]))
    x = np.random.RandomState(0).randn(5, tr.shape[1])
    assert np.abs(S.apply_compressed(row_ptr, cols, vals, x) - x @ tr.astype(np.float64).T).max() <= 1e-13
    dense = np.random.RandomState(1).randn(14, 9).astype(np.float32)
    dense[3] = 0                                                              # an empty row
    rp, c, v = S.compress_transform(dense)
    assert rp[3] == rp[4] and np.abs(S.apply_compressed(rp, c, v, x[:, :9]) - x[:, :9] @ dense.astype(np.float64).T).max() <= 1e-13


# ------------------------------------------------------------------------------------------------ rejections
def test_every_rejection_names_the_offending_entry(gold):
    skel = _skel(gold)
    J, V = skel["parents"].size, skel["rest_vertices"].shape[0]
    parents = skel["parents"].copy()
    parents[5] = 9
    with pytest.raises(ValueError, match="joint 5: parent 9 does not precede"):
        _build(skel, parents=parents)
    parents[5] = 5
    with pytest.raises(ValueError, match="joint 5: parent 5"):
        _build(skel, parents=parents)
    for bad in (J, -1, 10 ** 6):
        idx = skel["skin_indices"].copy()
        idx[17, 2] = bad
        with pytest.raises(ValueError, match=rf"skin_indices\[17, 2\] = {bad} is outside \[0, J={J}\)"):
            _build(skel, skin_indices=idx)
    for name, where, pat in (("pre_rotation", (3, 1), r"pre_rotation\[3, 1\]"), ("joint_offset", (39, 2), r"joint_offset\[39, 2\]"),
                             ("transform", (8, 100), r"transform\[8, 100\]"), ("transform_offsets", (11,), r"transform_offsets\[11\]"),
                             ("rest_vertices", (499, 0), r"rest_vertices\[499, 0\]"), ("skin_weights", (0, 7), r"skin_weights\[0, 7\]")):
        for v in (np.nan, np.inf):
            a = skel[name].copy()
            a[where] = v
            with pytest.raises(ValueError, match=pat + " is not finite"):
                _build(skel, **{name: a})
    t = gold["template_verts"].copy()
    t[4, 1] = np.nan
    with pytest.raises(ValueError, match=r"template_verts\[4, 1\]"):
        _build(skel, template_verts=t)
    with pytest.raises(ValueError, match=r"lbs_scale\[2\]"):
        _build(skel, lbs_scale=np.r_[0.0, 0.0, np.inf, np.zeros(9)])
    with pytest.raises(ValueError, match=r"global_scaling\[1\]"):
        _build(skel, global_scaling=[1.0, np.nan, 1.0])
    Jbig = _lib.SKIN_MAX_JOINTS + 1
    with pytest.raises(ValueError, match=f"J={Jbig} joints"):
        S.BodySkeleton.from_arrays(np.arange(-1, Jbig - 1), np.tile([0, 0, 0, 1.0], (Jbig, 1)), np.zeros((Jbig, 3)),
                                   np.zeros((7 * Jbig, 4)), np.zeros(7 * Jbig), 4, 0, np.zeros((1, 3)), np.zeros((1, 1), np.int64), np.ones((1, 1)))
    with pytest.raises(ValueError, match="K=17 influences"):
        _build(skel, skin_indices=np.zeros((V, 17), np.int64), skin_weights=np.zeros((V, 17), np.float32))
    with pytest.raises(ValueError, match="num_max_skin_joints=17"):
        S.BodySkeleton.from_model({}, {}, num_max_skin_joints=17)
    with pytest.raises(ValueError, match=r"expected \[7 J, P\] = \[280, 116\]"):
        _build(skel, transform=skel["transform"][:, :-1])
    q = skel["pre_rotation"].copy()
    q[6] = 0                                                                  # a zero quaternion has no inverse: the bind state
    with pytest.raises(ValueError, match="bind"):
        _build(skel, pre_rotation=q)
    sk = _build(skel)
    with pytest.raises(_lib.A2PError, match="no CPU implementation"):         # the methods never compute on the host
        sk.joint_states(torch.zeros(2, 104))
    with pytest.raises(_lib.A2PError, match="no CPU implementation"):
        sk.skin(torch.zeros(2, J, 3, 4))
    for call in (sk.joint_states, sk.transforms, sk.pose_vertices, sk.joint_positions, sk.skin):
        with pytest.raises(_lib.A2PError, match="must be a tensor"):         # an array is refused by every entry point alike
            call(np.zeros((2, J, 3, 4), np.float32))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.A2PError, match="no CPU implementation"):
            S.pose_motion(sk, np.zeros((1, 2, 104), np.float32))


def test_the_new_exports_are_bound():
    assert {"a2p_skin_states", "a2p_skin_vertices"} <= set(_lib.EXPORTS)
    src = open(os.path.join(ROOT, "include", "a2p_hip.h")).read()
    for name, val in (("JOINTS", _lib.SKIN_MAX_JOINTS), ("PARAMS", _lib.SKIN_MAX_PARAMS), ("INFLUENCES", _lib.SKIN_MAX_INFLUENCES)):
        assert f"#define A2P_SKIN_MAX_{name} {val}\n" in src


# ------------------------------------------------------------------------------------------------ pose_motion layouts
def test_every_motion_layout_gives_the_same_frames():
    rs = np.random.RandomState(3)
    pose = rs.randn(2, 5, 104)                                                # the generators' "pose": [B, T, 104] float64
    flat, lead = S.motion_frames(pose)
    assert flat.dtype == np.float32 and flat.shape == (10, 104) and lead == (2, 5)
    assert np.array_equal(flat, pose.astype(np.float32).reshape(10, 104))
    sampler = torch.from_numpy(pose).permute(0, 2, 1)[:, :, None, :]         # [B, 104, 1, T]
    f2, lead2 = S.motion_frames(sampler)
    assert torch.is_tensor(f2) and f2.dtype == torch.float32 and f2.is_contiguous() and lead2 == (2, 5)
    assert np.array_equal(f2.numpy(), flat)
    f3, lead3 = S.motion_frames(sampler.numpy())
    assert np.array_equal(f3, flat) and lead3 == (2, 5)
    f4, lead4 = S.motion_frames(torch.from_numpy(flat))
    assert np.array_equal(f4.numpy(), flat) and lead4 == (10,)
    f5, lead5 = S.motion_frames(rs.randn(104, 104, 1, 3).astype(np.float32))   # B == 104 is still the sampler layout
    assert f5.shape == (312, 104) and lead5 == (104, 3)
    for bad in (np.zeros((2, 5, 103)), np.zeros((2, 104, 2, 5)), np.zeros(104), [[0.0] * 104]):
        with pytest.raises(_lib.A2PError):
            S.motion_frames(bad)
