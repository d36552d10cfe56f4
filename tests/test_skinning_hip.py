"""Posed geometry on the MI355X (csrc/kernels_skin.h, audio2photoreal_amd/skinning.py) against the float64 restatement
(tests/skinning_restatement.py).

Gate: the normalised error of every output (max |difference| / max |value|) is at most 4 x the float32 error of the same formulas
on the same skeleton: for the fixture skeleton the reference's own error stored in tests/golden/golden_skinning_v1.npz (e_ref),
for every other skeleton the restatement run in float32 against itself in float64.  The factor 4 pays for a different summation
order and for the device's sinf / cosf / exp2f.  No number is hard-coded; every measured value goes to record(...) beside its allowance
(the skin_* entries; a copy of them is what profiles/skinning_parity.json is meant to hold)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import skinning_restatement as R
from audio2photoreal_amd import skinning as S
from conftest import record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P_POS, P_SCALE = 104, 12


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_skinning_v1.npz"))


@pytest.fixture(scope="module")
def fix(gold):
    """The fixture skeleton (dict of arrays) and the product object built from it, with LBSModule's extras."""
    skel = {k.split("/", 1)[1]: gold[k] for k in gold.files if k.startswith("skel/")}
    return skel, build(skel, template_verts=gold["template_verts"], lbs_scale=gold["scales"][0], global_scaling=gold["global_scaling"])


def build(skel, **kw):
    return S.BodySkeleton.from_arrays(skel["parents"], skel["pre_rotation"], skel["joint_offset"], skel["transform"],
                                      skel["transform_offsets"], int(skel["nr_position_params"]), int(skel["nr_scaling_params"]),
                                      skel["rest_vertices"], skel["skin_indices"], skel["skin_weights"], **kw)


def gate(name, got, want, allowance):
    """Record and assert one output: got (device tensor) against want (float64) within `allowance` (normalised)."""
    err = R.nerr(got.cpu().numpy(), want)
    record(name, err=err, allowance=float(allowance))
    assert np.isfinite(err) and err <= allowance, (name, err, allowance)


def own_allowance(skel, poses, scales, **kw):
    """4 x (restatement in float32 against itself in float64) per output, for a skeleton that is not in the fixture."""
    f32, f64 = {}, {}
    for d, dt in ((f32, np.float32), (f64, np.float64)):
        d["states"] = R.joint_states(skel, poses, scales, dt)
        d["matrices"] = R.transforms(skel, poses, scales, dt)
        d["vertices"] = R.pose_vertices(skel, poses, scales, kw.get("verts_unposed"), kw.get("template_verts"), kw.get("global_scaling", 1.0), dt)
        d["joints"] = R.joint_positions(skel, poses, scales, kw.get("global_scaling", 1.0), dt)
    return f64, {k: 4 * R.nerr(f32[k], f64[k]) for k in f64}


def check_all(name, sk, skel, poses, scales, dev, **kw):
    """The four outputs of `sk` against the restatement, each within its own float32 allowance."""
    want, allow = own_allowance(skel, poses, scales, **kw)
    tp, ts = torch.from_numpy(poses).to(dev), torch.from_numpy(scales).to(dev)
    vu = kw.get("verts_unposed")
    got = {"states": sk.joint_states(tp, ts), "matrices": sk.transforms(tp, ts), "joints": sk.joint_positions(tp, ts),
           "vertices": sk.pose_vertices(tp, ts, None if vu is None else torch.from_numpy(vu).to(dev))}
    J, V = sk.J, sk.V
    assert got["states"].shape == (len(poses), J, 8) and got["matrices"].shape == (len(poses), J, 3, 4)
    assert got["joints"].shape == (len(poses), J, 3) and got["vertices"].shape == (len(poses), V, 3)
    for k in ("states", "matrices", "joints", "vertices"):
        gate(f"skin_{name}_{k}", got[k], want[k], allow[k])
    return got


# ------------------------------------------------------------------------------------------------ the fixture skeleton
def test_fixture_skeleton_within_four_times_the_references_own_error(dev, gold, fix):
    skel, sk = fix
    poses, scales = gold["poses"], gold["scales"]
    tp, ts = torch.from_numpy(poses).to(dev), torch.from_numpy(scales).to(dev)
    g = gold["global_scaling"]
    want = {"states": R.joint_states(skel, poses, scales), "matrices": R.transforms(skel, poses, scales),
            "vertices": R.pose_vertices(skel, poses, scales, gold["verts_unposed"], gold["template_verts"], g),
            "joints": R.joint_positions(skel, poses, scales, g)}
    got = {"states": sk.joint_states(tp, ts), "matrices": sk.transforms(tp, ts), "joints": sk.joint_positions(tp, ts),
           "vertices": sk.pose_vertices(tp, ts, torch.from_numpy(gold["verts_unposed"]).to(dev))}
    e_ref = {k: float(gold[f"e_ref/{k}"]) for k in ("states", "matrices", "vertices")}
    # joint positions are the reference's state translations times global_scaling: its own error on that output, from its states
    e_ref["joints"] = R.nerr(gold["ref/states"][:, :, 0:3] * g, want["joints"])
    assert got["states"].shape == (8, 40, 8) and got["matrices"].shape == (8, 40, 3, 4)
    assert got["joints"].shape == (8, 40, 3) and got["vertices"].shape == (8, 500, 3)
    for k in ("states", "matrices", "vertices", "joints"):
        gate(f"skin_fixture_{k}", got[k], want[k], 4 * e_ref[k])
    assert torch.equal(sk.joint_states(tp), got["states"])                    # scales=None: the skeleton's lbs_scale


# ------------------------------------------------------------------------------------------------ topologies
TOPOLOGIES = {
    "root_only": dict(J=1, parents=[-1]),
    "chain33": dict(J=33, parents=list(range(-1, 32))),                       # as many levels as joints
    "star130": dict(J=130, parents=[-1] + [0] * 129),                         # one level wider than two waves
    "star300": dict(J=300, parents=[-1] + [0] * 299),                         # a level wider than the workgroup: a second pass
    "two_roots": dict(J=12, parents=[-1, 0, 1, 1, 2 ** 31, 4, 4, 5, 2, 6, 7, 3]),
    "cap1024": dict(J=1024, parents=None),                                    # the joint cap: the largest LDS footprint of both kernels
}


@pytest.mark.parametrize("name", list(TOPOLOGIES))
def test_topologies(dev, name):
    t = TOPOLOGIES[name]
    skel = R.make_skeleton(20 + t["J"], t["J"], 96, 4, parents=t["parents"])
    poses, scales = R.make_inputs(30 + t["J"], 16)
    sk = build(skel)
    levels = {"root_only": 1, "chain33": 33, "star130": 2, "star300": 2, "two_roots": 4}
    assert name not in levels or sk.level_start.size - 1 == levels[name]
    check_all(name, sk, skel, poses, scales, dev)


def test_scale_on_an_inner_joint_scales_children_matrices_and_vertices(dev):
    """Pose parameter 0 drives the `sc` channel of joint 1 alone; nothing else depends on it.  Every odd frame is the frame before
    it with sc 0 -> 1; the properties are checked on frames 0 and 1."""
    skel = R.make_skeleton(41, 5, 64, 2, parents=[-1, 0, 1, 1, 3], drive_scale=False)
    skel["transform"][:, 0] = 0
    skel["transform"][6::7] = 0
    skel["transform_offsets"][6::7] = 0                                       # bind scales 1
    skel["transform"][7 * 1 + 6, 0] = 1.0
    skel["skin_indices"][:] = 0
    skel["skin_weights"][:] = 0
    skel["skin_indices"][:, 0] = np.arange(64) % 5
    skel["skin_weights"][:, 0] = 1.0                                          # rigid vertices: vertex v follows joint v % 5
    poses, scales = R.make_inputs(42, 16)
    poses[1::2] = poses[0::2]
    poses[0::2, 0], poses[1::2, 0] = 0.0, 1.0
    sk = build(skel)
    got = check_all("inner_scale", sk, skel, poses, scales, dev)
    st, m, v = (got[k].double().cpu().numpy() for k in ("states", "matrices", "vertices"))
    assert np.allclose(st[:2, :, 7], [[1, 1, 1, 1, 1], [1, 2, 2, 2, 2]], rtol=1e-6, atol=0)
    assert np.array_equal(st[0, 0], st[1, 0]) and np.array_equal(st[0, 1, :7], st[1, 1, :7])     # the root and joint 1 do not move
    for child, parent in ((2, 1), (3, 1), (4, 3)):                            # offsets below joint 1 double
        assert np.allclose(st[1, child, :3] - st[1, 1, :3], 2 * (st[0, child, :3] - st[0, 1, :3]), rtol=1e-5, atol=1e-5), (child, parent)
    norms = np.linalg.norm(m[:, :, :, :3], axis=2)                            # column norms of the 3 x 3 block = s / bind_s
    assert np.allclose(norms[0], 1, atol=1e-5) and np.allclose(norms[1, 0], 1, atol=1e-5) and np.allclose(norms[1, 1:], 2, atol=1e-5)
    for vert in range(64):
        j = vert % 5
        if j == 0:
            assert np.array_equal(v[0, vert], v[1, vert])
        else:                                                                 # the vertex's offset from joint 1 doubles
            assert np.allclose(v[1, vert] - st[1, 1, :3], 2 * (v[0, vert] - st[0, 1, :3]), rtol=1e-5, atol=1e-5)


# ------------------------------------------------------------------------------------------------ vertex and influence counts
@pytest.mark.parametrize("V,K", [(1, 1), (257, 8), (257, 1), (1100, 3)])
def test_vertex_counts_and_influences(dev, V, K):
    skel = R.make_skeleton(50 + V + K, 20, V, K)
    if V > 5:
        skel["skin_weights"][5] = 0                                           # every slot of vertex 5 unused
        skel["skin_indices"][5] = 0
    poses, scales = R.make_inputs(60 + V, 16)
    got = check_all(f"V{V}_K{K}", build(skel), skel, poses, scales, dev)
    if V > 5:
        assert torch.equal(got["vertices"][:, 5], torch.zeros(16, 3, device=dev))
        assert float(got["vertices"][:, 4].abs().max()) > 0 and float(got["vertices"][:, 6].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ frame counts, determinism
def test_one_frame_and_601_frames_bit_exact_per_frame(dev, gold, fix):
    skel, sk = fix
    poses, scales = R.make_inputs(70, 601)
    want, allow = own_allowance(skel, poses, scales, template_verts=gold["template_verts"], global_scaling=gold["global_scaling"])
    tp, ts = torch.from_numpy(poses).to(dev), torch.from_numpy(scales).to(dev)
    run = lambda p: (sk.joint_states(p, ts), sk.transforms(p, ts), sk.pose_vertices(p, ts), sk.joint_positions(p, ts))
    full = run(tp)
    for k, got in zip(("states", "matrices", "vertices", "joints"), full):
        gate(f"skin_N601_{k}", got, want[k], allow[k])
    again = run(tp)
    assert all(torch.equal(a, b) for a, b in zip(full, again)), "two identical runs differ"
    for i in (0, 299, 600):
        alone = run(tp[i:i + 1])
        assert all(a.shape[0] == 1 and torch.equal(a[0], b[i]) for a, b in zip(alone, full)), f"frame {i} depends on the batch"
    tail = run(tp[590:])                                                      # another N and another index for the same poses
    assert all(torch.equal(a, b[590:]) for a, b in zip(tail, full))
    w1, a1 = own_allowance(skel, poses[:1], scales, template_verts=gold["template_verts"], global_scaling=gold["global_scaling"])
    for k, got in zip(("states", "matrices", "vertices", "joints"), run(tp[:1])):
        gate(f"skin_N1_{k}", got, w1[k], a1[k])


# ------------------------------------------------------------------------------------------------ argument forms
def test_unposed_scaling_and_scale_forms(dev, gold, fix):
    skel, _ = fix
    N, V = 9, 500
    poses, scales = R.make_inputs(80, N)
    rs = np.random.RandomState(81)
    per_frame_scales = (rs.randn(N, P_SCALE) * 0.2).astype(np.float32)
    vu = (rs.randn(V, 3) * 0.02).astype(np.float32)
    vun = (rs.randn(N, V, 3) * 0.02).astype(np.float32)
    template = gold["template_verts"]
    tp = torch.from_numpy(poses).to(dev)
    for gname, g in (("scalar", np.float32(10.0)), ("vec3", gold["global_scaling"])):
        sk = build(skel, template_verts=template, lbs_scale=scales[0], global_scaling=g)
        for sname, sc in (("shared", scales), ("perframe", per_frame_scales)):
            ts = torch.from_numpy(sc).to(dev)
            for uname, u in (("none", None), ("V3", vu), ("NV3", vun)):
                f32 = R.pose_vertices(skel, poses, sc, u, template, g, np.float32)
                want = R.pose_vertices(skel, poses, sc, u, template, g)
                got = sk.pose_vertices(tp, ts, None if u is None else torch.from_numpy(u).to(dev))
                gate(f"skin_forms_{gname}_{sname}_{uname}", got, want, 4 * R.nerr(f32, want))
        assert torch.equal(sk.pose_vertices(tp, None, torch.from_numpy(vu[None]).to(dev)),
                           sk.pose_vertices(tp, torch.from_numpy(scales).to(dev), torch.from_numpy(vu).to(dev)))   # [1, V, 3]; lbs_scale
        wantj = R.joint_positions(skel, poses, per_frame_scales, g)
        gate(f"skin_forms_{gname}_joints", sk.joint_positions(tp, torch.from_numpy(per_frame_scales).to(dev)), wantj,
             4 * R.nerr(R.joint_positions(skel, poses, per_frame_scales, g, np.float32), wantj))
    plain = build(skel)                                                       # no template: the rest vertices are skinned
    want = R.pose_vertices(skel, poses, scales)
    gate("skin_forms_rest", plain.pose_vertices(tp, torch.from_numpy(scales).to(dev)), want,
         4 * R.nerr(R.pose_vertices(skel, poses, scales, dtype=np.float32), want))
    with pytest.raises(S.A2PError, match="lbs_scale"):
        plain.pose_vertices(tp)
    with pytest.raises(S.A2PError, match="scales must be"):
        plain.joint_states(tp, torch.zeros(2, P_SCALE, device=dev))
    with pytest.raises(S.A2PError, match="verts_unposed must be"):
        sk.pose_vertices(tp, None, torch.zeros(2, V, 3, device=dev))
    with pytest.raises(S.A2PError, match=r"poses must be \[N, 104\]"):
        sk.joint_states(torch.zeros(3, 103, device=dev))


def test_a_nan_pose_stays_in_its_frame(dev, fix):
    skel, sk = fix
    poses, _ = R.make_inputs(90, 7)
    clean = torch.from_numpy(poses).to(dev)
    dirty = clean.clone()
    dirty[3, int(np.nonzero(skel["transform"][:, :P_POS])[1][0])] = float("nan")      # a parameter some joint reads
    for fn in (sk.joint_states, sk.transforms, sk.pose_vertices, sk.joint_positions):
        a, b = fn(clean), fn(dirty)
        keep = [0, 1, 2, 4, 5, 6]
        assert torch.equal(a[keep], b[keep]) and bool(torch.isfinite(a).all())
        assert not bool(torch.isfinite(b[3]).all())


def test_non_default_stream_matches(dev, fix):
    skel, sk = fix
    poses, _ = R.make_inputs(91, 33)
    tp = torch.from_numpy(poses).to(dev)
    want = (sk.joint_states(tp), sk.transforms(tp), sk.pose_vertices(tp))
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        got = (sk.joint_states(tp), sk.transforms(tp), sk.pose_vertices(tp))
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(want, got))


# ------------------------------------------------------------------------------------------------ pose_motion, command line
def test_pose_motion_layouts(dev, fix):
    skel, sk = fix
    pose = np.random.RandomState(92).randn(2, 5, P_POS) * 0.6                 # [B, T, 104] float64 like the generators' "pose"
    a = S.pose_motion(sk, pose)
    b = S.pose_motion(sk, torch.from_numpy(pose).permute(0, 2, 1)[:, :, None, :].to(dev))     # [B, 104, 1, T]
    c = S.pose_motion(sk, torch.from_numpy(pose.reshape(10, P_POS)).to(dev))
    assert a["joints"].shape == (2, 5, 40, 3) and a["vertices"].shape == (2, 5, 500, 3) and a["joints"].is_cuda
    assert torch.equal(a["joints"], b["joints"]) and torch.equal(a["vertices"], b["vertices"])
    assert c["joints"].shape == (10, 40, 3) and torch.equal(c["vertices"].reshape(2, 5, 500, 3), a["vertices"])
    j = S.pose_motion(sk, pose, vertices=False)
    assert set(j) == {"joints"} and torch.equal(j["joints"], a["joints"])
    flat = pose.reshape(10, P_POS).astype(np.float32)
    tp = torch.from_numpy(flat).to(dev)
    assert torch.equal(a["vertices"].reshape(10, 500, 3), sk.pose_vertices(tp))
    assert torch.equal(a["joints"].reshape(10, 40, 3), sk.joint_positions(tp))


def test_command_line_matches_the_direct_call(dev, gold, fix, tmp_path):
    skel, sk = fix
    model, cfg = R.as_model_dicts(skel)
    assets = {"lbs_model_json": model, "lbs_config_dict": cfg, "lbs_template_verts": torch.from_numpy(gold["template_verts"]),
              "lbs_scale": torch.from_numpy(gold["scales"][0]), "global_scaling": torch.from_numpy(gold["global_scaling"])}
    torch.save(assets, tmp_path / "static_assets.pt")
    motions = np.random.RandomState(93).randn(2, P_POS, 1, 5) * 0.6           # un-normalised results.npy motions, float64
    np.save(tmp_path / "results.npy", {"motions": motions, "lengths": np.array([5, 5])})
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    argv = ["--results", str(tmp_path / "results.npy"), "--assets", str(tmp_path / "static_assets.pt"), "--out"]
    r = subprocess.run([sys.executable, "-m", "audio2photoreal_amd.skinning"] + argv + [str(tmp_path / "geometry.npy")],
                       capture_output=True, text=True, env=env, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert S.main(argv + [str(tmp_path / "joints.npy"), "--joints-only"]) == 0            # the same entry point, in this process
    for name, vertices in (("geometry.npy", True), ("joints.npy", False)):
        geo = np.load(tmp_path / name, allow_pickle=True).item()
        want = S.pose_motion(sk, motions, vertices=vertices)
        assert set(geo) == set(want) == ({"joints", "vertices"} if vertices else {"joints"})
        for k in want:
            assert geo[k].dtype == np.float32 and np.array_equal(geo[k], want[k].cpu().numpy()), k
