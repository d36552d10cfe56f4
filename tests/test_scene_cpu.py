"""The multi-body scene render without a GPU: the float64 / float32 restatement (tests/scene_restatement.py) against itself and
against the single-body restatement, the fixture tests/golden/golden_scene_v1.npz regenerated from its stored cameras, the host side
of audio2photoreal_amd/scene.py (placement, the camera in a body's frame, every refusal that comes before GPU work,
conversation_inputs) and the argument refusals of a2p_scene_render, which all come before any launch."""
import ctypes
import os

import numpy as np
import pytest
import torch

import render_aa_restatement as A
import render_restatement as R
import scene_restatement as SC
from audio2photoreal_amd import _lib
from audio2photoreal_amd import scene as SN
from audio2photoreal_amd import surface as S
from audio2photoreal_amd._lib import A2PError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_scene_v1.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def fixture():
    return SC.fixture_bodies()


def tiny():
    """Two 12-vertex bodies of 4 faces each in front of a 10 x 14 camera, body 1 nearer and shifted."""
    rs = np.random.RandomState(3)
    tri = np.array([[-1.3, -1.1, 4], [1.4, -0.9, 4.2], [0.1, 1.3, 4.1], [-0.6, -0.5, 3.5], [0.7, -0.4, 3.6], [0.0, 0.6, 3.4],
                    [-1.0, 0.2, 3.8], [-0.2, 0.3, 3.9], [-0.6, 1.0, 3.7], [0.3, 0.1, 3.3], [1.1, 0.2, 3.2], [0.6, 0.9, 3.3]], np.float32)
    vi = np.arange(12).reshape(4, 3)
    body = {"vi": vi, "vt": rs.rand(12, 2).astype(np.float32), "vti": vi[::-1].copy(), "n_verts": 12}
    other = {"vi": vi[:, ::-1].copy(), "vt": rs.rand(9, 2).astype(np.float32), "vti": rs.randint(0, 9, (4, 3)), "n_verts": 12}
    verts = [tri[None] + rs.randn(2, 12, 3).astype(np.float32) * 0.01, tri[None] * np.float32(0.8) + rs.randn(2, 12, 3).astype(np.float32) * 0.01]
    K = np.array([[[12.0, 0.3, 7.0], [0, 12.5, 5.0], [0, 0, 1]]], np.float32)
    Rt = np.concatenate([np.eye(3), [[0.05], [-0.02], [0.1]]], 1)[None].astype(np.float32)
    tex = [rs.randn(1, 2, 5, 6).astype(np.float32), rs.randn(2, 2, 3, 4).astype(np.float32)]
    return [body, other], verts, tex, K, Rt


# ------------------------------------------------------------------------------------------------ the restatement against itself
@pytest.mark.parametrize("s", [1, 2, 3])
def test_one_body_without_placement_is_the_single_body_restatement(s):
    bodies, verts, tex, K, Rt = tiny()
    bg = np.random.RandomState(5).randn(1, 2, 10, 14).astype(np.float32)
    for dtype in (np.float64, np.float32):
        got = SC.render(bodies[:1], verts[:1], tex[:1], K, Rt, 10, 14, s, flips=[True], background=bg, dtype=dtype)
        want = A.render_antialiased(verts[0], bodies[0], K, Rt, 10, 14, s, tex[0], True, bg, dtype=dtype)
        assert got["image"].dtype == dtype and np.array_equal(got["image"], want["image"]) and np.array_equal(got["alpha"], want["alpha"])
        assert np.array_equal(got["count"], want["count"]) and np.array_equal(got["body_count"][:, 0], want["count"])
        depth = A.interpolate_antialiased(verts[0], bodies[0], K, Rt, 10, 14, s, verts[0], dtype=dtype)["depth"]
        assert np.array_equal(got["depth"], depth) and (want["count"] > 0).any() and (want["count"] == 0).any()


def test_placement_composes_with_moved_vertices_and_bodies_share_the_z_buffer():
    bodies, verts, tex, K, Rt = tiny()
    M = SC.placement(25.0, (0.2, -0.1, 0.3), (0.1, 1.0, 0.05), pivot=(0.0, 0.0, 3.5))
    Mn = np.stack([M, SC.placement(-10.0, (0.0, 0.1, 0.0), (0, 1, 0))])          # one per frame
    for place in (M, Mn):
        got = SC.render(bodies, verts, tex, K, Rt, 10, 14, 2, placements=[None, place], flips=[False, True])
        moved = SC.place(verts[1], place)
        assert moved.dtype == np.float64
        want = SC.render(bodies, [verts[0], moved], tex, K, Rt, 10, 14, 2, flips=[False, True])
        assert all(np.array_equal(got[k], want[k]) for k in got)
    R3, t = M[:, :3], M[:, 3]
    assert np.allclose(SC.place(verts[1], M), verts[1].astype(np.float64) @ R3.T + t, rtol=0, atol=1e-14)
    assert SC.place(verts[1], M, np.float32).dtype == np.float32 and SC.place(verts[1], None, np.float32).dtype == np.float32
    # both bodies win samples, the counts add up, and swapping the bodies swaps the planes and nothing else (no depth ties here)
    got = SC.render(bodies, verts, tex, K, Rt, 10, 14, 2, placements=[None, M])
    assert (got["body_count"][:, 0] > 0).any() and (got["body_count"][:, 1] > 0).any()
    assert np.array_equal(got["body_count"].sum(1), got["count"])
    swapped = SC.render(bodies[::-1], verts[::-1], tex[::-1], K, Rt, 10, 14, 2, placements=[M, None])
    assert np.array_equal(swapped["image"], got["image"]) and np.array_equal(swapped["depth"], got["depth"])
    assert np.array_equal(swapped["body_count"], got["body_count"][:, ::-1])
    # the tie rule: two copies of a body at the same place -- the earlier body keeps every sample
    tie = SC.render([bodies[0], bodies[0]], [verts[0], verts[0]], [tex[0], tex[0]], K, Rt, 10, 14, 2)
    assert (tie["body_count"][:, 1] == 0).all() and (tie["body_count"][:, 0] > 0).any()
    m = SC.merged_mesh(bodies)
    assert np.array_equal(m["vi"][4:], bodies[1]["vi"] + 12) and list(m["f0"]) == [0, 4, 8] and list(m["v0"]) == [0, 12, 24]
    assert list(SC.body_of(np.array([-1, 0, 3, 4, 7]), m["f0"])) == [-1, 0, 0, 1, 1]


# ------------------------------------------------------------------------------------------------ the fixture
def test_fixture_is_what_its_generator_states(gold, fixture):
    bodies, verts = fixture
    assert [b["n_verts"] for b in bodies] == [874, 437] and verts[0].shape == (3, 874, 3) and verts[1].shape == (3, 437, 3)
    assert np.array_equal(gold["frames"], np.asarray(SC.FRAMES)) and int(gold["clearance_factor"]) == SC.CLEARANCE_FACTOR == 8
    assert sorted(s for _, s, _, _ in SC.FRAMES) == [1, 2, 3, 4, 4]
    factor = SC.CLEARANCE_FACTOR
    assert gold["edge_clearance"].min() > factor * gold["e_proj"].max() and gold["depth_clearance"].min() > factor * gold["e_depth"].max()
    for k, (kind, s, H, W) in enumerate(SC.FRAMES):
        M = gold[f"M{k}"]
        assert M.dtype == np.float32 and M.shape == (3, 4)
        SN.check_rigid(M)
        assert gold[f"tex{k}_0"].shape == (3,) + SC.TEX_SIZES[0] and gold[f"tex{k}_1"].shape == (3,) + SC.TEX_SIZES[1]
        assert SC.TEX_SIZES[0] != SC.TEX_SIZES[1] and gold[f"bg{k}"].shape == (3, H, W)
        c = SC.clearances(bodies, [v[kind:kind + 1] for v in verts], [None, M], gold[f"K{k}"][None], gold[f"Rt{k}"][None], H, W, s)
        assert c["same_faces"] and np.array_equal(c["f64"]["face"][0], gold[f"face{k}"])
        for name in ("e_proj", "edge_clearance", "e_depth", "depth_clearance"):
            assert c[name] == gold[name][k], (k, name)
        count = A.block_count(c["f64"]["face"] >= 0, s)
        partly, both = int(((count > 0) & (count < s * s)).sum()), int(SC.both_bodies(c["f64"], s).sum())
        assert (partly, both, int((c["f64"]["body"] == 1).sum())) == (int(gold["partly"][k]), int(gold["both"][k]), int(gold["covered1"][k]))
        assert gold["covered1"][k] > 0 and gold["covered"][k] > gold["covered1"][k]          # both bodies are seen
        if s > 1:
            assert partly >= SC.MIN_PARTLY == 20 and both >= SC.MIN_BOTH == 20


# ------------------------------------------------------------------------------------------------ scene.py on the host
def test_placement_is_rodrigues_in_float64():
    for yaw, pos, up, pivot in ((35.0, (0.05, 0.03, -0.22), (0, 1, 0), (1.1, 0.9, 0.0)), (-120.5, (1, 2, 3), (0.3, -2.0, 0.4), (0, 0, 0)),
                                (0.0, (0, 0, 0), (0, 0, 1), (5, 6, 7)), (360.0 + 17, (0.1, 0, 0), (1, 1, 1), (-1, 0.5, 2))):
        got = SN.placement(yaw, pos, up, pivot)
        assert torch.is_tensor(got) and got.dtype == torch.float32 and tuple(got.shape) == (3, 4) and got.device.type == "cpu"
        want = SC.placement(yaw, pos, up, pivot)
        assert np.array_equal(got.numpy(), want.astype(np.float32))            # float64 on the host, rounded once
        Rm = want[:, :3]
        axis = np.asarray(up, np.float64) / np.linalg.norm(up)
        assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-14) and np.isclose(np.linalg.det(Rm), 1.0) and np.allclose(Rm @ axis, axis, atol=1e-14)
        assert np.allclose(Rm @ np.asarray(pivot, np.float64) + want[:, 3], np.asarray(pivot, np.float64) + np.asarray(pos, np.float64), atol=1e-13)
        assert np.isclose(np.trace(Rm), 1 + 2 * np.cos(np.radians(yaw)))
        SN.check_rigid(got)
    assert np.array_equal(SN.placement(0.0, (0, 0, 0), (0, 1, 0)).numpy(), np.eye(3, 4, dtype=np.float32))
    quarter = SN.placement(90.0, (0, 0, 0), (0, 1, 0)).numpy().astype(np.float64)
    assert np.allclose(quarter[:, :3] @ [0, 0, 1], [1, 0, 0], atol=1e-7)       # counter-clockwise about up, seen from its tip
    for bad, match in ((dict(up=(0, 0, 0)), "no direction"), (dict(up=(0, 1)), "3 finite numbers"), (dict(position=(0, np.nan, 0)), "3 finite numbers"),
                       (dict(yaw_degrees=float("inf")), "not finite")):
        kw = {"yaw_degrees": 10.0, "position": (0, 0, 0), "up": (0, 1, 0), **bad}
        with pytest.raises(ValueError, match=match):
            SN.placement(**kw)


def test_camera_in_the_bodys_frame():
    rs = np.random.RandomState(8)
    M = SC.placement(40.0, (0.5, -0.2, 1.0), (0.2, 1.0, -0.1), (0.3, 0.1, 0.2))
    cams = rs.randn(3, 3)
    want = SC.camera_in_body_frame(cams, M)
    assert np.allclose(want @ M[:, :3].T + M[:, 3], cams, atol=1e-13)           # placing the body-frame camera gives the world camera back
    assert np.array_equal(SC.camera_in_body_frame(cams, None), cams)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    got = SN.camera_in_body_frame(t(cams[:1]), t(M))
    assert tuple(got.shape) == (1, 3) and np.allclose(got.numpy(), want[:1], atol=1e-6)
    Mn = np.stack([M, SC.placement(-15.0, (0, 0, 2), (0, 1, 0))])
    per = SN.camera_in_body_frame(t(cams[:1]), t(Mn))
    assert tuple(per.shape) == (2, 3) and np.allclose(per.numpy(), np.stack([SC.camera_in_body_frame(cams[0], m) for m in Mn]), atol=1e-6)
    # the view the texture gets: the direction from the camera to a vertex, in body coordinates, is the world direction turned back
    x = rs.randn(3)
    world = M[:, :3] @ x + M[:, 3]
    assert np.allclose(M[:, :3].T @ (world - cams[0]), x - want[0], atol=1e-13)


def surfaces():
    surf = R.make_surface()
    two = R.two_layers(surf)
    a = S.BodySurface.from_arrays(two["vi"], two["vt"], two["vti"], n_verts=two["n_verts"], v2uv=np.zeros((two["n_verts"], 4), np.int64), uv_size=8)
    return surf, two, a


def test_scene_rasterizer_construction_and_refusals():
    surf, two, a = surfaces()
    arrays = (surf["vi"], surf["vt"], surf["vti"], surf["n_verts"])
    from audio2photoreal_amd.render import BodyRasterizer
    rz = BodyRasterizer(arrays, 7, 9, flip_uv=True)
    sc = SN.SceneRasterizer([a, (arrays, True), rz, {"body": arrays[:3]}], 24, 32)
    assert (sc.P, sc.V, sc.F, sc.sum_V, sc.sum_F) == (4, [874, 437, 437, 437], [1584, 792, 792, 792], 2185, 3960)
    assert [b.flip_uv for b in sc.bodies] == [False, True, True, False] and all((b.height, b.width) == (24, 32) for b in sc.bodies)
    assert sc.bodies[0].surface is a and sc.bodies[2]._vi is rz._vi and (rz.height, rz.width) == (7, 9)      # shared tables, the given object untouched
    want = SC.merged_mesh([two, surf, surf, surf])
    assert sc.faces.dtype == np.int32 and np.array_equal(sc.faces, want["vi"]) and sc.scratch_bytes_per_frame(3) == 12 * 2185 + 8 * 9 * 24 * 32
    assert not SN.SceneRasterizer([(rz, False)], 4, 4).bodies[0].flip_uv
    for bodies, err, match in (([], ValueError, "1 to 4 bodies"), ([a] * 5, ValueError, "1 to 4 bodies"), (a, TypeError, "sequence of bodies"),
                               ([a, "mesh"], TypeError, r"bodies\[1\] must be a BodySurface"), ([{"surface": a}], TypeError, "holds `body`"),
                               ([(surf["vi"], surf["vt"], surf["vti"][:5])], ValueError, "need the same F"),
                               ([(surf["vi"], surf["vt"], surf["vti"] + 10 ** 6)], ValueError, "is outside")):
        with pytest.raises(err, match=match):
            SN.SceneRasterizer(bodies, 24, 32)
    for kw, match in ((dict(height=0), "height=0"), (dict(width=_lib.RENDER_MAX_SIZE + 1), "width="), (dict(near=0.0), "near=")):
        with pytest.raises(ValueError, match=match):
            SN.SceneRasterizer([a], **{"height": 4, "width": 4, **kw})


def test_render_refuses_malformed_input_before_gpu_work():
    surf, two, a = surfaces()
    sc = SN.SceneRasterizer([a, (surf["vi"], surf["vt"], surf["vti"], surf["n_verts"])], 6, 8)
    v = [torch.zeros(2, 874, 3), torch.zeros(2, 437, 3)]
    tex = [torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 5, 6)]
    K, Rt = torch.eye(3), torch.eye(3, 4)
    for kw, err, match in ((dict(supersample=0), ValueError, "supersample=0"), (dict(supersample=5), ValueError, "supersample=5"),
                           (dict(supersample=2.5), ValueError, "supersample=2.5"), (dict(max_bytes=0), A2PError, "max_bytes=0"),
                           (dict(verts=v[:1]), A2PError, "verts must be a sequence of 2 entries"), (dict(verts=v[0]), A2PError, "got Tensor"),
                           (dict(textures=tex + tex), A2PError, "textures must be a sequence of 2 entries"),
                           (dict(placements=[None]), A2PError, "placements must be a sequence of 2 entries"),
                           (dict(verts=[v[0].numpy(), v[1]]), A2PError, r"verts\[0\] must be a tensor on the MI355X \(got ndarray\)"),
                           (dict(), A2PError, r"verts\[0\] must live on the MI355X \(got device cpu\)")):
        args = {"verts": v, "textures": tex, "K": K, "Rt": Rt, **kw}
        with pytest.raises(err, match=match):
            sc.render(**args)


def test_conversation_refusals_come_before_any_gpu_work():
    av = SN.Avatar(*[None] * 7)
    poses, codes = [np.zeros((3, 104), np.float32)] * 2, [np.zeros((3, 256), np.float32)] * 2
    K, Rt = np.eye(3)[None], np.eye(3, 4)[None]
    good = SN.placement(20.0, (1, 0, 0), (0, 1, 0)).numpy()
    shear = good.copy()
    shear[0, 1] += 0.01
    mirror = good.copy()
    mirror[:, 0] *= -1
    scaled = good.copy()
    scaled[:, :3] *= 1.001
    call = lambda **kw: SN.render_conversation_motion(**{"avatars": [av, av], "poses": poses, "face_codes": codes, "placements": [None, good], "K": K,
                                                         "Rt": Rt, "height": 8, "width": 8, **kw})
    for kw, err, match in ((dict(avatars=[av]), A2PError, "poses must be a sequence of 1 entries"), (dict(avatars=[av] * 5), A2PError, "1 to 4 Avatar"),
                           (dict(avatars=[av, (None,) * 7]), A2PError, "1 to 4 Avatar"), (dict(placements=[good]), A2PError, "placements must be a sequence of 2"),
                           (dict(face_codes=codes[:1]), A2PError, "face_codes must be a sequence of 2"),
                           (dict(face_codes=[codes[0], codes[1][:2]]), A2PError, "share their frames"),
                           (dict(placements=[None, shear]), ValueError, r"placements\[1\] is not rigid"),
                           (dict(placements=[mirror, None]), ValueError, r"placements\[0\] is not rigid"),
                           (dict(placements=[None, scaled]), ValueError, "not rigid"), (dict(placements=[None, good[:, :3]]), ValueError, r"\[3, 4\]"),
                           (dict(placements=[None, good * np.nan]), ValueError, "not finite"), (dict(placements=[None, "left"]), ValueError, "must be None or an array"),
                           (dict(body_embs="mean"), A2PError, "body_embs='mean'"), (dict(background=[1.0, 2.0]), ValueError, "three numbers")):
        with pytest.raises(err, match=match):
            call(**kw)
    video = lambda **kw: SN.render_conversation_video(**{"avatars": [av, av], "poses": poses, "face_codes": codes, "placements": [None, good], "K": K,
                                                         "Rt": Rt, "height": 8, "width": 8, "path": os.devnull, **kw})
    for kw, err, match in ((dict(poses=[poses[0], poses[1][:2]]), A2PError, "one T"), (dict(poses=[p[None] for p in poses]), A2PError, "one T"),
                           (dict(placements=[None, shear]), ValueError, "not rigid"), (dict(placements=[None, np.stack([good] * 2)]), A2PError, r"\[3 or 1, 3, 4\]")):
        with pytest.raises(err, match=match):
            video(**kw)
    assert SN.check_rigid(np.stack([good, good])).shape == (2, 3, 4) and SN.check_rigid(torch.from_numpy(good)).dtype == np.float64


def test_conversation_inputs():
    rs = np.random.RandomState(2)
    person = lambda: {"pose": rs.randn(2, 5, 104), "face": rs.randn(2, 5, 256), "keyframes": rs.randn(2, 1, 104), "audio": rs.randn(2, 8000), "T": 5, "sr": 48000}
    result = {"people": [person(), person()], "T": 5, "sr": 48000}
    poses, codes, audio = SN.conversation_inputs(result, repetition=1)
    assert len(poses) == len(codes) == 2 and audio.shape == (8000, 2) and audio.dtype == np.float64
    for p in range(2):
        assert np.array_equal(poses[p], result["people"][p]["pose"][1]) and np.array_equal(codes[p], result["people"][p]["face"][1])
        assert np.array_equal(audio[:, p], result["people"][p]["audio"][0])    # every person's own microphone
    assert np.array_equal(SN.conversation_inputs(result)[0][0], result["people"][0]["pose"][0])
    for bad, match in (({"people": [person(), None]}, r"people\[1\] is None"), ({"pose": 1}, "generate_conversation returns"), ([], "generate_conversation returns"),
                       ({"people": [{k: v for k, v in person().items() if k != "face"}]}, "holds no `face`")):
        with pytest.raises(A2PError, match=match):
            SN.conversation_inputs(bad)
    with pytest.raises(A2PError, match="repetition=2"):
        SN.conversation_inputs(result, repetition=2)
    short = person()
    short["audio"] = short["audio"][:, :100]
    with pytest.raises(A2PError, match="same number of frames and samples"):
        SN.conversation_inputs({"people": [person(), short]})


def test_command_line_refusals():
    with pytest.raises(A2PError, match="one file per person"):
        SN.main(["--results", "a.npy", "b.npy", "--assets", "a.pt", "--checkpoint", "a.ckpt", "b.ckpt", "--out", "x.npy"])
    with pytest.raises(A2PError, match="--yaw takes 2 numbers"):
        SN.main(["--results", "a.npy", "b.npy", "--assets", "a.pt", "b.pt", "--checkpoint", "a.ckpt", "b.ckpt", "--out", "x.npy", "--yaw", "3"])
    with pytest.raises(A2PError, match="--audio goes with --video"):
        SN.main(["--results", "a.npy", "--assets", "a.pt", "--checkpoint", "a.ckpt", "--out", "x.npy", "--audio", "a.wav"])


# ------------------------------------------------------------------------------------------------ the C ABI
def test_abi_refuses_bad_arguments_before_any_launch():
    """Every pointer is a made-up address: a refusal must come before anything is launched or read on the device."""
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.load()
    assert _lib.SCENE_MAX_BODIES == 4 and "a2p_scene_render" in _lib.EXPORTS and hasattr(lib, "a2p_scene_render")
    assert ctypes.sizeof(_lib.A2PSceneBody) == 5 * 8 + 8 * 4
    at = lambda k: 0x10000 * (k + 1)

    def bodies(P=2, **kw):
        arr = (_lib.A2PSceneBody * max(P, 1))()
        for p in range(max(P, 1)):
            arr[p] = _lib.A2PSceneBody(at(10 + 5 * p), None, at(11 + 5 * p), at(12 + 5 * p), at(13 + 5 * p), 12, 4, 12, 6, 7, 0, 0, 0)
            for name, value in kw.items():
                setattr(arr[p], name, value)
        return arr

    def call(b=None, P=2, faces=at(0), N=2, K=at(1), Rt=at(2), H=24, W=40, S=2, near=1e-3, C=3, bg=at(3), proj=at(4), key=at(5), out=at(6), alpha=at(7),
             depth=at(8), body_alpha=at(9)):
        return lib.a2p_scene_render(bodies(P) if b is None else b, P, faces, N, K, 0, Rt, 0, H, W, S, near, C, bg, 1, proj, key, out, alpha, depth,
                                    body_alpha, None)

    big = 0x7fffffff // 3 // 2 + 1
    cases = ((dict(faces=None), "null argument"), (dict(out=None), "null argument"), (dict(depth=None), "null argument"), (dict(body_alpha=None), "null argument"),
             (dict(b=bodies(verts=None)), "body 0: null argument"), (dict(b=bodies(vti=None)), "body 0: null argument"),
             (dict(P=0), "need 1 <= P <= 4"), (dict(P=5, b=bodies(5)), "need 1 <= P <= 4"), (dict(S=0), "need 1 <= S <= 4"), (dict(S=5), "need 1 <= S <= 4"),
             (dict(H=0), "need 1 <= H, W"), (dict(S=4, W=_lib.RENDER_MAX_SIZE // 4 + 1), "S H, S W <= 8192"), (dict(near=0.0), "positive finite"),
             (dict(C=0), r"C=0 outside \[1, 16\]"), (dict(C=17), r"C=17 outside \[1, 16\]"), (dict(N=-1), "exceed the grid"),
             (dict(b=bodies(V=0)), "need V, F, T >= 1"), (dict(b=bodies(F=0)), "need V, F, T >= 1"), (dict(b=bodies(T=0)), "need V, F, T >= 1"),
             (dict(b=bodies(Ht=0)), "body 0: a 0 x 7 texture"), (dict(b=bodies(Ht=1 << 16, Wt=1 << 16)), "need 1 <= Ht Wt < 2"),
             (dict(b=bodies(F=big)), "3 sum V, 3 sum F < 2"), (dict(b=bodies(V=big)), "3 sum V, 3 sum F < 2"),
             (dict(N=1 << 30, H=64, W=64), "exceed the grid"), (dict(N=0x7fffffff), "exceed the grid"),
             (dict(out=at(11)), "must not alias an input"), (dict(proj=at(0)), "must not alias an input"), (dict(key=at(3)), "must not alias an input"),
             (dict(body_alpha=at(18)), "must not alias an input"), (dict(depth=at(7)), "must be distinct"), (dict(body_alpha=at(4)), "must be distinct"))
    for kw, match in cases:
        rc = call(**kw)
        assert rc == -1, (kw, rc)                                              # A2P_ERR_ARG
        with pytest.raises(A2PError, match=match):
            _lib.check(rc, "a2p_scene_render")
    placed = bodies(placement=at(30))
    assert call(b=placed, out=at(30)) == -1
    with pytest.raises(A2PError, match="must not alias an input"):
        _lib.check(-1, "a2p_scene_render")
    assert call(N=0) == 0 and call(N=0, P=1) == 0 and call(N=0, bg=None) == 0 and call(N=0, out=None) == -1     # N = 0: checked, nothing launched
