"""Host side of the rendered images (audio2photoreal_amd/render.py), no GPU: the restatement (tests/render_restatement.py) against
hand-computed cases, the stored fixture's clearances (tests/golden/golden_render_v1.npz), every rejection of the constructors, of
look_at and of the command line, and the refusal to compute anything on the CPU."""
import os

import numpy as np
import pytest
import torch

import render_restatement as R
from audio2photoreal_amd import _lib
from audio2photoreal_amd import render as RD
from audio2photoreal_amd import surface as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)[None]                  # Rt of a camera at the origin looking along +z
K8 = np.array([[[4.0, 0, 4], [0, 4, 4], [0, 0, 1]]])                          # an 8 x 8 image, 90 degrees across


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_render_v1.npz"))


# ------------------------------------------------------------------------------------------------ the restatement
def test_one_triangle_by_hand():
    """(-2, -2, 2), (2, -2, 2), (-2, 2, 2) project to (0, 0), (8, 0), (0, 8): the centres (j + 0.5, i + 0.5) with i + j <= 7 are
    covered, those with i + j = 7 lying exactly on the long edge; depth 2; barycentrics (1 - (x + y) / 8, x / 8, y / 8)."""
    verts = np.array([[[-2.0, -2, 2], [2, -2, 2], [-2, 2, 2]]])
    vi = np.array([[0, 1, 2]])
    i, j = np.meshgrid(np.arange(8), np.arange(8), indexing="ij")
    want = i + j <= 7
    sb = np.stack([1 - (i + j + 1) / 8, (j + 0.5) / 8, (i + 0.5) / 8], -1)
    for dtype in (np.float64, np.float32):
        for faces in (vi, vi[:, ::-1]):                                       # both windings
            got = R.rasterize(verts, faces, K8, EYE, 8, 8, dtype=dtype)
            assert np.array_equal(got["face"][0] >= 0, want) and want.sum() == 36
            assert np.array_equal(got["depth"][0], np.where(want, 2.0, 0.0))
            order = [0, 1, 2] if faces is vi else [2, 1, 0]
            assert np.allclose(got["bary"][0][want], sb[want][:, order], atol=1e-6) and np.all(got["bary"][0][~want] == 0)
    assert np.array_equal(R.project(verts, K8, EYE)[0], [[0, 0, 2], [8, 0, 2], [0, 8, 2]])
    skew = K8.copy()
    skew[0, 0, 1] = 2.0                                                       # u gains 2 (y / z)
    assert np.array_equal(R.project(verts, skew, EYE)[0], [[-2, 0, 2], [6, 0, 2], [2, 8, 2]])
    # a zero-area face covers nothing; a corner nearer than `near` drops the face whole; the nearer of two faces wins
    flat = np.array([[[-2.0, -2, 2], [0, 0, 2], [2, 2, 2]]])
    assert (R.rasterize(flat, vi, K8, EYE, 8, 8)["face"] == -1).all()
    assert (R.rasterize(verts, vi, K8, EYE, 8, 8, near=2.5)["face"] == -1).all()
    both = np.concatenate([verts, verts * 0.5], 1)                            # the same screen triangle at depth 1, listed second
    got = R.rasterize(both, np.array([[0, 1, 2], [3, 4, 5]]), K8, EYE, 8, 8, runner_up=True)
    assert np.array_equal(got["face"][0], np.where(want, 1, -1)) and np.array_equal(got["second"][0][want], np.full(36, 2.0))
    assert R.depth_clearance(got) == 1.0
    tie = R.rasterize(np.concatenate([verts, verts], 1), np.array([[3, 4, 5], [0, 1, 2]]), K8, EYE, 8, 8)
    assert np.array_equal(tie["face"][0], np.where(want, 0, -1))              # equal depth: the lowest index
    # the long edge passes through centres (distance 0); the other two edges are half a pixel from the nearest centres
    assert R.edge_clearance(verts, vi, K8, EYE, 8, 8) == 0.0
    small = np.array([[[-2.0, -2, 2], [1.9, -2, 2], [-2, 1.9, 2]]])           # u + v = 7.8: nearest centres 0.2 / sqrt 2 away
    assert R.edge_clearance(small, vi, K8, EYE, 8, 8) == pytest.approx(0.2 / np.sqrt(2), rel=1e-9)


def test_perspective_correction_by_the_closed_form():
    """The same screen triangle with depths (2, 4, 4): with s the screen-space weight of the near corner, its corrected weight is
    2 s / (1 + s), so the correction is s (1 - s) / (1 + s), and the depth is 4 / (1 + s)."""
    verts = np.array([[[-2.0, -2, 2], [4, -4, 4], [-4, 4, 4]]])
    vi = np.array([[0, 1, 2]])
    got = R.rasterize(verts, vi, K8, EYE, 8, 8)
    hit = got["face"][0] >= 0
    i, j = np.nonzero(hit)
    assert hit.sum() == 36
    screen = R.screen_barycentrics(verts, vi, K8, EYE, got["face"], 8, 8)[0][hit]
    s = 1 - (i + j + 1) / 8
    assert np.allclose(screen, np.stack([s, (j + 0.5) / 8, (i + 0.5) / 8], -1), atol=1e-12)
    bary = got["bary"][0][hit]
    assert np.allclose(bary[:, 0] - screen[:, 0], s * (1 - s) / (1 + s), atol=1e-12)
    assert np.abs(bary[:, 0] - screen[:, 0]).max() > 0.15                     # a real correction, not a rounding
    assert np.allclose(bary.sum(1), 1, atol=1e-12) and np.allclose(got["depth"][0][hit], 4 / (1 + s), atol=1e-12)
    # interpolating the camera-space z of the corners with the corrected weights gives the depth back
    z = R.interpolate(verts[:, :, 2:], vi, got["face"], got["bary"])
    assert np.allclose(z[0, 0][hit], got["depth"][0][hit], atol=1e-12) and np.all(z[0, 0][~hit] == 0)


def test_texture_sampling_by_hand():
    """uv = (0, 0), (1, 0), (0, 1) at the corners of the hand triangle: pixel (i, j) samples x = (j + 0.5) / 8 (Wt - 1), y = (i +
    0.5) / 8 (Ht - 1) of the texture as given; flip_uv samples row Ht - 1 - y."""
    verts = np.array([[[-2.0, -2, 2], [2, -2, 2], [-2, 2, 2]]])
    vi = np.array([[0, 1, 2]])
    vt = np.array([[0.0, 0], [1, 0], [0, 1]])
    frag = R.rasterize(verts, vi, K8, EYE, 8, 8)
    yy, xx = np.meshgrid(np.arange(5.0), np.arange(9.0), indexing="ij")
    tex = np.stack([xx, yy, 10 * yy + xx])[None]                              # linear in x and y: bilinear sampling is exact
    i, j = np.nonzero(frag["face"][0] >= 0)
    for flip in (False, True):
        got = R.sample_texture(tex, vt, vi, frag["face"], frag["bary"], flip_uv=flip)
        x, y = (j + 0.5) / 8 * 8, (i + 0.5) / 8 * 4
        y = 4 - y if flip else y
        assert got.shape == (1, 3, 8, 8) and np.allclose(got[0][:, i, j], [x, y, 10 * y + x], atol=1e-12)
        assert np.all(got[0][:, frag["face"][0] < 0] == 0)
    # uv beyond [0, 1] clamps to the border texel
    far = R.sample_texture(tex, vt * 3 - 1, vi, frag["face"], frag["bary"])
    assert far.min() >= 0 and far[0, 0].max() == 8 and far[0, 1].max() == 4


def test_look_at_is_a_rotation_with_a_centred_target():
    rs = np.random.RandomState(2)
    for _ in range(5):
        eye, target, up = rs.randn(3) * 3, rs.randn(3), rs.randn(3)
        K, Rt = R.look_at(eye, target, up, 48, 64, 35.0)
        Rm = Rt[:, :3]
        assert np.allclose(Rm @ Rm.T, np.eye(3), atol=1e-12) and np.linalg.det(Rm) == pytest.approx(1.0)
        assert np.allclose(Rm @ eye + Rt[:, 3], 0, atol=1e-12)                # the eye is the camera centre
        p = R.project(np.stack([target, target + 0.1 * up])[None], K[None], Rt[None])[0]
        assert np.allclose(p[0], [32, 24, np.linalg.norm(target - eye)], atol=1e-9)
        assert p[1, 1] < 24 and p[1, 0] == pytest.approx(32, abs=1e-9)        # `up` points up in the image: y runs down
        assert K[0, 0] == K[1, 1] == pytest.approx(24 / np.tan(np.radians(17.5)))
        Kp, Rtp = RD.look_at(eye, target, up, 48, 64, 35.0)                   # the product's own, float32 tensors
        assert Kp.dtype == Rtp.dtype == torch.float32 and Kp.shape == (3, 3) and Rtp.shape == (3, 4)
        assert np.array_equal(Kp.numpy(), K.astype(np.float32)) and np.array_equal(Rtp.numpy(), Rt.astype(np.float32))
    x_right = R.look_at([0, 0, 5], [0, 0, 0], [0, 1, 0], 8, 8, 90)[1]
    assert np.allclose(x_right, [[1, 0, 0, 0], [0, -1, 0, 0], [0, 0, -1, 5]], atol=1e-12)


# ------------------------------------------------------------------------------------------------ the fixture
def test_the_fixture_scene_is_what_the_builder_makes(gold):
    surf = R.make_surface()
    mesh = R.two_layers(surf)
    for k in ("vi", "vt", "vti"):
        assert np.array_equal(mesh[k], gold[k]), k
    assert np.array_equal(R.layered_frames(surf, 5, 3), gold["verts"])
    assert gold["verts"].shape == (3, 874, 3) and gold["vi"].shape == (1584, 3) and gold["tex"].shape == (3, 3, 40, 56)
    assert [tuple(s) for s in gold["sizes"]] == list(R.SIZES) and int(gold["clearance_factor"]) == R.CLEARANCE_FACTOR
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_render_v1.npz")) < 1 << 20


def test_the_stored_clearances_are_reproduced(gold):
    """Each frame keeps every pixel centre clear of every edge, and every winner clear of its runner-up, by more than the stated
    multiple of the LARGEST float32 error of the fixture -- with no pixel excluded: float32 and float64 give the same faces."""
    factor = int(gold["clearance_factor"])
    vi = gold["vi"].astype(np.int64)
    for k, (H, W) in enumerate(R.SIZES):
        v, K, Rt = gold["verts"][k:k + 1], gold["K"][k:k + 1], gold["Rt"][k:k + 1]
        p64, p32 = R.project(v, K, Rt), R.project(v, K, Rt, np.float32)
        e_proj = float(np.abs(p32[..., :2].astype(np.float64) - p64[..., :2]).max())
        assert e_proj == pytest.approx(float(gold["e_proj"][k]), rel=1e-9)
        edge = R.edge_clearance(v, vi, K, Rt, H, W)
        assert edge == pytest.approx(float(gold["edge_clearance"][k]), rel=1e-9) and edge > factor * gold["e_proj"].max()
        f64 = R.rasterize(v, vi, K, Rt, H, W, runner_up=True)
        f32 = R.rasterize(v, vi, K, Rt, H, W, dtype=np.float32)
        assert np.array_equal(f64["face"][0], gold[f"face{k}"]) and np.array_equal(f32["face"], f64["face"])
        hit = f64["face"] >= 0
        e_depth = float((np.abs(f32["depth"][hit].astype(np.float64) - f64["depth"][hit]) / f64["depth"][hit]).max())
        assert e_depth == pytest.approx(float(gold["e_depth"][k]), rel=1e-9)
        gap = R.depth_clearance(f64)
        assert gap == pytest.approx(float(gold["depth_clearance"][k]), rel=1e-9) and gap > factor * gold["e_depth"].max()
        twice = np.isfinite(f64["second"]) & hit
        assert int(hit.sum()) == int(gold["covered"][k]) and int(twice.sum()) == int(gold["twice"][k])
        assert hit.mean() > 0.3 and twice.sum() > 0.5 * hit.sum()             # most covered pixels see both layers
        front = f64["face"][twice] < 792                                      # ... and the front layer is not always the winner's
        assert front.any()


# ------------------------------------------------------------------------------------------------ host validation
def test_every_rejection_of_the_constructors(gold):
    vi, vt, vti = gold["vi"].astype(np.int64), gold["vt"], gold["vti"].astype(np.int64)
    build = RD.BodyRasterizer.from_arrays
    ok = build(vi, vt, vti, 48, 64)
    assert (ok.V, ok.F, ok.T, ok.height, ok.width, ok.near, ok.flip_uv) == (874, 1584, len(vt), 48, 64, 1e-3, False)
    assert build(vi[:1], vt, vti[:1], 4, 4, n_verts=900).V == 900             # unused vertices are fine here
    for name, h, w in (("height", 0, 8), ("height", _lib.RENDER_MAX_SIZE + 1, 8), ("width", 8, 0), ("width", 8, -2)):
        with pytest.raises(ValueError, match=f"{name}={h if name == 'height' else w} is outside"):
            build(vi, vt, vti, h, w)
    for near in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="must be a positive finite distance"):
            build(vi, vt, vti, 8, 8, near=near)
    bad = vi.copy()
    bad[7, 2] = 874
    with pytest.raises(ValueError, match=r"vi\[7, 2\] = 874 is outside \[0, V=874\)"):
        build(bad, vt, vti, 8, 8, n_verts=874)
    bad = vti.copy()
    bad[3, 1] = -1
    with pytest.raises(ValueError, match=r"vti\[3, 1\] = -1 is outside"):
        build(vi, vt, bad, 8, 8)
    with pytest.raises(ValueError, match="F=1584 faces and vti 1583"):
        build(vi, vt, vti[:-1], 8, 8)
    with pytest.raises(ValueError, match=r"vt must be \[T >= 1, 2\]"):
        build(vi, vt[:, :1], vti, 8, 8)
    nan = vt.copy()
    nan[9, 1] = np.nan
    with pytest.raises(ValueError, match=r"vt\[9, 1\] is not finite"):
        build(vi, nan, vti, 8, 8)
    with pytest.raises(TypeError, match="a BodySurface or a tuple"):
        RD.BodyRasterizer(5, 8, 8)
    # from a BodySurface, and from the mapping the reference reads
    sf = S.BodySurface.from_arrays(vi, vt, vti, uv_size=16)
    shared = RD.BodyRasterizer(sf, 37, 53, flip_uv=True, near=0.5)
    assert shared.surface is sf and (shared.V, shared.F, shared.T, shared.flip_uv, shared.near) == (874, 1584, len(vt), True, 0.5)
    topo = {"vi": torch.from_numpy(vi), "vt": torch.from_numpy(vt), "vti": torch.from_numpy(vti), "v2uv": torch.from_numpy(sf.v2uv)}
    assert RD.BodyRasterizer.from_static_assets({"topology": topo}, 8, 9).width == 9


def test_look_at_rejections():
    ok = ([0, 0, 5], [0, 0, 0], [0, 1, 0], 8, 8, 40.0)
    RD.look_at(*ok)
    cases = {"coincide": ([0, 0, 0], [0, 0, 0], [0, 1, 0], 8, 8, 40.0), "parallel to the viewing direction": ([0, 5, 0], [0, 0, 0], [0, 2, 0], 8, 8, 40.0),
             "outside \\(0, 180\\)": ok[:5] + (180.0,), "need height, width >= 1": ok[:3] + (0, 8, 40.0),
             "3 finite numbers": ([0, 0, np.nan],) + ok[1:]}
    for match, args in cases.items():
        with pytest.raises(ValueError, match=match):
            RD.look_at(*args)
    with pytest.raises(ValueError, match="outside"):
        RD.look_at(*ok[:5], 0.0)


def test_nothing_is_computed_on_the_cpu(gold):
    vi, vt, vti = gold["vi"].astype(np.int64), gold["vt"], gold["vti"].astype(np.int64)
    rast = RD.BodyRasterizer.from_arrays(vi, vt, vti, 8, 8)
    sf = S.BodySurface.from_arrays(vi, vt, vti, uv_size=16)
    verts, K, Rt = torch.zeros(2, 874, 3), torch.zeros(1, 3, 3), torch.zeros(1, 3, 4)
    frag = {"face": torch.zeros(2, 8, 8, dtype=torch.int32), "bary": torch.zeros(2, 8, 8, 3)}
    calls = {"rasterize": lambda x: rast.rasterize(x, K, Rt), "render": lambda x: rast.render(x, torch.zeros(1, 3, 4, 4), K, Rt),
             "interpolate": lambda x: rast.interpolate(frag, x), "render_motion": lambda x: RD.render_motion(rast, sf, x, K, Rt)}
    for name, call in calls.items():
        with pytest.raises(_lib.A2PError, match="must be a tensor"):
            call(np.zeros((2, 874, 3), np.float32))
        with pytest.raises(_lib.A2PError, match="no CPU implementation"):
            call(verts)
    for call in (rast.mask, lambda f: rast.sample_texture(f, torch.zeros(1, 3, 4, 4))):
        with pytest.raises(_lib.A2PError, match="no CPU implementation"):
            call(frag)
        with pytest.raises(_lib.A2PError, match="the dict rasterize returns"):
            call({"face": frag["face"]})
    with pytest.raises(_lib.A2PError, match="background and output_filters must be None"):
        rast.render(verts, torch.zeros(1, 3, 4, 4), K, Rt, background=torch.zeros(1))
    with pytest.raises(_lib.A2PError, match=r"vertices must be \[B, T, 874, 3\]"):
        RD.render_motion(rast, sf, torch.zeros(2, 5, 3), K, Rt)
    with pytest.raises(_lib.A2PError, match="choose from"):
        RD.render_motion(rast, sf, verts, K, Rt, outputs=("depth", "albedo"))
    with pytest.raises(_lib.A2PError, match="positive byte budget"):
        RD.render_motion(rast, sf, verts, K, Rt, max_bytes=0)


def test_the_new_exports_are_bound():
    names = {"a2p_render_rasterize", "a2p_render_interpolate", "a2p_render_texture"}
    assert names <= set(_lib.EXPORTS)
    src = open(os.path.join(ROOT, "include", "a2p_hip.h")).read()
    for name, val in (("SIZE", _lib.RENDER_MAX_SIZE), ("CHANNELS", _lib.RENDER_MAX_CHANNELS)):
        assert f"#define A2P_RENDER_MAX_{name} {val}\n" in src
    import __graft_entry__ as ge
    ge.build()
    for half in (False, True):
        lib = _lib.load(half)
        assert all(hasattr(lib, n) for n in names)
        # argument checks come before any GPU work
        with pytest.raises(_lib.A2PError, match="render_rasterize: null argument"):
            _lib.check(lib.a2p_render_rasterize(None, 0, 1, None, 1, None, 0, None, 0, 4, 4, 1e-3, None, None, None, None, None, None),
                       "a2p_render_rasterize")
        with pytest.raises(_lib.A2PError, match="render_interpolate: null argument"):
            _lib.check(lib.a2p_render_interpolate(None, 0, 1, 1, None, 1, None, None, 4, 4, None, None), "a2p_render_interpolate")
        with pytest.raises(_lib.A2PError, match="render_texture: null argument"):
            _lib.check(lib.a2p_render_texture(None, None, 0, 4, 4, None, 1, None, 1, None, 0, 1, 4, 4, 0, None, None), "a2p_render_texture")


# ------------------------------------------------------------------------------------------------ command line
def test_the_command_line_parser(tmp_path):
    base = ["--geometry", "g.npy", "--assets", "a.pt", "--out", "o.npy"]
    args = RD.parser().parse_args(base)
    assert tuple(args.size) == (256, 256) and args.outputs == ["depth", "normals", "view_cos", "mask"] and args.fov == 40.0
    assert args.eye is None and args.camera_json is None and args.png_dir is None and args.frames is None
    args = RD.parser().parse_args(base + ["--size", "48", "64", "--eye", "0", "1", "2", "--target", "0", "0", "0", "--fov", "30", "--outputs",
                                          "depth", "mask", "--frames", "2:5", "--png-dir", "p"])
    assert tuple(args.size) == (48, 64) and args.eye == [0.0, 1.0, 2.0] and args.outputs == ["depth", "mask"] and args.frames == "2:5"
    for bad in (["--eye", "0", "0", "1", "--camera-json", "c.json"], ["--outputs", "albedo"], ["--size", "48"], ["--eye", "0", "1"]):
        with pytest.raises(SystemExit):
            RD.parser().parse_args(base + bad)
    with pytest.raises(SystemExit):
        RD.parser().parse_args(base[:-2])                                     # --out is required
    np.save(tmp_path / "geometry.npy", {"joints": np.zeros((1, 2, 4, 3), np.float32)})
    with pytest.raises(_lib.A2PError, match="holds no `vertices`"):
        RD.main(["--geometry", str(tmp_path / "geometry.npy"), "--assets", str(tmp_path / "none.pt"), "--out", str(tmp_path / "o.npy")])


def test_png_files_have_the_image_size(tmp_path):
    rs = np.random.RandomState(4)
    mask = (rs.rand(1, 2, 1, 6, 9) > 0.4).astype(np.float32)
    normals = rs.randn(1, 2, 3, 6, 9).astype(np.float32)
    normals = normals / np.linalg.norm(normals, axis=2, keepdims=True) * mask
    n = RD.write_pngs({"mask": mask, "normals": normals, "depth": (2 + rs.rand(1, 2, 1, 6, 9).astype(np.float32)) * mask}, str(tmp_path))
    assert n == 6 and sorted(os.listdir(tmp_path))[0] == "depth_00_00000.png"
    from PIL import Image
    img = np.asarray(Image.open(tmp_path / "normals_00_00001.png"))
    assert img.shape == (6, 9, 3) and np.array_equal(img, np.clip(np.rint(127.5 * (1 + normals[0, 1]) * mask[0, 1]), 0, 255).transpose(1, 2, 0))
    grey = np.asarray(Image.open(tmp_path / "mask_00_00000.png"))
    assert grey.shape == (6, 9) and np.array_equal(grey, 255 * mask[0, 0, 0])
    depth = np.asarray(Image.open(tmp_path / "depth_00_00000.png"))
    assert np.array_equal(depth > 0, mask[0, 0, 0] > 0)


def test_the_command_line_cameras(tmp_path):
    """--camera-json is taken as given; without a camera the default one sees every vertex, from the +z side."""
    import json
    base = ["--geometry", "g.npy", "--assets", "a.pt", "--out", "o.npy"]
    K, Rt = R.look_at([0, 0, 5], [0, 0, 0], [0, 1, 0], 30, 44, 40.0)
    (tmp_path / "one.json").write_text(json.dumps({"K": K.tolist(), "Rt": Rt.tolist()}))
    (tmp_path / "two.json").write_text(json.dumps({"K": [K.tolist()] * 2, "Rt": [Rt.tolist()] * 2}))
    verts = np.random.RandomState(8).randn(1, 2, 50, 3).astype(np.float32) * [0.4, 1.0, 0.2]
    for name, n in (("one.json", 1), ("two.json", 2)):
        Kc, Rtc = RD._camera_from_args(RD.parser().parse_args(base + ["--camera-json", str(tmp_path / name)]), verts, 30, 44)
        assert Kc.shape == (n, 3, 3) and Rtc.shape == (n, 3, 4) and Kc.dtype == Rtc.dtype == torch.float32
        assert np.array_equal(Kc[0].numpy(), K.astype(np.float32)) and np.array_equal(Rtc[-1].numpy(), Rt.astype(np.float32))
    with pytest.raises(_lib.A2PError, match="--target goes with --eye"):
        RD._camera_from_args(RD.parser().parse_args(base + ["--camera-json", str(tmp_path / "one.json"), "--target", "0", "0", "0"]), verts, 30, 44)
    for size in ((30, 44), (44, 30)):
        Kc, Rtc = RD._camera_from_args(RD.parser().parse_args(base), verts, *size)
        p = R.project(verts.reshape(1, -1, 3), Kc.numpy(), Rtc.numpy())[0]
        assert Kc.shape == (1, 3, 3) and p[:, 2].min() > 0 and RD.camera_centre(Rtc)[0, 2] > verts[..., 2].max()
        assert p[:, 0].min() >= 0 and p[:, 0].max() <= size[1] and p[:, 1].min() >= 0 and p[:, 1].max() <= size[0]
    Kc, Rtc = RD._camera_from_args(RD.parser().parse_args(base + ["--eye", "1", "2", "3", "--fov", "50"]), verts, 30, 44)
    want = RD.look_at([1, 2, 3], (verts.reshape(-1, 3).min(0) + verts.reshape(-1, 3).max(0)) / 2, [0, 1, 0], 30, 44, 50.0)
    assert torch.equal(Kc[0], want[0]) and torch.equal(Rtc[0], want[1])
