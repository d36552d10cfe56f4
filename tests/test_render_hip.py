"""Rendered images on the MI355X (csrc/kernels_render.h, audio2photoreal_amd/render.py) against the float64 restatement
(tests/render_restatement.py) on the two-layer fixture scene (tests/golden/golden_render_v1.npz).

Gate: face images are compared with array_equal, no pixel excluded (the fixture's cameras keep every pixel centre clear of every
edge and every winner clear of its runner-up by 8 x the float32 error, see tests/golden/make_golden_render.py).  The normalised
error of every float output (max |difference| / max |value|) is at most 4 x the error of the float32 restatement against the
float64 one on the same input.  The factor 4 pays for the device's fused multiply-adds and division.  No number is hard-coded;
every measured value goes to record(...) beside its allowance (render_* entries).  Exact branches are compared with ==."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import render_restatement as R
from audio2photoreal_amd import _lib
from audio2photoreal_amd import render as RD
from audio2photoreal_amd import skinning as SK
from audio2photoreal_amd import surface as S
from conftest import record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, F1 = 874, 792                                                              # vertices of the scene, faces of one layer


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_render_v1.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def mesh(gold):
    return {"vi": gold["vi"].astype(np.int64), "vt": gold["vt"], "vti": gold["vti"].astype(np.int64)}


@pytest.fixture(scope="module")
def rast(mesh):
    """The product object of the fixture scene at each of the three image sizes."""
    return [RD.BodyRasterizer.from_arrays(mesh["vi"], mesh["vt"], mesh["vti"], H, W) for H, W in R.SIZES]


@pytest.fixture(scope="module")
def want(gold, mesh):
    """The restatement's fragments of the three fixture frames, in float64 and in float32, computed once."""
    out = []
    for k, (H, W) in enumerate(R.SIZES):
        args = (gold["verts"][k:k + 1], mesh["vi"], gold["K"][k:k + 1], gold["Rt"][k:k + 1], H, W)
        out.append((R.rasterize(*args), R.rasterize(*args, dtype=np.float32)))
        assert np.array_equal(out[-1][0]["face"], out[-1][1]["face"])
    return out


@pytest.fixture(scope="module")
def frags(dev, gold, rast):
    """The GPU's fragments of the three fixture frames."""
    return [rast[k].rasterize(up(gold["verts"][k:k + 1], dev), up(gold["K"][k:k + 1], dev), up(gold["Rt"][k:k + 1], dev)) for k in range(3)]


def gate(name, got, want, allowance):
    """Record and assert one output: got (device tensor) against want (float64) within `allowance` (normalised)."""
    err = R.nerr(got.cpu().numpy(), want)
    record(name, err=err, allowance=float(allowance))
    assert np.isfinite(err) and err <= allowance, (name, err, allowance)


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def same(a: dict, b: dict):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


# ------------------------------------------------------------------------------------------------ the fixture scene
def test_fixture_faces_barycentrics_and_depth(gold, want, frags):
    for k, (H, W) in enumerate(R.SIZES):
        f64, f32 = want[k]
        got = frags[k]
        assert got["face"].shape == (1, H, W) and got["bary"].shape == (1, H, W, 3) and got["depth"].shape == (1, H, W)
        assert (got["face"].dtype, got["bary"].dtype, got["depth"].dtype) == (torch.int32, torch.float32, torch.float32)
        face = got["face"].cpu().numpy()
        record(f"render_fixture_face{k}", differing_pixels=int((face != f64["face"]).sum()), excluded_pixels=0, covered=int((face >= 0).sum()))
        assert np.array_equal(face[0], gold[f"face{k}"]) and np.array_equal(face, f64["face"])
        gate(f"render_fixture_bary{k}", got["bary"], f64["bary"], 4 * R.nerr(f32["bary"], f64["bary"]))
        gate(f"render_fixture_depth{k}", got["depth"], f64["depth"], 4 * R.nerr(f32["depth"], f64["depth"]))
        hole = got["face"] < 0
        assert bool(hole.any()) and bool((got["face"][hole] == -1).all())
        assert bool((got["bary"][hole] == 0).all()) and bool((got["depth"][hole] == 0).all()) and bool((got["depth"][~hole] > 0).all())


@pytest.mark.parametrize("C", [1, 7, 16])
def test_interpolate_channel_counts(dev, mesh, rast, want, frags, C):
    k = C % 3                                                                 # a different frame and size per channel count
    H, W = R.SIZES[k]
    f64, f32 = want[k]
    values = np.random.RandomState(20 + C).randn(1, V, C).astype(np.float32)
    ref = R.interpolate(values, mesh["vi"], f64["face"], f64["bary"])
    allow = 4 * R.nerr(R.interpolate(values, mesh["vi"], f32["face"], f32["bary"], np.float32), ref)
    out = rast[k].interpolate(frags[k], up(values, dev))
    assert out.shape == (1, C, H, W) and out.dtype == torch.float32
    gate(f"render_interpolate_C{C}", out, ref, allow)
    assert bool((out[:, :, frags[k]["face"][0] < 0] == 0).all())
    with pytest.raises(RD.A2PError, match="1 <= C <= 16"):
        rast[k].interpolate(frags[k], torch.zeros(1, V, 17, device=dev))
    with pytest.raises(RD.A2PError, match=r"fragments\['face'\] must be int32"):
        rast[(k + 1) % 3].interpolate(frags[k], up(values, dev))              # fragments of another image size


@pytest.mark.parametrize("flip", [False, True])
def test_render_samples_the_texture(dev, gold, mesh, want, frags, flip):
    tex = gold["tex"]
    assert tex.shape == (3, 3, 40, 56)
    for k, (H, W) in enumerate(R.SIZES):                                      # one frame per size, a shared [1, ...] texture
        f64, f32 = want[k]
        rz = RD.BodyRasterizer.from_arrays(mesh["vi"], mesh["vt"], mesh["vti"], H, W, flip_uv=flip)
        ref = R.sample_texture(tex[k:k + 1], mesh["vt"], mesh["vti"], f64["face"], f64["bary"], flip)
        allow = 4 * R.nerr(R.sample_texture(tex[k:k + 1], mesh["vt"], mesh["vti"], f32["face"], f32["bary"], flip, np.float32), ref)
        out = rz.render(up(gold["verts"][k:k + 1], dev), up(tex[k:k + 1], dev), up(gold["K"][k:k + 1], dev), up(gold["Rt"][k:k + 1], dev))
        assert set(out) == {"render"} and out["render"].shape == (1, 3, H, W)
        gate(f"render_texture{k}_flip{int(flip)}", out["render"], ref, allow)
        assert torch.equal(out["render"], rz.sample_texture(frags[k], up(tex[k:k + 1], dev)))
        assert bool((out["render"][:, :, frags[k]["face"][0] < 0] == 0).all())
    # frame 0 three times with three textures [3, 3, 40, 56], and with one shared texture
    H, W = R.SIZES[0]
    f64, f32 = want[0]
    rep = lambda x: np.repeat(x, 3, axis=0)
    rz = RD.BodyRasterizer.from_arrays(mesh["vi"], mesh["vt"], mesh["vti"], H, W, flip_uv=flip)
    verts3, K, Rt = up(rep(gold["verts"][:1]), dev), up(gold["K"][:1], dev), up(gold["Rt"][:1], dev)
    ref = R.sample_texture(tex, mesh["vt"], mesh["vti"], rep(f64["face"]), rep(f64["bary"]), flip)
    allow = 4 * R.nerr(R.sample_texture(tex, mesh["vt"], mesh["vti"], rep(f32["face"]), rep(f32["bary"]), flip, np.float32), ref)
    per_frame = rz.render(verts3, up(tex, dev), K, Rt)["render"]
    gate(f"render_texture_per_frame_flip{int(flip)}", per_frame, ref, allow)
    shared = rz.render(verts3, up(tex[1:2], dev), K, Rt)["render"]
    assert torch.equal(shared[0], per_frame[1]) and torch.equal(shared[2], per_frame[1]) and not torch.equal(per_frame[0], per_frame[1])
    with pytest.raises(RD.A2PError, match="tex must be float32"):
        rz.render(verts3, up(tex[:2], dev), K, Rt)
    with pytest.raises(RD.A2PError, match="background and output_filters must be None"):
        rz.render(verts3, up(tex, dev), K, Rt, output_filters=["render"])


def test_shared_and_per_frame_cameras_give_the_same_bits(dev, gold, rast):
    verts = up(gold["verts"], dev)                                            # three different frames, one camera
    K, Rt = up(gold["K"][1:2], dev), up(gold["Rt"][1:2], dev)
    shared = rast[1].rasterize(verts, K, Rt)
    assert same(shared, rast[1].rasterize(verts, K.repeat(3, 1, 1), Rt.repeat(3, 1, 1)))
    assert same(shared, rast[1].rasterize(verts, K[0], Rt.repeat(3, 1, 1)))   # [3, 3] counts as shared
    assert same(shared, rast[1].rasterize(verts, K.repeat(3, 1, 1), Rt[0]))
    mixed = rast[1].rasterize(verts, up(gold["K"][[1, 1, 1]], dev), up(gold["Rt"][[1, 0, 1]], dev))       # a camera of its own for frame 1
    assert all(torch.equal(mixed[k][[0, 2]], shared[k][[0, 2]]) for k in shared) and not torch.equal(mixed["face"][1], shared["face"][1])
    with pytest.raises(RD.A2PError, match=r"K must be float32 \[3 or 1, 3, 3\]"):
        rast[1].rasterize(verts, K.repeat(2, 1, 1), Rt)
    with pytest.raises(RD.A2PError, match="Rt must be float32"):
        rast[1].rasterize(verts, K, Rt.double())
    with pytest.raises(RD.A2PError, match=r"verts must be float32 \[N, 874, 3\]"):
        rast[1].rasterize(verts[:, :-1], K, Rt)


# ------------------------------------------------------------------------------------------------ occlusion, ties
def test_the_nearer_layer_wins_whatever_the_face_order(dev, gold, mesh, frags):
    vi, vt, vti = mesh["vi"], mesh["vt"], mesh["vti"]
    for k, (H, W) in enumerate(R.SIZES):
        args = (up(gold["verts"][k:k + 1], dev), up(gold["K"][k:k + 1], dev), up(gold["Rt"][k:k + 1], dev))
        front = RD.BodyRasterizer.from_arrays(vi[:F1], vt, vti[:F1], H, W, n_verts=V).rasterize(*args)
        back = RD.BodyRasterizer.from_arrays(vi[F1:], vt, vti[F1:], H, W, n_verts=V).rasterize(*args)
        full = frags[k]
        both = (front["face"] >= 0) & (back["face"] >= 0)
        if k < 2:                                                             # at the grazing angle the layers barely overlap on screen
            assert int(both.sum()) > 0.3 * int((full["face"] >= 0).sum())
        # every pixel: the layer with the smaller depth, or the only one that covers it; depth and barycentrics are that layer's
        nearer = (front["face"] >= 0) & (~(back["face"] >= 0) | (front["depth"] <= back["depth"]))
        expect = torch.where(nearer, front["face"], torch.where(back["face"] >= 0, back["face"] + F1, back["face"]))
        assert torch.equal(full["face"], expect)
        assert torch.equal(full["depth"], torch.where(nearer, front["depth"], back["depth"]))
        assert torch.equal(full["bary"], torch.where(nearer[..., None], front["bary"], back["bary"]))
        if k == 0:                                                            # seen from the front the first layer hides the second
            assert bool((full["face"][both] < F1).all())
        record(f"render_occlusion{k}", both_layers=int(both.sum()), front_wins=int((full["face"][both] < F1).sum()))
        # the two halves of the face list swapped: the same surfaces win, with shifted indices
        swapped = RD.BodyRasterizer.from_arrays(np.concatenate([vi[F1:], vi[:F1]]), vt, np.concatenate([vti[F1:], vti[:F1]]), H, W).rasterize(*args)
        shifted = torch.where(full["face"] < 0, full["face"], (full["face"] + F1) % (2 * F1))
        assert torch.equal(swapped["face"], shifted) and torch.equal(swapped["depth"], full["depth"]) and torch.equal(swapped["bary"], full["bary"])


def test_the_lowest_face_wins_a_tie(dev, gold, mesh, frags):
    """A visible face listed again as face 0 and another listed again as the last face: equal depth bits on all their pixels."""
    vi, vti = mesh["vi"], mesh["vti"]
    H, W = R.SIZES[0]
    face = gold["face0"]
    seen = [f for f in np.unique(face[face >= 0]) if (face == f).sum() >= 3]
    a, b = int(seen[len(seen) // 3]), int(seen[-1])
    vi2, vti2 = np.concatenate([vi[a:a + 1], vi, vi[b:b + 1]]), np.concatenate([vti[a:a + 1], vti, vti[b:b + 1]])
    got = RD.BodyRasterizer.from_arrays(vi2, mesh["vt"], vti2, H, W).rasterize(
        up(gold["verts"][:1], dev), up(gold["K"][:1], dev), up(gold["Rt"][:1], dev))
    expect = np.where(face < 0, -1, np.where(face == a, 0, face + 1))         # a's pixels report 0, b's the earlier copy b + 1
    assert np.array_equal(got["face"][0].cpu().numpy(), expect)
    assert (expect == 0).sum() >= 3 and (expect == b + 1).sum() >= 3 and not (expect == a + 1).any() and not (expect == len(vi2) - 1).any()
    assert torch.equal(got["depth"], frags[0]["depth"]) and torch.equal(got["bary"], frags[0]["bary"])


# ------------------------------------------------------------------------------------------------ exact branches
def test_near_and_zero_area_faces_vanish_whole(dev, gold, mesh, frags):
    vi, vt, vti = mesh["vi"], mesh["vt"], mesh["vti"]
    H, W = R.SIZES[0]
    face = gold["face0"]
    f = int(np.bincount(face[face >= 0]).argmax())                            # the face with the most pixels
    K, Rt = gold["K"][0].astype(np.float64), gold["Rt"][0].astype(np.float64)
    centre = -Rt[:, :3].T @ Rt[:, 3]
    close = centre + Rt[:, :3].T @ np.array([0.0, 0.0, 5e-4])                 # half of `near` in front of the camera
    verts = np.concatenate([gold["verts"][:1], close[None, None].astype(np.float32)], 1)
    near_vi = vi.copy()
    near_vi[f, 1] = V                                                         # one corner of f becomes the close vertex
    flat_vi = vi.copy()
    flat_vi[f] = vi[f, 0]                                                     # f becomes a point: zero area
    cam = (up(gold["K"][:1], dev), up(gold["Rt"][:1], dev))
    dropped = RD.BodyRasterizer.from_arrays(near_vi, vt, vti, H, W, n_verts=V + 1).rasterize(up(verts, dev), *cam)
    flat = RD.BodyRasterizer.from_arrays(flat_vi, vt, vti, H, W, n_verts=V + 1).rasterize(up(verts, dev), *cam)
    assert same(dropped, flat)
    was_f = frags[0]["face"] == f
    assert int(was_f.sum()) >= 3 and not bool((dropped["face"] == f).any())
    assert all(torch.equal(dropped[k][~was_f], frags[0][k][~was_f]) for k in dropped)          # every other pixel is unchanged
    assert bool((dropped["face"][was_f] >= 0).all())                          # f was hiding other faces: they show now
    # a near plane of the caller's own: everything nearer than the scene's median depth goes, whole faces at a time
    z = R.project(gold["verts"][:1], gold["K"][:1], gold["Rt"][:1])[0, :, 2]
    near = float(np.median(z))
    cut = RD.BodyRasterizer.from_arrays(vi, vt, vti, H, W, near=near).rasterize(up(gold["verts"][:1], dev), *cam)
    alive = np.nonzero((z[vi] >= np.float32(near)).all(1))[0]
    got = np.unique(cut["face"].cpu().numpy())
    assert 0 < len(alive) < len(vi) and np.isin(got[got >= 0], alive).all() and bool((cut["depth"][cut["face"] >= 0] >= near * (1 - 1e-6)).all())


def guarded(dev, shape, dtype, fill, pad=4096):
    """(view of `shape`, whole buffer): the view sits between two guard bands holding `fill`, like itself."""
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * pad,), fill, dtype=dtype, device=dev)
    return whole[pad:pad + n].view(*shape), whole


def test_off_screen_triangles_and_prefilled_outputs_through_the_c_abi(dev):
    """Three triangles on a 37 x 53 image: one entirely off-screen, one hanging over the left and top borders, one over the right
    and bottom corner.  Outputs and scratch are filled with NaN (face with a marker) and sit between guard bands."""
    H, W = 37, 53
    K = np.array([[[30.0, 0, 26.5], [0, 30, 18.5], [0, 0, 1]]], np.float32)
    Rt = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)[None].astype(np.float32)
    verts = np.array([[[-9.1, 0.2, 3], [-7.3, 0.4, 3], [-8.2, 1.7, 3.5],      # u < 0 for every corner
                       [-3.13, -2.21, 3], [0.47, -0.33, 3.2], [-1.71, 1.37, 2.8],
                       [0.93, 0.41, 2], [2.77, 0.83, 2.3], [1.21, 2.49, 2.6]]], np.float32)
    vi = np.arange(9).reshape(3, 3)
    assert R.edge_clearance(verts, vi, K, Rt, H, W) > 1e-3                    # the scene itself: no centre near an edge
    ref = R.rasterize(verts, vi, K, Rt, H, W)
    ref32 = R.rasterize(verts, vi, K, Rt, H, W, dtype=np.float32)
    seen = set(np.unique(ref["face"]))
    assert seen == {-1, 1, 2} and ref["face"][0, 0, 0] == 1 and ref["face"][0, H - 1, W - 1] == 2 and np.array_equal(ref32["face"], ref["face"])
    nan = float("nan")
    face, face_all = guarded(dev, (1, H, W), torch.int32, -7)
    bary, bary_all = guarded(dev, (1, H, W, 3), torch.float32, nan)
    depth, depth_all = guarded(dev, (1, H, W), torch.float32, nan)
    proj, proj_all = guarded(dev, (1, 9, 3), torch.float32, nan)
    key, key_all = guarded(dev, (1, H, W), torch.int64, -7)
    tv, tvi, tK, tRt = up(verts, dev), up(vi.astype(np.int32), dev), up(K, dev), up(Rt, dev)
    lib = _lib.load()
    _lib.check(lib.a2p_render_rasterize(_lib.ptr(tv), 1, 9, _lib.ptr(tvi), 3, _lib.ptr(tK), 0, _lib.ptr(tRt), 0, H, W, 1e-3, _lib.ptr(proj),
                                        _lib.ptr(key), _lib.ptr(face), _lib.ptr(bary), _lib.ptr(depth), _lib.current_stream(dev)),
               "a2p_render_rasterize")
    torch.cuda.synchronize()
    pad = 4096
    for whole, n in ((bary_all, 3 * H * W), (depth_all, H * W), (proj_all, 27)):
        assert bool(torch.isnan(whole[:pad]).all()) and bool(torch.isnan(whole[pad + n:]).all())
    for whole in (face_all, key_all):
        assert bool((whole[:pad] == -7).all()) and bool((whole[pad + H * W:] == -7).all())
    assert np.array_equal(face.cpu().numpy(), ref["face"])
    gate("render_offscreen_bary", bary, ref["bary"], 4 * R.nerr(ref32["bary"], ref["bary"]))
    gate("render_offscreen_depth", depth, ref["depth"], 4 * R.nerr(ref32["depth"], ref["depth"]))
    hole = face < 0
    assert bool((bary[hole] == 0).all()) and bool((depth[hole] == 0).all()) and bool(torch.isfinite(bary).all())
    # the per-pixel passes into NaN as well: background is written as exactly 0
    values = up(np.random.RandomState(3).randn(1, 9, 5).astype(np.float32), dev)
    out, out_all = guarded(dev, (1, 5, H, W), torch.float32, nan)
    _lib.check(lib.a2p_render_interpolate(_lib.ptr(values), 1, 9, 5, _lib.ptr(tvi), 3, _lib.ptr(face), _lib.ptr(bary), H, W, _lib.ptr(out),
                                          _lib.current_stream(dev)), "a2p_render_interpolate")
    vt = up(np.random.RandomState(4).rand(9, 2).astype(np.float32), dev)
    tex = up(np.random.RandomState(5).randn(1, 2, 6, 7).astype(np.float32), dev)
    img, img_all = guarded(dev, (1, 2, H, W), torch.float32, nan)
    _lib.check(lib.a2p_render_texture(_lib.ptr(face), _lib.ptr(bary), 1, H, W, _lib.ptr(vt), 9, _lib.ptr(tvi), 3, _lib.ptr(tex), 0, 2, 6, 7, 0,
                                      _lib.ptr(img), _lib.current_stream(dev)), "a2p_render_texture")
    torch.cuda.synchronize()
    for view, whole in ((out, out_all), (img, img_all)):
        assert bool(torch.isfinite(view).all()) and bool((view[:, :, hole[0]] == 0).all()) and bool((view[:, :, ~hole[0]] != 0).any())
        assert bool(torch.isnan(whole[:pad]).all()) and bool(torch.isnan(whole[pad + view.numel():]).all())
    # only the wanted outputs: NULL skips one, the others hold the same bits
    only, _ = guarded(dev, (1, H, W), torch.float32, nan)
    _lib.check(lib.a2p_render_rasterize(_lib.ptr(tv), 1, 9, _lib.ptr(tvi), 3, _lib.ptr(tK), 0, _lib.ptr(tRt), 0, H, W, 1e-3, _lib.ptr(proj),
                                        _lib.ptr(key), None, None, _lib.ptr(only), _lib.current_stream(dev)), "a2p_render_rasterize")
    assert torch.equal(only, depth)
    for bad, match in (((0, 8), "need 1 <= H, W"), ((8, _lib.RENDER_MAX_SIZE + 1), "need 1 <= H, W")):
        with pytest.raises(_lib.A2PError, match=match):
            _lib.check(lib.a2p_render_rasterize(_lib.ptr(tv), 1, 9, _lib.ptr(tvi), 3, _lib.ptr(tK), 0, _lib.ptr(tRt), 0, bad[0], bad[1], 1e-3,
                                                _lib.ptr(proj), _lib.ptr(key), _lib.ptr(face), None, None, None), "a2p_render_rasterize")
    with pytest.raises(_lib.A2PError, match="must not alias an input"):
        _lib.check(lib.a2p_render_rasterize(_lib.ptr(tv), 1, 9, _lib.ptr(tvi), 3, _lib.ptr(tK), 0, _lib.ptr(tRt), 0, H, W, 1e-3, _lib.ptr(tv),
                                            _lib.ptr(key), _lib.ptr(face), None, None, None), "a2p_render_rasterize")
    with pytest.raises(_lib.A2PError, match="near=0"):
        _lib.check(lib.a2p_render_rasterize(_lib.ptr(tv), 1, 9, _lib.ptr(tvi), 3, _lib.ptr(tK), 0, _lib.ptr(tRt), 0, H, W, 0.0, _lib.ptr(proj),
                                            _lib.ptr(key), _lib.ptr(face), None, None, None), "a2p_render_rasterize")


def test_texture_coordinates_0_and_1_hit_the_corner_texels(dev):
    """Hand-made fragments whose barycentrics select one corner of a face: uv is exactly (0, 0), (1, 0), (0, 1) or (1, 1), and
    the sample is the corner texel with weight 1 (the taps beyond the border count 0)."""
    vt = np.array([[0.0, 0], [1, 0], [0, 1], [1, 1]], np.float32)
    vti = np.array([[0, 1, 2], [3, 1, 2]])
    rz = RD.BodyRasterizer.from_arrays(vti, vt, vti, 2, 3)
    face = torch.tensor([[[0, 0, 0], [1, -1, 5]]], dtype=torch.int32, device=dev)           # 5: not a face, counts as background
    bary = torch.zeros(1, 2, 3, 3, device=dev)
    bary[0, 0, 0, 0] = bary[0, 0, 1, 1] = bary[0, 0, 2, 2] = bary[0, 1, 0, 0] = 1.0
    bary[0, 1, 2, 0] = 1.0
    tex = torch.from_numpy(np.random.RandomState(6).randn(1, 4, 40, 56).astype(np.float32)).to(dev)
    out = rz.sample_texture({"face": face, "bary": bary}, tex)
    assert torch.equal(out[0, :, 0, 0], tex[0, :, 0, 0]) and torch.equal(out[0, :, 0, 1], tex[0, :, 0, 55])
    assert torch.equal(out[0, :, 0, 2], tex[0, :, 39, 0]) and torch.equal(out[0, :, 1, 0], tex[0, :, 39, 55])
    assert bool((out[0, :, 1, 1:] == 0).all())
    flipped = RD.BodyRasterizer.from_arrays(vti, vt, vti, 2, 3, flip_uv=True).sample_texture({"face": face, "bary": bary}, tex)
    assert torch.equal(flipped[0, :, 0, 0], tex[0, :, 39, 0]) and torch.equal(flipped[0, :, 1, 0], tex[0, :, 0, 55])
    assert torch.equal(rz.interpolate({"face": face, "bary": bary}, torch.arange(12.0, device=dev).reshape(1, 4, 3))[0, :, 1, 2], torch.zeros(3, device=dev))


# ------------------------------------------------------------------------------------------------ determinism, frame independence
@pytest.fixture(scope="module")
def nineteen(dev, gold):
    """19 frames of the scene with a camera each: the per-frame strides of every array are exercised."""
    rs = np.random.RandomState(70)
    verts = gold["verts"][rs.randint(0, 3, 19)] + rs.randn(19, 1, 3).astype(np.float32) * 0.02
    Rt = gold["Rt"][[2] * 19].copy()
    Rt[:, :, 3] += rs.randn(19, 3).astype(np.float32) * 0.03
    K = gold["K"][[2] * 19].copy()
    K[:, 0, 0] *= (1 + rs.rand(19).astype(np.float32) * 0.1)
    values = rs.randn(19, V, 2).astype(np.float32)
    return tuple(up(a, dev) for a in (verts, K, Rt, values, gold["tex"][:1]))


def run_all(rz, verts, K, Rt, values, tex):
    frag = rz.rasterize(verts, K, Rt)
    return {**frag, "values": rz.interpolate(frag, values), "render": rz.sample_texture(frag, tex), "mask": rz.mask(frag)}


def test_frames_do_not_depend_on_the_batch(dev, rast, nineteen):
    verts, K, Rt, values, tex = nineteen
    rz = rast[2]
    H, W = R.SIZES[2]
    full = run_all(rz, verts, K, Rt, values, tex)
    assert full["face"].shape == (19, H, W) and full["values"].shape == (19, 2, H, W) and full["render"].shape == (19, 3, H, W)
    assert full["mask"].shape == (19, 1, H, W) and torch.equal(full["mask"][:, 0] > 0, full["face"] >= 0)
    assert len({int((full["face"][n] >= 0).sum()) for n in range(19)}) > 5   # the frames do differ
    assert same(full, run_all(rz, verts, K, Rt, values, tex)), "two identical runs differ"
    for lo, hi in ((0, 1), (7, 9), (18, 19)):
        alone = run_all(rz, verts[lo:hi], K[lo:hi], Rt[lo:hi], values[lo:hi], tex)
        assert all(torch.equal(alone[k], full[k][lo:hi]) for k in full), (lo, hi)
    empty = run_all(rz, verts[:0], K[:1], Rt[:1], values[:0], tex)
    assert {k: tuple(v.shape) for k, v in empty.items()} == {"face": (0, H, W), "bary": (0, H, W, 3), "depth": (0, H, W), "values": (0, 2, H, W),
                                                             "render": (0, 3, H, W), "mask": (0, 1, H, W)}


def test_a_side_stream_gives_the_same_bits(dev, gold, mesh, rast, nineteen):
    want = run_all(rast[2], *nineteen)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        fresh = RD.BodyRasterizer.from_arrays(mesh["vi"], mesh["vt"], mesh["vti"], *R.SIZES[2])
        got = run_all(fresh, *nineteen)
    side.synchronize()
    assert same(want, got) and all(t.device == dev for t in got.values())
    with pytest.raises(RD.A2PError, match="must live on the MI355X"):
        rast[2].rasterize(nineteen[0].cpu(), nineteen[1], nineteen[2])


# ------------------------------------------------------------------------------------------------ render_motion, command line
@pytest.fixture(scope="module")
def skinned(dev):
    """The skinning fixture's skeleton with its 500 vertices re-meshed as a 25 x 20 grid, one chart (as tests/test_surface_hip.py)."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_skinning_v1.npz"))
    skel = {k.split("/", 1)[1]: g[k] for k in g.files if k.startswith("skel/")}
    sk = SK.BodySkeleton.from_arrays(skel["parents"], skel["pre_rotation"], skel["joint_offset"], skel["transform"],
                                     skel["transform_offsets"], 104, 12, skel["rest_vertices"], skel["skin_indices"], skel["skin_weights"],
                                     template_verts=g["template_verts"], lbs_scale=g["scales"][0], global_scaling=g["global_scaling"])
    vid = lambda i, j: j * 25 + i
    vi = np.array([t for j in range(19) for i in range(24) for t in ([vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)],
                                                                     [vid(i, j), vid(i + 1, j + 1), vid(i, j + 1)])])
    ii, jj = np.meshgrid(np.arange(25), np.arange(20))
    vt = np.stack([0.02 + ii * 0.04, 0.03 + jj * 0.049], -1).reshape(500, 2).astype(np.float32)
    return sk, {"vi": vi, "vt": vt, "vti": vi}


def framing(verts: np.ndarray, H, W, dev):
    """A camera that sees all of `verts` from the +z side."""
    lo, hi = verts.reshape(-1, 3).min(0), verts.reshape(-1, 3).max(0)
    centre = (lo + hi) / 2
    K, Rt = RD.look_at(centre + [0.1 * (hi[0] - lo[0]), 0.0, 1.2 * np.linalg.norm(hi - lo)], centre, [0, 1, 0], H, W, 35.0, device=dev)
    return K[None], Rt[None]


def test_render_motion_on_pose_motion(dev, skinned):
    sk, topo = skinned
    H, W = 40, 52
    sf = S.BodySurface.from_arrays(topo["vi"], topo["vt"], topo["vti"], uv_size=32)
    rz = RD.BodyRasterizer(sf, H, W)
    pose = np.random.RandomState(60).randn(2, 3, 104) * 0.6
    with torch.cuda.device(dev):
        verts = SK.pose_motion(sk, pose)["vertices"]
        K, Rt = framing(verts.cpu().numpy(), H, W, dev)
        names = ("depth", "normals", "view_cos", "positions", "mask")
        maps = RD.render_motion(rz, sf, verts, K, Rt, outputs=names)
        default = RD.render_motion(rz, sf, verts, K, Rt)
    assert verts.shape == (2, 3, 500, 3)
    assert {k: tuple(v.shape) for k, v in maps.items()} == {"depth": (2, 3, 1, H, W), "normals": (2, 3, 3, H, W), "view_cos": (2, 3, 1, H, W),
                                                           "positions": (2, 3, 3, H, W), "mask": (2, 3, 1, H, W)}
    assert set(default) == {"depth", "normals", "view_cos"} and all(torch.equal(default[k], maps[k]) for k in default)
    # equality with the separately called pieces
    flat = verts.reshape(6, 500, 3)
    frag = rz.rasterize(flat, K, Rt)
    assert 0.05 < float((frag["face"] >= 0).float().mean()) < 0.95
    normals, cos = sf.normals_and_view_cos(flat, RD.camera_centre(Rt))
    assert torch.equal(maps["depth"].reshape(6, H, W), frag["depth"]) and torch.equal(maps["mask"].reshape(6, 1, H, W), rz.mask(frag))
    assert torch.equal(maps["normals"].reshape(6, 3, H, W), rz.interpolate(frag, normals))
    assert torch.equal(maps["view_cos"].reshape(6, 1, H, W), rz.interpolate(frag, cos[:, :, None].contiguous()))
    assert torch.equal(maps["positions"].reshape(6, 3, H, W), rz.interpolate(frag, flat))
    eye = RD.camera_centre(Rt)
    assert bool((maps["view_cos"][maps["mask"] > 0].abs() <= 1.0001).all()) and eye.shape == (1, 3)
    # chunked by a tiny byte budget (one frame per chunk), a camera per frame, the flat layout
    Kn, Rtn = K.repeat(6, 1, 1), Rt.repeat(6, 1, 1)
    Rtn[:, :, 3] += torch.linspace(0, 0.5, 6, device=dev)[:, None]
    whole = RD.render_motion(rz, sf, flat, Kn, Rtn, outputs=names)
    tiny = RD.render_motion(rz, sf, flat, Kn, Rtn, outputs=names, max_bytes=1)
    mid = RD.render_motion(rz, sf, verts, Kn, Rtn, outputs=names, max_bytes=4 * 4 * 14 * (500 + H * W) + 100)   # four frames per chunk: 4 + 2
    assert whole["depth"].shape == (6, 1, H, W) and not torch.equal(whole["depth"][0], whole["depth"][5])
    for k in whole:
        assert torch.equal(tiny[k], whole[k]) and torch.equal(mid[k].reshape(whole[k].shape), whole[k]), k
    given = RD.render_motion(rz, sf, flat, Kn, Rtn, outputs=("view_cos",), camera_pos=RD.camera_centre(Rtn))
    assert torch.equal(given["view_cos"], whole["view_cos"])
    with pytest.raises(RD.A2PError, match=r"vertices must be \[B, T, 500, 3\]"):
        RD.render_motion(rz, sf, verts[..., :2], K, Rt)


def test_command_line_matches_the_direct_call(dev, skinned, tmp_path):
    sk, topo = skinned
    rs = np.random.RandomState(61)
    ii, jj = np.meshgrid(np.arange(25), np.arange(20))
    sheet = np.stack([ii * 0.1, jj * 0.1, 0.2 * np.sin(ii * 0.5)], -1).reshape(500, 3)
    verts = (sheet + rs.randn(1, 4, 500, 3) * 0.01).astype(np.float32)
    v2uv = S.compute_v2uv(500, topo["vi"], topo["vti"])
    torch.save({"topology": {"vi": torch.from_numpy(topo["vi"]), "vt": torch.from_numpy(topo["vt"]), "vti": torch.from_numpy(topo["vti"]),
                             "v2uv": torch.from_numpy(v2uv)}}, tmp_path / "static_assets.pt")
    np.save(tmp_path / "geometry.npy", {"joints": np.zeros((1, 4, 40, 3), np.float32), "vertices": verts})
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    argv = ["--geometry", str(tmp_path / "geometry.npy"), "--assets", str(tmp_path / "static_assets.pt"), "--size", "30", "44",
            "--eye", "1.0", "0.5", "4.0", "--target", "1.2", "0.9", "0.0", "--fov", "38", "--frames", "1:3", "--out", str(tmp_path / "frames.npy"),
            "--png-dir", str(tmp_path / "png")]
    r = subprocess.run([sys.executable, "-m", "audio2photoreal_amd.render"] + argv, capture_output=True, text=True, env=env,
                       cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(tmp_path / "frames.npy", allow_pickle=True).item()
    sf = S.BodySurface.from_arrays(topo["vi"], topo["vt"], topo["vti"], v2uv=v2uv)
    with torch.cuda.device(dev):
        K, Rt = RD.look_at([1.0, 0.5, 4.0], [1.2, 0.9, 0.0], [0, 1, 0], 30, 44, 38.0, device=dev)
        want = RD.render_motion(RD.BodyRasterizer(sf, 30, 44), sf, up(verts[:, 1:3], dev), K[None], Rt[None],
                                outputs=("depth", "normals", "view_cos", "mask"))
    assert set(got) == set(want) == {"depth", "normals", "view_cos", "mask"}
    for k in want:
        assert got[k].dtype == np.float32 and got[k].shape[:2] == (1, 2) and np.array_equal(got[k], want[k].cpu().numpy()), k
    from PIL import Image
    files = sorted(os.listdir(tmp_path / "png"))
    assert len(files) == 8 and "mask_00_00001.png" in files and "normals_00_00000.png" in files
    mask = np.asarray(Image.open(tmp_path / "png" / "mask_00_00001.png"))
    assert mask.shape == (30, 44) and np.array_equal(mask > 0, got["mask"][0, 1, 0] > 0) and 0.2 < (mask > 0).mean() < 1.0
    assert np.asarray(Image.open(tmp_path / "png" / "normals_00_00000.png")).shape == (30, 44, 3)
