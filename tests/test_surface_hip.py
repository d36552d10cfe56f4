"""Surface maps on the MI355X (csrc/kernels_surface.h, audio2photoreal_amd/surface.py) against the float64 restatement
(tests/surface_restatement.py).

Gate: the normalised error of every output (max |difference| / max |value|) is at most 4 x the float32 error of the same formulas
on the same mesh: for the fixture mesh the reference's own error stored in tests/golden/golden_surface_v1.npz (e_ref), for every
other shape the restatement run in float32 against itself in float64.  The factor 4 pays for the device's sqrtf and division and
for fused multiply-adds.  No number is hard-coded; every measured value goes to record(...) beside its allowance (surf_* entries).
Index images and the exact branches are compared with == / array_equal."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import surface_restatement as R
from audio2photoreal_amd import skinning as SK
from audio2photoreal_amd import surface as S
from conftest import record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 437


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_surface_v1.npz"))


@pytest.fixture(scope="module")
def mesh(gold):
    return {"vi": gold["vi"].astype(np.int64), "vt": gold["vt"], "vti": gold["vti"].astype(np.int64), "n_verts": V}


@pytest.fixture(scope="module")
def fix(mesh):
    """The product object of the fixture mesh at each uv_size the fixture was cleared for."""
    return {H: S.BodySurface.from_arrays(mesh["vi"], mesh["vt"], mesh["vti"], uv_size=H) for H in R.UV_SIZES}


@pytest.fixture(scope="module")
def images(mesh):
    """The restatement's images of the fixture mesh (float64), computed once."""
    return {H: R.uv_images(mesh, H) for H in R.UV_SIZES}


def gate(name, got, want, allowance):
    """Record and assert one output: got (device tensor) against want (float64) within `allowance` (normalised)."""
    err = R.nerr(got.cpu().numpy(), want)
    record(name, err=err, allowance=float(allowance))
    assert np.isfinite(err) and err <= allowance, (name, err, allowance)


def own(fn):
    """(float64 result, 4 x the float32 restatement's error against it): the allowance of a shape outside the fixture."""
    want = fn(np.float64)
    return want, 4 * R.nerr(fn(np.float32), want)


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------ the fixture mesh
def test_fixture_normals_and_view_cosine(dev, gold, mesh, fix):
    sf, verts, cam = fix[48], gold["verts"], gold["camera"]
    tv, tc = up(verts, dev), up(cam, dev)
    e = {k: float(gold[f"e_ref/{k}"]) for k in ("normals", "view_cos", "view_cos_shared")}
    normals = sf.normals(tv)
    assert normals.shape == (3, V, 3) and normals.dtype == torch.float32
    gate("surf_fixture_normals", normals, R.vert_normals(verts, mesh["vi"]), 4 * e["normals"])
    cos = sf.view_cos(tv, tc)
    assert cos.shape == (3, V)
    gate("surf_fixture_view_cos", cos, R.view_cos(verts, mesh["vi"], cam), 4 * e["view_cos"])
    gate("surf_fixture_view_cos_shared", sf.view_cos(tv, tc[:1]), R.view_cos(verts, mesh["vi"], cam[:1]), 4 * e["view_cos_shared"])
    both = sf.normals_and_view_cos(tv, tc)
    assert torch.equal(both[0], normals) and torch.equal(both[1], cos)        # one launch gives the bits of the separate ones
    with pytest.raises(S.A2PError, match="camera_pos must be float32"):
        sf.view_cos(tv, tc[:2])
    with pytest.raises(S.A2PError, match=r"verts must be float32 \[N, 437, 3\]"):
        sf.normals(tv[:, :-1])
    with pytest.raises(S.A2PError, match="verts must be float32"):
        sf.normals(tv.double())


def test_fixture_to_uv_with_given_and_rasterised_maps(dev, gold, mesh, fix, images):
    verts = gold["verts"]
    tv = up(verts, dev)
    given = fix[48].with_images(gold["index_image48"], gold["ref/bary48"])
    got = given.to_uv(tv)
    assert got.shape == (3, 3, 48, 48) and given.face_index_image is None
    assert torch.equal(given.index_image.cpu(), torch.from_numpy(gold["index_image48"]))
    gate("surf_fixture_to_uv_given", got, R.to_uv(verts, gold["index_image48"], gold["ref/bary48"]), 4 * float(gold["e_ref/to_uv"]))
    for H in R.UV_SIZES:                                                      # through the surface's own rasterised maps
        index, bary, _ = images[H]
        want, allow = own(lambda dt: R.to_uv(verts, index, R.uv_images(mesh, H, dtype=dt)[1], dt))
        out = fix[H].to_uv(tv)
        assert out.shape == (3, 3, H, H)
        gate(f"surf_fixture_to_uv_raster{H}", out, want, allow)
        hole = torch.from_numpy(~(index != -1).all(-1)).to(dev)
        assert bool((out[:, :, hole] == 0).all()) and bool(hole.any())


@pytest.mark.parametrize("C", [1, 7, 16])
def test_to_uv_channel_counts(dev, gold, fix, C):
    values = np.random.RandomState(20 + C).randn(3, V, C).astype(np.float32)
    given = fix[48].with_images(gold["index_image48"], gold["ref/bary48"])
    want, allow = own(lambda dt: R.to_uv(values, gold["index_image48"], gold["ref/bary48"], dt))
    out = given.to_uv(up(values, dev))
    assert out.shape == (3, C, 48, 48)
    gate(f"surf_to_uv_C{C}", out, want, allow)
    with pytest.raises(S.A2PError, match="1 <= C <= 16"):
        given.to_uv(torch.zeros(1, V, 17, device=dev))


def test_frame_groups_of_to_uv(dev, gold, fix):
    """19 frames: two full groups of 8 frames and a group of 3."""
    values = np.random.RandomState(31).randn(19, V, 2).astype(np.float32)
    given = fix[48].with_images(gold["index_image48"], gold["ref/bary48"])
    want, allow = own(lambda dt: R.to_uv(values, gold["index_image48"], gold["ref/bary48"], dt))
    tvals = up(values, dev)
    out = given.to_uv(tvals)
    gate("surf_to_uv_N19", out, want, allow)
    for lo, hi in ((0, 1), (7, 9), (16, 19), (18, 19)):
        assert torch.equal(given.to_uv(tvals[lo:hi]), out[lo:hi])
    assert given.to_uv(tvals[:0]).shape == (0, 2, 48, 48)


def test_fixture_from_uv(dev, gold, mesh, fix):
    got = fix[48].from_uv(up(gold["values_uv"], dev))
    assert got.shape == (3, V, 4)
    gate("surf_fixture_from_uv", got, R.from_uv(gold["values_uv"], mesh["vt"], gold["ref/v2uv"]), 4 * float(gold["e_ref/from_uv"]))


def test_from_uv_non_square_and_the_image_border(dev, mesh, fix):
    rs = np.random.RandomState(40)
    uv = rs.randn(2, 5, 40, 56).astype(np.float32)                            # H' = 40, W' = 56
    want, allow = own(lambda dt: R.from_uv(uv, mesh["vt"], fix[48].v2uv, dt))
    got = fix[48].from_uv(up(uv, dev))
    assert got.shape == (2, V, 5)
    gate("surf_from_uv_40x56", got, want, allow)
    # texture coordinates exactly 0 and exactly 1: the east / south taps of u = 1 / v = 1 fall outside and count 0
    vt = np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [0.3, 0.6], [1.0, 0.45]], np.float32)
    vi = np.array([[0, 1, 2], [1, 3, 2], [2, 3, 4], [3, 5, 4]])
    sf = S.BodySurface.from_arrays(vi, vt, vi, uv_size=8)
    assert np.array_equal(sf.v2uv, np.repeat(np.arange(6)[:, None], 4, 1))
    want, allow = own(lambda dt: R.from_uv(uv, vt, sf.v2uv, dt))
    got = sf.from_uv(up(uv, dev))
    gate("surf_from_uv_border", got, want, allow)
    corners = torch.from_numpy(uv[:, :, [0, 0, 39, 39], [0, 55, 0, 55]]).permute(0, 2, 1).to(dev)
    assert torch.equal(got[:, :4], corners)                                   # weight 1 on the corner pixel, 0 on the taps outside


# ------------------------------------------------------------------------------------------------ rasterisation
def test_rasterised_images_match_the_rule_on_every_texel(dev, gold, fix, images):
    for H in R.UV_SIZES:
        sf = fix[H]
        with torch.cuda.device(dev):
            index, bary, face = sf.index_image, sf.bary_image, sf.face_index_image
        assert (index.dtype, bary.dtype, face.dtype) == (torch.int32, torch.float32, torch.int32)
        assert index.shape == (H, H, 3) and bary.shape == (H, H, 3) and face.shape == (H, H) and index.device == dev
        want_index, want_bary, want_face = images[H]
        assert np.array_equal(face.cpu().numpy(), want_face) and np.array_equal(face.cpu().numpy(), gold[f"face_image{H}"])
        assert np.array_equal(index.cpu().numpy(), want_index)
        gate(f"surf_raster_bary{H}", bary, want_bary, 4 * float(gold[f"e_ref/bary{H}"]))
        assert bool((bary[face < 0] == 0).all()) and bool((index[face < 0] == -1).all())
        assert sf.index_image is index                                        # rasterised once


def test_lowest_face_wins_where_uv_triangles_overlap(dev, mesh):
    """Face 700's UV triangle is listed again as face 0 and face 10's again as the last face: every texel of both is covered twice."""
    vi = np.concatenate([mesh["vi"][700:701], mesh["vi"], mesh["vi"][10:11]])
    vti = np.concatenate([mesh["vti"][700:701], mesh["vti"], mesh["vti"][10:11]])
    surf = {"vi": vi, "vt": mesh["vt"], "vti": vti}
    sf = S.BodySurface.from_arrays(vi, mesh["vt"], vti, uv_size=130)
    with torch.cuda.device(dev):
        face = sf.face_index_image.cpu().numpy()
    want = R.uv_images(surf, 130)[2]
    assert np.array_equal(face, want)
    assert (face == 0).sum() > 3 and (face == 11).sum() > 3 and not (face == 701).any() and not (face == len(vi) - 1).any()
    flipped = S.BodySurface.from_arrays(vi, mesh["vt"], vti, uv_size=48, flip_uv=True)
    with torch.cuda.device(dev):
        assert np.array_equal(flipped.face_index_image.cpu().numpy(), want_flip(surf))


def want_flip(surf):
    face = R.uv_images(surf, 48, flip_uv=True)[2]
    assert np.array_equal(face, R.uv_images(surf, 48, flip_uv=True, dtype=np.float32)[2])   # v -> 1 - v keeps the clearance at 48
    return face


# ------------------------------------------------------------------------------------------------ exact branches
def test_exact_branches(dev, gold, mesh):
    rs = np.random.RandomState(50)
    # vertex 4 sits only in a face with two identical corners (contributes exactly 0); vertex 5 is used by no face
    vi = np.array([[0, 1, 2], [0, 2, 3], [4, 4, 1]])
    vt = rs.rand(6, 2).astype(np.float32)
    sf = S.BodySurface.from_arrays(vi, vt, vi, v2uv=np.repeat(np.arange(6)[:, None], 4, 1), uv_size=8)
    assert sf.V == 6 and sf.inc_ptr.tolist() == [0, 2, 4, 6, 7, 9, 9]
    verts = up(rs.randn(2, 6, 3).astype(np.float32), dev)
    normals, cos = sf.normals_and_view_cos(verts, up(rs.randn(1, 3).astype(np.float32), dev))
    zero = torch.zeros(2, 3, device=dev)
    assert torch.equal(normals[:, 4], zero) and torch.equal(normals[:, 5], zero)
    assert torch.equal(cos[:, 4], zero[:, 0]) and torch.equal(cos[:, 5], zero[:, 0])
    assert bool((normals[:, :4].norm(dim=-1) > 0.99).all())
    # the degenerate face adds exactly 0 to vertex 1 as well: the same normal as without it
    plain = S.BodySurface.from_arrays(vi[:2], vt, vi[:2], v2uv=np.repeat(np.arange(6)[:, None], 4, 1), uv_size=8)
    assert torch.equal(plain.normals(verts)[:, :4], normals[:, :4])
    # one index of a texel is -1: the texel is written as exactly 0, over whatever the allocation held
    index = gold["index_image48"].copy()
    full = np.argwhere((index != -1).all(-1))
    (i, j), (i2, j2) = full[5], full[40]
    index[i, j, 1] = -1
    index[i2, j2, 2] = -1
    given = S.BodySurface.from_arrays(mesh["vi"], mesh["vt"], mesh["vti"], uv_size=48).with_images(index, gold["ref/bary48"])
    values = up(gold["verts"], dev)
    size = 3 * 3 * 48 * 48
    poison = torch.full((size,), float("nan"), device=dev)                    # the caching allocator hands this block back
    ptr = poison.data_ptr()
    del poison
    out = given.to_uv(values)
    record("surf_to_uv_prefilled_with_nan", reused_block=bool(out.data_ptr() == ptr))
    assert bool(torch.isfinite(out).all())
    assert bool((out[:, :, i, j] == 0).all()) and bool((out[:, :, i2, j2] == 0).all())
    # the same through the C ABI, into an output the test itself filled with NaN
    from audio2photoreal_amd import _lib
    out2 = torch.full((3, 3, 48, 48), float("nan"), device=dev)
    im, ba, _ = given._images(dev)
    _lib.check(_lib.load().a2p_surface_to_uv(_lib.ptr(values), 3, V, 3, _lib.ptr(im), _lib.ptr(ba), 48, _lib.ptr(out2),
                                             _lib.current_stream(dev)), "a2p_surface_to_uv")
    assert torch.equal(out2, out) and bool((out2[:, :, i, j] == 0).all())


# ------------------------------------------------------------------------------------------------ determinism, frame independence
def test_two_runs_and_a_frame_alone_give_the_same_bits(dev, gold, mesh, fix):
    sf = fix[48]
    tv, tc, tu = up(gold["verts"], dev), up(gold["camera"], dev), up(gold["values_uv"], dev)
    run = lambda v, c, u: (*sf.normals_and_view_cos(v, c), sf.to_uv(v), sf.from_uv(u))
    full, again = run(tv, tc, tu), run(tv, tc, tu)
    assert all(torch.equal(a, b) for a, b in zip(full, again)), "two identical runs differ"
    alone = run(tv[1:2], tc[1:2], tu[1:2])
    assert all(a.shape[0] == 1 and torch.equal(a[0], b[1]) for a, b in zip(alone, full)), "frame 1 depends on the batch"
    fresh = S.BodySurface.from_arrays(mesh["vi"], mesh["vt"], mesh["vti"], uv_size=48)      # the rasterisation, run again
    with torch.cuda.device(dev):
        for a, b in zip((fresh.index_image, fresh.bary_image, fresh.face_index_image), (sf.index_image, sf.bary_image, sf.face_index_image)):
            assert a is not b and torch.equal(a, b)


def test_non_default_stream_and_device_placement(dev, gold, mesh, fix):
    sf = fix[48]
    tv, tc, tu = up(gold["verts"], dev), up(gold["camera"], dev), up(gold["values_uv"], dev)
    run = lambda s: (*s.normals_and_view_cos(tv, tc), s.to_uv(tv), s.from_uv(tu))
    want = run(sf)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        fresh = S.BodySurface.from_arrays(mesh["vi"], mesh["vt"], mesh["vti"], uv_size=48)  # rasterises on the side stream too
        got = run(fresh)
    side.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    assert all(t.device == dev for t in got)
    with pytest.raises(S.A2PError, match="must live on the MI355X"):
        sf.normals(tv.cpu())


# ------------------------------------------------------------------------------------------------ surface_maps, command line
@pytest.fixture(scope="module")
def skinned(dev):
    """The skinning fixture's skeleton with its 500 vertices re-meshed as a 25 x 20 grid, one chart."""
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


def test_surface_maps_on_pose_motion(dev, skinned):
    sk, topo = skinned
    sf = S.BodySurface.from_arrays(topo["vi"], topo["vt"], topo["vti"], uv_size=32)
    pose = np.random.RandomState(60).randn(2, 3, 104) * 0.6
    with torch.cuda.device(dev):
        verts = SK.pose_motion(sk, pose)["vertices"]
        cam = torch.tensor([[0.5, 0.2, 30.0]], device=dev)
        maps = S.surface_maps(sf, verts, cam)
        plain = S.surface_maps(sf, verts)
    assert verts.shape == (2, 3, 500, 3)
    assert {k: tuple(v.shape) for k, v in maps.items()} == {
        "normals": (2, 3, 500, 3), "view_cos": (2, 3, 500), "position_uv": (2, 3, 3, 32, 32), "normal_uv": (2, 3, 3, 32, 32),
        "view_cos_uv": (2, 3, 1, 32, 32)}
    assert set(plain) == {"normals", "position_uv", "normal_uv"}
    flat = verts.reshape(6, 500, 3)
    normals, cos = sf.normals_and_view_cos(flat, cam)
    assert torch.equal(maps["normals"].reshape(6, 500, 3), normals) and torch.equal(maps["view_cos"].reshape(6, 500), cos)
    assert torch.equal(maps["position_uv"].reshape(6, 3, 32, 32), sf.to_uv(flat))
    assert torch.equal(maps["normal_uv"].reshape(6, 3, 32, 32), sf.to_uv(normals))
    assert torch.equal(maps["view_cos_uv"].reshape(6, 1, 32, 32), sf.to_uv(cos[:, :, None].contiguous()))
    for k in plain:
        assert torch.equal(plain[k], maps[k]), k
    assert torch.equal(S.surface_maps(sf, flat, cam)["normal_uv"], maps["normal_uv"].reshape(6, 3, 32, 32))
    with pytest.raises(S.A2PError, match=r"vertices must be \[B, T, 500, 3\]"):
        S.surface_maps(sf, verts[..., :2])


def test_command_line_matches_the_direct_call(dev, skinned, tmp_path):
    sk, topo = skinned
    rs = np.random.RandomState(61)
    verts = rs.randn(1, 4, 500, 3).astype(np.float32)
    v2uv = S.compute_v2uv(500, topo["vi"], topo["vti"])
    torch.save({"topology": {"vi": torch.from_numpy(topo["vi"]), "vt": torch.from_numpy(topo["vt"]), "vti": torch.from_numpy(topo["vti"]),
                             "v2uv": torch.from_numpy(v2uv)}}, tmp_path / "static_assets.pt")
    np.save(tmp_path / "geometry.npy", {"joints": np.zeros((1, 4, 40, 3), np.float32), "vertices": verts})
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    argv = ["--geometry", str(tmp_path / "geometry.npy"), "--assets", str(tmp_path / "static_assets.pt"), "--uv-size", "24",
            "--camera", "0.5", "0.25", "9", "--frames", "1:3", "--out", str(tmp_path / "surface.npy")]
    r = subprocess.run([sys.executable, "-m", "audio2photoreal_amd.surface"] + argv, capture_output=True, text=True, env=env,
                       cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    got = np.load(tmp_path / "surface.npy", allow_pickle=True).item()
    sf = S.BodySurface.from_arrays(topo["vi"], topo["vt"], topo["vti"], v2uv=v2uv, uv_size=24)
    with torch.cuda.device(dev):
        want = S.surface_maps(sf, up(verts[:, 1:3], dev), torch.tensor([[0.5, 0.25, 9.0]], device=dev))
    assert set(got) == set(want) == {"normals", "view_cos", "position_uv", "normal_uv", "view_cos_uv"}
    for k in want:
        assert got[k].dtype == np.float32 and got[k].shape[:2] == (1, 2) and np.array_equal(got[k], want[k].cpu().numpy()), k
