"""Host side of the surface maps (audio2photoreal_amd/surface.py), no GPU: the restatement (tests/surface_restatement.py) against
the reference's own float32 outputs on the fixture mesh (tests/golden/golden_surface_v1.npz), the host tables, every rejection of
the constructors, and the refusal to compute anything on the CPU."""
import os

import numpy as np
import pytest
import torch

import surface_restatement as R
from audio2photoreal_amd import _lib
from audio2photoreal_amd import surface as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_surface_v1.npz"))


@pytest.fixture(scope="module")
def mesh(gold):
    return {"vi": gold["vi"].astype(np.int64), "vt": gold["vt"], "vti": gold["vti"].astype(np.int64), "n_verts": 437}


def test_the_fixture_mesh_is_what_the_builder_makes(gold):
    surf = R.make_surface()                                                   # asserts clearance, normal lengths, the 4-index vertex
    for k in ("vi", "vt", "vti", "rest"):
        assert np.array_equal(surf[k], gold[k]), k
    assert np.array_equal(R.make_frames(surf, 5, 3), gold["verts"])
    assert (surf["n_verts"], len(surf["vi"])) == (437, 792)
    ptr, _ = R.incidence(437, surf["vi"])
    assert np.diff(ptr).max() == 70 and np.diff(ptr)[R.FAN[1] * R.NX + R.FAN[0]] == 70      # the fan: more than a wave
    owned = np.array([len(set(r)) for r in gold["ref/v2uv"]])
    assert (owned == 4).sum() == 1 and (owned == 3).sum() >= 1 and (owned == 2).sum() > 10


def test_restatement_reproduces_the_reference_within_float32_rounding(gold, mesh):
    """The reference's float32 outputs sit within a few float32 roundings of the float64 restatement (the error of a handful of
    operations on values of order 1: 64 eps covers the longest chain, from_uv's 31 x coordinate), and the restatement run in
    float32 is as close to them as they are to float64."""
    vi, vt = mesh["vi"], mesh["vt"]
    verts, cam = gold["verts"], gold["camera"]
    want = {"normals": lambda dt: R.vert_normals(verts, vi, dt), "view_cos": lambda dt: R.view_cos(verts, vi, cam, dt),
            "view_cos_shared": lambda dt: R.view_cos(verts, vi, cam[:1], dt),
            "from_uv": lambda dt: R.from_uv(gold["values_uv"], vt, gold["ref/v2uv"], dt),
            "to_uv": lambda dt: R.to_uv(verts, gold["index_image48"], gold["ref/bary48"], dt)}
    for k, fn in want.items():
        e = R.nerr(gold[f"ref/{k}"], fn(np.float64))
        assert e == pytest.approx(float(gold[f"e_ref/{k}"]), rel=1e-6) and 0 < e < 64 * EPS32, (k, e)
        assert R.nerr(fn(np.float32), gold[f"ref/{k}"]) < 64 * EPS32, k
    for H in R.UV_SIZES:
        index, bary, face = R.uv_images(mesh, H)
        assert np.array_equal(face, gold[f"face_image{H}"]) and np.array_equal(index, gold[f"index_image{H}"])
        assert np.array_equal(R.uv_images(mesh, H, dtype=np.float32)[2], face)          # the clearance at work
        assert R.nerr(gold[f"ref/bary{H}"], bary) == pytest.approx(float(gold[f"e_ref/bary{H}"]), rel=1e-6)
        assert float(gold[f"e_ref/bary{H}"]) < 64 * EPS32
        hit = face >= 0
        assert 0.5 < hit.mean() < 0.9 and np.all(bary[hit] > 0) and np.all(bary[~hit] == 0)
        assert not np.isin(np.nonzero(np.all(mesh["vti"] == mesh["vti"][:, :1], axis=1))[0], face).any()   # zero-area faces cover nothing


def test_v2uv_matches_the_reference_exactly(gold, mesh):
    got = S.compute_v2uv(437, mesh["vi"], mesh["vti"])
    assert got.shape == (437, 4) and np.array_equal(got, gold["ref/v2uv"])
    assert np.array_equal(R.compute_v2uv(437, mesh["vi"], mesh["vti"]), gold["ref/v2uv"])
    sf = S.BodySurface.from_arrays(mesh["vi"], mesh["vt"], mesh["vti"], uv_size=48)
    assert np.array_equal(sf.v2uv, gold["ref/v2uv"]) and (sf.V, sf.F, sf.T) == (437, 792, len(mesh["vt"]))


def test_incidence_table_order(mesh):
    vi = np.array([[2, 0, 1], [0, 0, 3], [3, 2, 0], [5, 3, 2]])               # face 1 lists vertex 0 twice; vertex 4 is unused
    ptr, face = S.incidence_table(6, vi)
    assert ptr.tolist() == [0, 4, 5, 8, 11, 11, 12]
    assert face.tolist() == [0, 1, 1, 2, 0, 0, 2, 3, 1, 2, 3, 3]
    ptr, face = S.incidence_table(437, mesh["vi"])
    want_ptr, want_face = R.incidence(437, mesh["vi"])
    assert np.array_equal(ptr, want_ptr) and np.array_equal(face, want_face)
    for v in (0, 200, R.FAN[1] * R.NX + R.FAN[0]):
        mine = face[ptr[v]:ptr[v + 1]]
        assert np.all(np.diff(mine) >= 0) and np.array_equal(np.sort(mine), np.nonzero((mesh["vi"] == v).any(1))[0])


def test_every_rejection_names_the_offending_element(mesh):
    vi, vt, vti = mesh["vi"], mesh["vt"], mesh["vti"]
    build = S.BodySurface.from_arrays
    with pytest.raises(TypeError, match="from_arrays"):
        S.BodySurface()
    bad = vi.copy()
    bad[7, 2] = 437
    with pytest.raises(ValueError, match=r"vi\[7, 2\] = 437 is outside \[0, V=437\)"):
        build(bad, vt, vti, n_verts=437)
    bad[7, 2] = -1
    with pytest.raises(ValueError, match=r"vi\[7, 2\] = -1"):
        build(bad, vt, vti)
    bad = vti.copy()
    bad[3, 1] = len(vt)
    with pytest.raises(ValueError, match=rf"vti\[3, 1\] = {len(vt)} is outside \[0, T={len(vt)}\)"):
        build(vi, vt, bad)
    for value in (np.nan, np.inf):
        bad = vt.copy()
        bad[9, 1] = value
        with pytest.raises(ValueError, match=r"vt\[9, 1\] is not finite"):
            build(vi, bad, vti)
    with pytest.raises(ValueError, match="F=0 faces"):
        build(np.zeros((0, 3), np.int64), vt, np.zeros((0, 3), np.int64), n_verts=437)
    with pytest.raises(ValueError, match="F=792 faces and vti 791"):
        build(vi, vt, vti[:-1])
    for size in (0, -3, _lib.SURFACE_MAX_UV + 1):
        with pytest.raises(ValueError, match=f"uv_size={size} is outside"):
            build(vi, vt, vti, uv_size=size)
    assert 3 * _lib.SURFACE_MAX_UV ** 2 < 2 ** 31
    with pytest.raises(ValueError, match=r"vi must be an integer array \[., 3\]"):
        build(vi.astype(np.float32), vt, vti)
    with pytest.raises(ValueError, match=r"vt must be \[T >= 1, 2\]"):
        build(vi, vt[:, :1], vti)
    # five texture indices at vertex 0; a vertex no face uses
    fan_vi = np.array([[0, 1, 2], [0, 2, 3], [0, 3, 4], [0, 4, 5], [0, 5, 1]])
    fan_vti = np.arange(15).reshape(5, 3)
    with pytest.raises(ValueError, match="vertex 0 owns 5 distinct texture indices"):
        build(fan_vi, np.random.RandomState(0).rand(15, 2), fan_vti)
    with pytest.raises(ValueError, match="vertex 3 is used by no face"):
        build(fan_vi[:1], vt, fan_vti[:1], n_verts=8)
    given = np.zeros((8, 4), np.int64)
    assert build(fan_vi[:1], vt, fan_vti[:1], v2uv=given).V == 8            # a given v2uv keeps unused vertices
    given[5, 3] = len(vt)
    with pytest.raises(ValueError, match=rf"v2uv\[5, 3\] = {len(vt)}"):
        build(fan_vi[:1], vt, fan_vti[:1], v2uv=given)
    with pytest.raises(ValueError, match="v2uv holds 8 vertices; the mesh has V=9"):
        build(fan_vi[:1], vt, fan_vti[:1], n_verts=9, v2uv=np.zeros((8, 4), np.int64))
    # with_images
    sf = build(vi, vt, vti, uv_size=48)
    index, bary = np.full((6, 6, 3), -1, np.int64), np.zeros((6, 6, 3), np.float32)
    other = sf.with_images(index, bary)
    assert other.uv_size == 6 and sf.uv_size == 48 and other.V == 437
    index[2, 4, 1] = 437
    with pytest.raises(ValueError, match=r"index_image\[2, 4, 1\] = 437 is outside \[-1, V=437\)"):
        sf.with_images(index, bary)
    index[2, 4, 1] = -2
    with pytest.raises(ValueError, match=r"index_image\[2, 4, 1\] = -2"):
        sf.with_images(index, bary)
    index[2, 4, 1] = 0
    with pytest.raises(ValueError, match="need the same H"):
        sf.with_images(index, np.zeros((5, 5, 3), np.float32))
    with pytest.raises(ValueError, match=r"integer array \[H, H, 3\]"):
        sf.with_images(index[:, :5], bary[:, :5])


def test_nothing_is_computed_on_the_cpu(mesh):
    sf = S.BodySurface.from_arrays(mesh["vi"], mesh["vt"], mesh["vti"], uv_size=48)
    verts, cam = torch.zeros(2, 437, 3), torch.zeros(1, 3)
    calls = {"normals": lambda x: sf.normals(x), "view_cos": lambda x: sf.view_cos(x, cam),
             "normals_and_view_cos": lambda x: sf.normals_and_view_cos(x, cam), "to_uv": lambda x: sf.to_uv(x),
             "from_uv": lambda x: sf.from_uv(x), "surface_maps": lambda x: S.surface_maps(sf, x)}
    for name, call in calls.items():
        with pytest.raises(_lib.A2PError, match="must be a tensor"):
            call(np.zeros((2, 437, 3), np.float32))
        if name != "surface_maps" or not torch.cuda.is_available():
            with pytest.raises(_lib.A2PError, match="no CPU implementation"):
                call(torch.zeros(2, 4, 8, 8) if name == "from_uv" else verts)
    if not torch.cuda.is_available():
        with pytest.raises(_lib.A2PError, match="no CPU implementation"):
            sf.index_image


def test_the_new_exports_are_bound():
    names = {"a2p_surface_normals", "a2p_surface_to_uv", "a2p_surface_from_uv", "a2p_surface_uv_index"}
    assert names <= set(_lib.EXPORTS)
    src = open(os.path.join(ROOT, "include", "a2p_hip.h")).read()
    for name, val in (("UV", _lib.SURFACE_MAX_UV), ("CHANNELS", _lib.SURFACE_MAX_CHANNELS)):
        assert f"#define A2P_SURFACE_MAX_{name} {val}\n" in src
    import __graft_entry__ as ge
    ge.build()
    for half in (False, True):
        lib = _lib.load(half)
        assert all(hasattr(lib, n) for n in names)
        with pytest.raises(_lib.A2PError, match="surface_to_uv: null argument"):        # argument checks come before any GPU work
            _lib.check(lib.a2p_surface_to_uv(None, 0, 1, 1, None, None, 4, None, None), "a2p_surface_to_uv")


def test_main_rejects_a_geometry_file_without_vertices(tmp_path):
    np.save(tmp_path / "geometry.npy", {"joints": np.zeros((1, 2, 4, 3), np.float32)})
    with pytest.raises(_lib.A2PError, match="holds no `vertices`"):
        S.main(["--geometry", str(tmp_path / "geometry.npy"), "--assets", str(tmp_path / "none.pt"), "--out", str(tmp_path / "o.npy")])
