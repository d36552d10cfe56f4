"""Host side of the anti-aliased rendered images, no GPU: the stored fixture's statements (tests/golden/golden_render_aa_v1.npz), the
properties of the restatement (tests/render_aa_restatement.py), texture.display_to_linear against linear_to_display, every rejection
that comes before a launch, and the declaration and binding of the two exports."""
import os

import numpy as np
import pytest
import torch

import render_aa_restatement as A
import render_restatement as R
from audio2photoreal_amd import _lib
from audio2photoreal_amd import render as RD
from audio2photoreal_amd import texture as T
from conftest import record

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EYE = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)[None]                  # Rt of a camera at the origin looking along +z
K8 = np.array([[[4.0, 0, 4], [0, 4, 4], [0, 0, 1]]])                          # an 8 x 8 image, 90 degrees across


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_render_aa_v1.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def scene():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_render_v1.npz"))
    return {"vi": g["vi"].astype(np.int64), "vt": g["vt"], "vti": g["vti"].astype(np.int64), "verts": g["verts"]}


# ------------------------------------------------------------------------------------------------ the fixture
def test_the_stored_clearances_and_sample_faces_are_reproduced(gold, scene):
    """On its s H x s W grid through K' every frame keeps every sample centre clear of every edge and every winner clear of its
    runner-up by more than the stated multiple of the LARGEST float32 error of the fixture; float32 and float64 agree on every
    sample's face; no sample is excluded."""
    factor = int(gold["clearance_factor"])
    assert factor == R.CLEARANCE_FACTOR and [tuple(f) for f in gold["frames"]] == list(A.FRAMES)
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "golden_render_aa_v1.npz")) < 1 << 20
    for k, (kind, s, H, W) in enumerate(A.FRAMES):
        assert gold[f"tex{k}"].shape == (3, 40, 56) and gold[f"bg{k}"].shape == (3, H, W) and gold[f"face{k}"].shape == (s * H, s * W)
        c = A.clearances(scene["verts"][kind:kind + 1], scene["vi"], gold[f"K{k}"][None], gold[f"Rt{k}"][None], H, W, s)
        for name in ("e_proj", "edge_clearance", "e_depth", "depth_clearance"):
            assert c[name] == pytest.approx(float(gold[name][k]), rel=1e-9), (k, name)
        assert c["edge_clearance"] > factor * gold["e_proj"].max() and c["depth_clearance"] > factor * gold["e_depth"].max()
        face = c["f64"]["face"][0]
        assert c["same_faces"] and np.array_equal(face, gold[f"face{k}"])
        count = A.block_count(face >= 0, s)
        partly, several = int(((count > 0) & (count < s * s)).sum()), int((A.winning_faces(face, s) > 1).sum())
        assert (partly, several, int((face >= 0).sum())) == (int(gold["partly"][k]), int(gold["several"][k]), int(gold["covered"][k]))
        assert partly >= 20 and several >= 0.4 * H * W                        # silhouettes and occlusion edges inside pixels
        record(f"render_aa_fixture{k}", e_proj=c["e_proj"], edge_clearance=c["edge_clearance"], e_depth=c["e_depth"],
               depth_clearance=c["depth_clearance"], partly_covered=partly, several_faces=several, excluded_samples=0)


# ------------------------------------------------------------------------------------------------ the restatement
def test_one_sample_per_axis_is_the_single_sample_image(gold, scene):
    kind, _, H, W = A.FRAMES[0]
    v, K, Rt = scene["verts"][kind:kind + 1], gold["K0"][None], gold["Rt0"][None]
    tex = gold["tex0"][None]
    for dtype in (np.float64, np.float32):
        frag = R.rasterize(v, scene["vi"], K, Rt, H, W, dtype=dtype)
        want = R.sample_texture(tex, scene["vt"], scene["vti"], frag["face"], frag["bary"], dtype=dtype)
        got = A.render_antialiased(v, scene, K, Rt, H, W, 1, tex, dtype=dtype)
        assert got["image"].dtype == dtype and np.array_equal(got["image"], want)
        assert np.array_equal(got["alpha"][:, 0], (frag["face"] >= 0).astype(dtype)) and np.array_equal(got["count"], frag["face"] >= 0)
        attr = A.interpolate_antialiased(v, scene, K, Rt, H, W, 1, v, dtype=dtype)
        assert np.array_equal(attr["image"], R.interpolate(v, scene["vi"], frag["face"], frag["bary"], dtype))
        assert np.array_equal(attr["depth"][:, 0], frag["depth"])
    assert np.array_equal(A.scaled_camera(K, 1), K.astype(np.float32))
    K3 = A.scaled_camera(K, 3)
    assert K3.dtype == np.float32 and np.array_equal(K3[0, :2], K[0, :2].astype(np.float32) * np.float32(3)) and np.array_equal(K3[0, 2], [0, 0, 1])


def test_the_coverage_of_a_triangle_tends_to_its_area():
    """One triangle across most of the 8 x 8 image, no edge along the grid.  The summed coverage is its area measured with (8 s)^2
    samples: a sample can only be wrong about the area of its own 1/s x 1/s cell when an edge crosses that cell, and such cells lie
    within half a cell diagonal of the perimeter P, so |sum of alpha - area| <= P sqrt(2) / s + pi / (2 s^2) (the second term: the
    half-discs around the ends of the edges)."""
    verts = np.array([[[-1.63, -1.79, 2], [1.67, -1.03, 2], [-0.89, 1.81, 2]]])  # projects to (0.74, 0.42), (7.34, 1.94), (2.22, 7.62)
    mesh = {"vi": np.array([[0, 1, 2]]), "vt": np.array([[0.0, 0], [1, 0], [0, 1]]), "vti": np.array([[0, 1, 2]])}
    tex = np.ones((1, 1, 2, 2))
    p = R.project(verts, K8, EYE)[0, :, :2]
    assert np.allclose(p, [[0.74, 0.42], [7.34, 1.94], [2.22, 7.62]], atol=1e-12)
    edge = lambda a, b, x, y: (b[0] - a[0]) * (y - a[1]) - (b[1] - a[1]) * (x - a[0])
    area = 0.5 * abs(edge(p[0], p[1], p[2][0], p[2][1]))
    perimeter = sum(np.linalg.norm(p[k] - p[(k + 1) % 3]) for k in range(3))
    errors, bounds = [], []
    for s in (1, 2, 3, 4):
        got = A.render_antialiased(verts, mesh, K8, EYE, 8, 8, s, tex)
        assert np.array_equal(got["alpha"][0, 0] * s * s, got["count"][0]) and np.allclose(got["image"], got["alpha"], atol=1e-12)
        errors.append(float(abs(got["alpha"].sum() - area)))
        bounds.append(float(perimeter * np.sqrt(2) / s + np.pi / (2 * s * s)))
        # the sample centres in the image's own units, (j + (b + 0.5) / s, i + (a + 0.5) / s), against the triangle seen through K
        x, y = np.meshgrid((np.arange(8 * s) + 0.5) / s, (np.arange(8 * s) + 0.5) / s)
        w = [edge(p[k], p[(k + 1) % 3], x, y) for k in range(3)]
        inside = ((w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0)) | ((w[0] <= 0) & (w[1] <= 0) & (w[2] <= 0))
        assert min(np.abs(wk).min() for wk in w) > 1e-9                       # no sample on an edge: the comparison is exact
        assert np.array_equal(A.sample_fragments(verts, mesh["vi"], K8, EYE, 8, 8, s)["face"][0] >= 0, inside)
    record("render_aa_triangle_area", area=float(area), errors=errors, bounds=bounds)
    assert all(e <= b for e, b in zip(errors, bounds)) and bounds == sorted(bounds, reverse=True)


def test_the_three_way_background_rule():
    s = 2
    samples = np.arange(1.0, 1 + 2 * 2 * 6).reshape(1, 2, 2, 6)               # one row of three pixels, two channels
    covered = np.array([[[True, True, True, False, False, False], [True, True, False, False, False, False]]])
    bg = np.array([[[[np.nan, 100.0, 7.0]], [[np.nan, 200.0, 9.0]]]])          # NaN behind the full pixel: it is not read
    for dtype in (np.float64, np.float32):
        got = A.resolve(samples, covered, s, bg, dtype)
        assert np.array_equal(got["count"][0, 0], [4, 1, 0]) and np.array_equal(got["alpha"][0, 0, 0], np.array([1, 0.25, 0], dtype))
        full = (samples[0, :, 0, 0] + samples[0, :, 0, 1] + samples[0, :, 1, 0] + samples[0, :, 1, 1]) / 4
        part = samples[0, :, 0, 2] / 4 + 0.75 * bg[0, :, 0, 1]
        assert np.array_equal(got["image"][0, :, 0, 0], full.astype(dtype)) and np.array_equal(got["image"][0, :, 0, 1], part.astype(dtype))
        assert np.array_equal(got["image"][0, :, 0, 2], bg[0, :, 0, 2].astype(dtype))
        none = A.resolve(samples, covered, s, None, dtype)
        assert np.array_equal(none["image"][0, :, 0], np.stack([full, samples[0, :, 0, 2] / 4, [0, 0]], 1).astype(dtype))
        colour = A.resolve(samples, covered, s, np.array([3.0, 5.0]), dtype)  # a colour [C]
        assert np.array_equal(colour["image"][0, :, 0, 2], [3, 5]) and np.array_equal(colour["image"][0, :, 0, 0], full.astype(dtype))
    assert np.array_equal(A.block_mean(samples * covered[:, None], s), none["image"]) and np.array_equal(A.block_count(covered, s), none["count"])


# ------------------------------------------------------------------------------------------------ the display curve
def test_display_to_linear_inverts_linear_to_display():
    """Every integer display value 0..255 in every channel: linear_to_display(display_to_linear(d)) against d.  Below half a code
    value the composite of an uncovered pixel would round to the given byte anyway; the final select makes even that irrelevant."""
    d = torch.arange(256, dtype=torch.float32).reshape(1, 256, 1).expand(3, 256, 1).contiguous()
    linear = T.display_to_linear(d)
    assert linear.shape == d.shape and linear.dtype == torch.float32 and bool(torch.isfinite(linear).all())
    assert bool((linear[:, 1:] > linear[:, :-1]).all())                       # increasing in every channel
    back = T.linear_to_display(linear)
    worst = float((back - d).abs().max())
    record("render_aa_display_roundtrip", max_deviation=worst, allowance=0.5)
    assert worst < 0.5
    assert torch.equal(back.round(), d)
    batch = T.display_to_linear(d[None].expand(2, -1, -1, -1))                # leading axes are carried
    assert torch.equal(batch[1], linear)
    with pytest.raises(_lib.A2PError, match=r"\[.., 3, H, W\]"):
        T.display_to_linear(torch.zeros(4, 5))
    shown, lin = T.display_background([10, 20, 250], 4, 5)
    assert shown.shape == (3, 1, 1) and lin.shape == (3,) and torch.equal(lin, T.display_to_linear(shown).reshape(3))
    panel = np.random.RandomState(3).uniform(0, 255, (4, 5, 3)).astype(np.float32)
    shown, lin = T.display_background(panel, 4, 5)
    assert shown.shape == (3, 4, 5) and lin.shape == (1, 3, 4, 5) and np.array_equal(shown.numpy(), panel.transpose(2, 0, 1))
    assert torch.equal(T.display_background(torch.from_numpy(panel.transpose(2, 0, 1).copy()), 4, 5)[0], shown)
    assert T.display_background(None, 4, 5) == (None, None)
    for bad, match in (([1, 2], "three numbers"), (np.zeros((5, 4, 3)), "three numbers"), ([0, 0, 256], r"\[0, 255\]"), ([0, -1, 0], r"\[0, 255\]"),
                       ([0, float("nan"), 0], r"\[0, 255\]"), ("red", "three numbers")):
        with pytest.raises(ValueError, match=match):
            T.display_background(bad, 4, 5)


# ------------------------------------------------------------------------------------------------ host validation
def test_every_rejection_comes_before_a_launch(scene):
    build = RD.BodyRasterizer.from_arrays
    rast = build(scene["vi"], scene["vt"], scene["vti"], 8, 9)
    verts, K, Rt, tex = torch.zeros(2, 874, 3), torch.zeros(1, 3, 3), torch.zeros(1, 3, 4), torch.zeros(1, 3, 4, 4)
    for s in (0, 5, -1, 2.5):
        with pytest.raises(ValueError, match="supersample="):
            rast.render_antialiased(verts, tex, K, Rt, supersample=s)
        with pytest.raises(ValueError, match="supersample="):
            rast.interpolate_antialiased(verts, verts, K, Rt, supersample=s)
        with pytest.raises(ValueError, match="supersample="):
            RD.render_motion(rast, None, verts, K, Rt, supersample=s)
    big = build(scene["vi"], scene["vt"], scene["vti"], _lib.RENDER_MAX_SIZE // 2 + 1, 8)
    with pytest.raises(ValueError, match=f"height={_lib.RENDER_MAX_SIZE // 2 + 1} exceeds {_lib.RENDER_MAX_SIZE}"):
        big.render_antialiased(verts, tex, K, Rt, supersample=2)
    wide = build(scene["vi"], scene["vt"], scene["vti"], 8, _lib.RENDER_MAX_SIZE // 4 + 1)
    with pytest.raises(ValueError, match="width="):
        wide.interpolate_antialiased(verts, verts, K, Rt, supersample=4)
    for bad in (torch.zeros(4), torch.zeros(1, 3, 8, 8), torch.zeros(3, 3, 8, 9), torch.zeros(3, 8, 9), torch.zeros(3, dtype=torch.float64)):
        with pytest.raises(_lib.A2PError, match=r"background must be float32 \[3\] or \[2 or 1, 3, 8, 9\]"):
            rast.render_antialiased(verts, tex, K, Rt, background=bad)
    with pytest.raises(_lib.A2PError, match="background must be None or a tensor"):
        rast.render_antialiased(verts, tex, K, Rt, background=[0.0, 0.0, 0.0])
    with pytest.raises(_lib.A2PError, match="background is on meta, verts on cpu"):
        rast.render_antialiased(verts, tex, K, Rt, background=torch.zeros(3, device="meta"))
    # a well-formed call gets as far as the refusal to compute on the CPU, like every other method
    for call in (lambda: rast.render_antialiased(verts, tex, K, Rt, background=torch.zeros(3)),
                 lambda: rast.interpolate_antialiased(verts, verts, K, Rt, supersample=3)):
        with pytest.raises(_lib.A2PError, match="no CPU implementation"):
            call()
    with pytest.raises(_lib.A2PError, match="must be a tensor"):
        rast.render_antialiased(np.zeros((2, 874, 3), np.float32), tex, K, Rt)
    with pytest.raises(_lib.A2PError, match="background and output_filters must be None"):
        rast.render(verts, tex, K, Rt, background=torch.zeros(3))                # render itself is unchanged
    assert RD.parser().parse_args(["--geometry", "g", "--assets", "a", "--out", "o"]).supersample == 1
    assert RD.parser().parse_args(["--geometry", "g", "--assets", "a", "--out", "o", "--supersample", "3"]).supersample == 3
    with pytest.raises(SystemExit):
        RD.parser().parse_args(["--geometry", "g", "--assets", "a", "--out", "o", "--supersample", "5"])


def test_the_new_exports_are_declared_and_bound():
    names = ("a2p_render_antialiased_texture", "a2p_render_antialiased_values")
    assert set(names) <= set(_lib.EXPORTS)
    src = open(os.path.join(ROOT, "include", "a2p_hip.h")).read()
    assert f"#define A2P_RENDER_MAX_SUPERSAMPLE {_lib.RENDER_MAX_SUPERSAMPLE}\n" in src and _lib.RENDER_MAX_SUPERSAMPLE == A.MAX_SUPERSAMPLE
    assert all(f"int {n}(" in src for n in names)
    import __graft_entry__ as ge
    ge.build()
    for half in (False, True):
        lib = _lib.load(half)
        assert all(hasattr(lib, n) for n in names)
        tex = lambda *a: _lib.check(lib.a2p_render_antialiased_texture(*a), "a2p_render_antialiased_texture")
        val = lambda *a: _lib.check(lib.a2p_render_antialiased_values(*a), "a2p_render_antialiased_values")
        # argument checks come before any GPU work: nulls first
        with pytest.raises(_lib.A2PError, match="render_antialiased_texture: null argument"):
            tex(None, 0, 1, None, 1, None, 1, None, None, 0, None, 0, 4, 4, 2, 1e-3, None, 0, 3, 4, 4, 0, None, 0, None, None, None, None, None)
        with pytest.raises(_lib.A2PError, match="render_antialiased_values: null argument"):
            val(None, 0, 1, None, 1, None, 0, None, 0, 4, 4, 2, 1e-3, None, 3, None, 0, None, None, None, None, None, None)
        # ... then the sizes, with pointers that are never followed (N = 0 would return before a launch anyway)
        p = [0x1000 * (k + 1) for k in range(12)]
        for S, H, W, match in ((0, 4, 4, "need 1 <= S <= 4"), (5, 4, 4, "need 1 <= S <= 4"), (2, _lib.RENDER_MAX_SIZE // 2 + 1, 4, "S H, S W <= 8192"),
                               (4, 4, _lib.RENDER_MAX_SIZE // 4 + 1, "S H, S W <= 8192"), (1, 0, 4, "need 1 <= H, W")):
            with pytest.raises(_lib.A2PError, match=match):
                tex(p[0], 0, 1, p[1], 1, p[2], 1, p[3], p[4], 0, p[5], 0, H, W, S, 1e-3, p[6], 0, 3, 4, 4, 0, None, 0, p[7], p[8], p[9], p[10], None)
            with pytest.raises(_lib.A2PError, match=match):
                val(p[0], 0, 1, p[1], 1, p[4], 0, p[5], 0, H, W, S, 1e-3, p[6], 3, None, 0, p[7], p[8], p[9], p[10], None, None)
        with pytest.raises(_lib.A2PError, match=r"C=17 outside \[1, 16\]"):
            val(p[0], 0, 1, p[1], 1, p[4], 0, p[5], 0, 4, 4, 2, 1e-3, p[6], 17, None, 0, p[7], p[8], p[9], p[10], None, None)
        with pytest.raises(_lib.A2PError, match="must not alias an input"):
            val(p[0], 0, 1, p[1], 1, p[4], 0, p[5], 0, 4, 4, 2, 1e-3, p[6], 3, None, 0, p[7], p[8], p[6], p[10], None, None)
        assert val(p[0], 0, 1, p[1], 1, p[4], 0, p[5], 0, 4, 4, 2, 1e-3, p[6], 3, None, 0, p[7], p[8], p[9], p[10], p[11], None) == 0   # N = 0
