"""Several bodies in one image on the MI355X (csrc/kernels_scene.h, audio2photoreal_amd/scene.py) against the float64 restatement
(tests/scene_restatement.py) on the fixture tests/golden/golden_scene_v1.npz: the two-layer scene of golden_render_v1 with a second,
placed body crossing it, through five cameras that keep every SAMPLE centre of the merged scene clear of every edge and every winner
clear of its runner-up by 8 x the float32 error (tests/golden/make_golden_scene.py).

Gate: coverage is compared exactly (counts with array_equal, alpha and body_alpha bit for bit), no pixel excluded.  The normalised
error of every float output (max |difference| / max |value|) is at most 4 x the error of the float32 restatement against the float64
one on the same input, the rule of tests/test_render_hip.py and tests/test_render_aa_hip.py; the factor 4 pays for the device's fused
multiply-adds and division.  Exact branches (one body against BodyRasterizer.render_antialiased, None against the identity, body
order, disjoint footprints, uncovered and fully covered pixels, call shapes, chunking, streams) are compared with ==.  Every measured
value goes to record(...) beside its allowance under scene_* names."""
import json
import os

import numpy as np
import pytest
import torch

import body_chain_restatement as B
import encoder_restatement as ER
import render_aa_restatement as A
import render_restatement as R
import scene_restatement as SC
import skinning_restatement as SR
import texture_restatement as TR
from audio2photoreal_amd import _lib
from audio2photoreal_amd import decoder as D
from audio2photoreal_amd import encoder as E
from audio2photoreal_amd import render as RD
from audio2photoreal_amd import scene as SN
from audio2photoreal_amd import texture as T
from audio2photoreal_amd import video as VD
from audio2photoreal_amd._lib import A2PError
from conftest import record
from test_render_codes_hip import ENC_UV, body, nets, scene  # noqa: F401  (body, scene: fixtures, the smallest synthetic assets)
from test_render_hip import guarded

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V0, V1 = 874, 437


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_scene_v1.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def bodies():
    return SC.fixture_bodies()[0]


@pytest.fixture(scope="module")
def want(gold, bodies):
    """Per fixture frame: its inputs and the restatement's sample fragments in float64 and float32, computed once and not changed."""
    verts = SC.fixture_bodies()[1]
    out = []
    for k, (kind, s, H, W) in enumerate(SC.FRAMES):
        f = {"verts": [v[kind:kind + 1] for v in verts], "K": gold[f"K{k}"][None], "Rt": gold[f"Rt{k}"][None], "M": gold[f"M{k}"], "s": s, "H": H,
             "W": W, "tex": [gold[f"tex{k}_0"][None], gold[f"tex{k}_1"][None]], "bg": gold[f"bg{k}"][None]}
        args = (bodies, f["verts"], [None, f["M"]], f["K"], f["Rt"], H, W, s)
        f["f64"], f["f32"] = SC.sample_fragments(*args), SC.sample_fragments(*args, dtype=np.float32)
        assert np.array_equal(f["f64"]["face"][0], gold[f"face{k}"]) and np.array_equal(f["f32"]["face"], f["f64"]["face"])
        f["count"] = A.block_count(f["f64"]["face"] >= 0, s)
        f["body_count"] = np.stack([A.block_count(f["f64"]["body"] == p, s) for p in range(2)], 1)
        out.append(f)
    return out


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def ups(xs, dev):
    return [None if x is None else up(x, dev) for x in xs]


def gate(name, got, ref, allowance):
    """Record and assert one output: got (device tensor or array) against ref (float64) within `allowance` (normalised)."""
    err = R.nerr(got.cpu().numpy() if torch.is_tensor(got) else got, ref)
    record(name, err=err, allowance=float(allowance))
    assert np.isfinite(err) and err <= allowance, (name, err, allowance)


def rasterizer(bodies, H, W, flips=(False, False)):
    return SN.SceneRasterizer([((b["vi"], b["vt"], b["vti"], b["n_verts"]), bool(f)) for b, f in zip(bodies, flips)], H, W)


def run(sc, f, dev, tex=None, background=None, placements="fixture", **kw):
    placements = [None, f["M"]] if isinstance(placements, str) else placements
    return sc.render(ups(f["verts"], dev), ups(f["tex"] if tex is None else tex, dev), up(f["K"], dev), up(f["Rt"], dev), ups(placements, dev),
                     supersample=f["s"], background=None if background is None else up(background, dev), **kw)


def same(a: dict, b: dict):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def references(f, bodies, tex, flips, bg):
    """(float64 reference, float32 reference) of one fixture frame."""
    args = (bodies, f["verts"], tex, f["K"], f["Rt"], f["H"], f["W"], f["s"], [None, f["M"]], flips, bg)
    return SC.render(*args, fragments=f["f64"]), SC.render(*args, dtype=np.float32, fragments=f["f32"])


# ------------------------------------------------------------------------------------------------ 1: coverage
def test_fixture_coverage_is_exact(dev, bodies, want):
    for k, f in enumerate(want):
        s, H, W = f["s"], f["H"], f["W"]
        out = run(rasterizer(bodies, H, W), f, dev)
        assert set(out) == {"render", "alpha", "depth", "body_alpha"} and all(x.dtype == torch.float32 for x in out.values())
        assert out["render"].shape == (1, 3, H, W) and out["alpha"].shape == out["depth"].shape == (1, 1, H, W) and out["body_alpha"].shape == (1, 2, H, W)
        alpha, share = out["alpha"].cpu().numpy()[:, 0], out["body_alpha"].cpu().numpy()
        got = np.rint(alpha.astype(np.float64) * s * s).astype(np.int64)
        got_p = np.rint(share.astype(np.float64) * s * s).astype(np.int64)
        both = int(((f["body_count"][:, 0] > 0) & (f["body_count"][:, 1] > 0)).sum())
        partly = int(((f["count"] > 0) & (f["count"] < s * s)).sum())
        record(f"scene_coverage{k}", differing_pixels=int((got != f["count"]).sum()), differing_body_pixels=int((got_p != f["body_count"]).any(1).sum()),
               excluded_pixels=0, partly_covered=partly, both_bodies=both)
        assert np.array_equal(got, f["count"]) and np.array_equal(got_p, f["body_count"]) and np.array_equal(got_p.sum(1), got)
        assert s == 1 or (partly >= 20 and both >= 20)
        assert np.array_equal(alpha, f["count"].astype(np.float32) / np.float32(s * s))      # the bits of (float)n / (float)(s s)
        assert np.array_equal(share, f["body_count"].astype(np.float32) / np.float32(s * s))


# ------------------------------------------------------------------------------------------------ 2: colours and depth
@pytest.mark.parametrize("flips", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("C", [1, 3, 16])
def test_fixture_colours_and_depth(dev, bodies, want, C, flips):
    rs = np.random.RandomState(200 + C)
    for k, f in enumerate(want):
        s, H, W = f["s"], f["H"], f["W"]
        tex = f["tex"] if C == 3 else [rs.randn(1, C, *size).astype(np.float32) for size in SC.TEX_SIZES]
        bg = f["bg"] if C == 3 else rs.randn(1, C, H, W).astype(np.float32)
        sc = rasterizer(bodies, H, W, flips)
        plain, over = run(sc, f, dev, tex), run(sc, f, dev, tex, bg)
        tag = f"{k}_C{C}_flip{int(flips[0])}{int(flips[1])}"
        for name, got, back in (("plain", plain, None), ("over", over, bg)):
            ref, ref32 = references(f, bodies, tex, flips, back)
            gate(f"scene_colour{tag}_{name}", got["render"], ref["image"], 4 * R.nerr(ref32["image"], ref["image"]))
            if name == "plain" and flips == (False, False):
                gate(f"scene_depth{k}_C{C}", got["depth"], ref["depth"], 4 * R.nerr(ref32["depth"], ref["depth"]))
        assert all(torch.equal(plain[n], over[n]) for n in ("alpha", "depth", "body_alpha"))
        none, full = (plain["alpha"] == 0).expand(-1, C, -1, -1), (plain["alpha"] == 1).expand(-1, C, -1, -1)
        assert bool(none.any()) and bool(full.any())
        assert bool((plain["render"][none] == 0).all()) and bool((plain["depth"][plain["alpha"] == 0] == 0).all())
        assert torch.equal(over["render"][none], up(bg, dev)[none])           # an uncovered pixel holds the background's bits
        holed = bg.copy()
        holed[np.broadcast_to(f["count"][:, None] == s * s, holed.shape)] = np.nan
        again = run(sc, f, dev, tex, holed)                                    # a fully covered pixel does not read the background
        assert torch.equal(again["render"], over["render"]) and torch.equal(over["render"][full], plain["render"][full])


# ------------------------------------------------------------------------------------------------ 3: one body is today's renderer
@pytest.mark.parametrize("flip", [False, True])
def test_one_body_without_placement_is_render_antialiased_bit_for_bit(dev, bodies, want, flip):
    seen = set()
    for k, f in enumerate(want):
        s, H, W = f["s"], f["H"], f["W"]
        seen.add(s)
        b = bodies[0]
        old = RD.BodyRasterizer.from_arrays(b["vi"], b["vt"], b["vti"], H, W, n_verts=V0, flip_uv=flip)
        for made in (SN.SceneRasterizer([(old, flip)], H, W), SN.SceneRasterizer([{"body": (b["vi"], b["vt"], b["vti"], V0), "flip_uv": flip}], H, W)):
            for bg in (None, up(f["bg"], dev), up(f["bg"][0, :, 0, 0].copy(), dev)):
                verts, tex, K, Rt = up(f["verts"][0], dev), up(f["tex"][0], dev), up(f["K"], dev), up(f["Rt"], dev)
                got = made.render([verts], [tex], K, Rt, supersample=s, background=bg)
                ref = old.render_antialiased(verts, tex, K, Rt, supersample=s, background=bg)
                assert torch.equal(got["render"], ref["render"]) and torch.equal(got["alpha"], ref["alpha"]), (k, s)
                assert torch.equal(got["body_alpha"], got["alpha"])
                assert bool(((ref["alpha"] > 0) & (ref["alpha"] < 1)).any()) or s == 1
    assert seen == {1, 2, 3, 4}


# ------------------------------------------------------------------------------------------------ 4: placement, order, footprints
def test_none_is_the_identity_and_the_body_order_does_not_matter(dev, bodies, want):
    eye = np.eye(3, 4, dtype=np.float32)
    for k, f in enumerate(want):
        s, H, W = f["s"], f["H"], f["W"]
        sc = rasterizer(bodies, H, W, (True, False))
        base = run(sc, f, dev, background=f["bg"])
        assert same(base, run(sc, f, dev, background=f["bg"], placements=[eye, f["M"]]))
        assert same(base, run(sc, f, dev, background=f["bg"], placements=[eye[None], f["M"][None]]))
        # body 1 first: the same image, coverage and depth (the fixture has no depth ties), the shares swapped
        back = rasterizer(bodies[::-1], H, W, (False, True))
        g = {**f, "verts": f["verts"][::-1], "tex": f["tex"][::-1]}
        swapped = run(back, g, dev, background=f["bg"], placements=[f["M"], None])
        assert all(torch.equal(swapped[n], base[n]) for n in ("render", "alpha", "depth")), k
        assert torch.equal(swapped["body_alpha"], base["body_alpha"].flip(1))
        assert bool((base["body_alpha"][:, 0] > 0).any()) and bool((base["body_alpha"][:, 1] > 0).any())


def disjoint_scene():
    """A 20 x 48 camera at 3 samples per axis that sees the fixture's two-layer body on its left and body 1, moved 2.9 to the right,
    on its right, with empty columns between them."""
    K, Rt = R.look_at([2.55, 0.9, 5.6], [2.55, 0.9, -0.2], [0, 1, 0], 20, 48, 24.0, np.float32)
    M = SC.placement(0.0, (2.9, 0.0, 0.0), (0, 1, 0)).astype(np.float32)
    return K[None], Rt[None], M, 20, 48, 3


def test_bodies_with_disjoint_footprints_render_as_they_do_alone(dev, bodies):
    K, Rt, M, H, W, s = disjoint_scene()
    rs = np.random.RandomState(31)
    verts = [v[1:2] for v in SC.fixture_bodies()[1]]
    tex = [rs.randn(1, 3, *size).astype(np.float32) for size in SC.TEX_SIZES]
    bg = rs.randn(1, 3, H, W).astype(np.float32)
    f = {"verts": verts, "tex": tex, "K": K, "Rt": Rt, "M": M, "s": s}
    both = run(rasterizer(bodies, H, W, (False, True)), f, dev, background=bg)
    b = bodies[0]
    first = RD.BodyRasterizer.from_arrays(b["vi"], b["vt"], b["vti"], H, W, n_verts=V0).render_antialiased(
        up(verts[0], dev), up(tex[0], dev), up(K, dev), up(Rt, dev), supersample=s, background=up(bg, dev))
    second = run(rasterizer(bodies[1:], H, W, (True,)), {**f, "verts": verts[1:], "tex": tex[1:]}, dev, background=bg, placements=[M])
    mine, yours = both["body_alpha"][:, :1] > 0, both["body_alpha"][:, 1:] > 0
    record("scene_disjoint", body0_pixels=int(mine.sum()), body1_pixels=int(yours.sum()), shared_pixels=int((mine & yours).sum()))
    assert int(mine.sum()) >= 50 and int(yours.sum()) >= 50 and not bool((mine & yours).any())
    assert torch.equal(both["alpha"], first["alpha"] + second["alpha"])
    for n in ("render", "alpha"):
        c = both[n].shape[1]
        assert torch.equal(both[n][mine.expand(-1, c, -1, -1)], first[n][mine.expand(-1, c, -1, -1)])
        assert torch.equal(both[n][yours.expand(-1, c, -1, -1)], second[n][yours.expand(-1, c, -1, -1)])
    assert torch.equal(both["depth"][yours], second["depth"][yours]) and torch.equal(both["body_alpha"][:, 1:], second["body_alpha"])
    nobody = ~(mine | yours)
    assert torch.equal(both["render"][nobody.expand(-1, 3, -1, -1)], up(bg, dev)[nobody.expand(-1, 3, -1, -1)])


# ------------------------------------------------------------------------------------------------ 5: call shapes
@pytest.fixture(scope="module")
def seven(dev, want):
    """7 frames of the fixture's frame 0 (s = 2, 24 x 32) with a camera, textures, a placement and a background each."""
    rs = np.random.RandomState(71)
    f = want[0]
    n = 7
    verts = [np.repeat(v, n, 0) + rs.randn(n, 1, 3).astype(np.float32) * 0.02 for v in f["verts"]]
    Rt = np.repeat(f["Rt"], n, 0)
    Rt[:, :, 3] += rs.randn(n, 3).astype(np.float32) * 0.03
    K = np.repeat(f["K"], n, 0)
    K[:, 0, 0] *= (1 + rs.rand(n).astype(np.float32) * 0.1)
    M = np.stack([SC.placement(35.0 + 3 * rs.randn(), (0.05, 0.03, -0.22) + 0.05 * rs.randn(3), (0, 1, 0), (1.1, 0.9, 0.0)) for _ in range(n)]).astype(np.float32)
    return {"verts": ups(verts, dev), "K": up(K, dev), "Rt": up(Rt, dev), "M": up(M, dev),
            "tex": [up(rs.randn(n, 3, *size).astype(np.float32), dev) for size in SC.TEX_SIZES], "bg": up(rs.randn(n, 3, f["H"], f["W"]).astype(np.float32), dev)}


def run_seven(sc, n, lo=0, hi=7, s=2, **kw):
    return sc.render([v[lo:hi] for v in n["verts"]], [t[lo:hi] for t in n["tex"]], n["K"][lo:hi], n["Rt"][lo:hi], [None, n["M"][lo:hi]], supersample=s,
                     background=n["bg"][lo:hi], **kw)


@pytest.mark.parametrize("s", [2, 3])
def test_a_frames_bits_do_not_depend_on_the_call(dev, bodies, seven, s):
    H, W = 24, 32
    sc = rasterizer(bodies, H, W)
    full = run_seven(sc, seven, s=s)
    assert full["render"].shape == (7, 3, H, W) and full["body_alpha"].shape == (7, 2, H, W)
    assert len({float(full["body_alpha"][n, 1].sum()) for n in range(7)}) > 3   # the frames do differ
    assert same(full, run_seven(sc, seven, s=s)), "two identical runs differ"
    for lo, hi in ((0, 1), (2, 4), (6, 7)):
        alone = run_seven(sc, seven, lo, hi, s=s)
        assert all(torch.equal(alone[k], full[k][lo:hi]) for k in full), (lo, hi)
    per = sc.scratch_bytes_per_frame(s)
    assert per == 12 * (V0 + V1) + 8 * s * s * H * W
    assert same(full, run_seven(sc, seven, s=s, max_bytes=1))                  # one frame per chunk
    assert same(full, run_seven(sc, seven, s=s, max_bytes=3 * per + 5))        # three per chunk: 3 + 3 + 1
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        got = run_seven(rasterizer(bodies, H, W), seven, s=s)
    side.synchronize()
    assert same(full, got)
    # one texture, placement, camera and background for all frames: shared ([1, ..] or without the axis) against repeated
    n = seven
    shared = lambda tex, M, K, Rt, bg: sc.render(n["verts"], tex, K, Rt, [None, M], supersample=s, background=bg)
    tex1, M1, K1, Rt1, bg1 = [t[3:4] for t in n["tex"]], n["M"][3:4], n["K"][3:4], n["Rt"][3:4], n["bg"][3:4]
    one = shared(tex1, M1, K1, Rt1, bg1)
    rep = lambda x: x.repeat(7, *([1] * (x.dim() - 1)))
    assert same(one, shared([rep(t) for t in tex1], rep(M1), rep(K1), rep(Rt1), rep(bg1)))
    assert same(one, shared([tex1[0], rep(tex1[1])], M1[0], K1[0], rep(Rt1), bg1))
    assert torch.equal(one["render"][3], full["render"][3]) and not torch.equal(one["render"][2], full["render"][2])
    empty = sc.render([v[:0] for v in n["verts"]], tex1, K1, Rt1, supersample=s)
    assert empty["render"].shape == (0, 3, H, W) and empty["body_alpha"].shape == (0, 2, H, W)


def test_render_refuses_malformed_tensors(dev, bodies):
    sc = rasterizer(bodies, 6, 8)
    z = lambda *shape, **kw: torch.zeros(*shape, device=dev, **kw)
    good = dict(verts=[z(2, V0, 3), z(2, V1, 3)], textures=[z(1, 3, 4, 4), z(2, 3, 5, 6)], K=z(3, 3), Rt=z(1, 3, 4))
    for kw, match in ((dict(verts=[z(2, V0, 3), z(3, V1, 3)]), r"verts\[1\] must be float32 \[2, 437, 3\]"),
                      (dict(verts=[z(2, V1, 3), z(2, V1, 3)]), r"verts\[0\] must be float32 \[2, 874, 3\]"),
                      (dict(verts=[z(2, V0, 3, dtype=torch.float64), z(2, V1, 3)]), r"verts\[0\] must be float32"),
                      (dict(textures=[z(1, 3, 4, 4), z(1, 2, 5, 6)]), r"textures\[1\] must be float32 \[2 or 1, 3, Ht, Wt\]"),
                      (dict(textures=[z(1, 17, 4, 4), z(1, 17, 5, 6)]), r"textures\[0\] must be float32"),
                      (dict(textures=[z(3, 3, 4, 4), z(1, 3, 5, 6)]), r"textures\[0\] must be float32 \[2 or 1"),
                      (dict(textures=[z(1, 3, 4, 4).cpu(), z(1, 3, 5, 6)]), r"textures\[0\] must live on the MI355X"),
                      (dict(placements=[None, z(4, 4)]), r"placements\[1\] must be float32 \[2 or 1, 3, 4\]"),
                      (dict(placements=[z(3, 3, 4), None]), r"placements\[0\] must be float32 \[2 or 1, 3, 4\]"),
                      (dict(placements=[None, np.eye(3, 4, dtype=np.float32)]), r"placements\[1\] must be a tensor"),
                      (dict(K=z(2, 2)), "K must be float32"), (dict(Rt=z(5, 3, 4)), "Rt must be float32"),
                      (dict(background=z(2)), "background must be float32"), (dict(background=[0.0, 0.0, 0.0]), "background must be None or a tensor")):
        with pytest.raises(A2PError, match=match):
            sc.render(**{**good, **kw})
    with pytest.raises(ValueError, match="exceeds 8192"):
        SN.SceneRasterizer([(bodies[1]["vi"], bodies[1]["vt"], bodies[1]["vti"])], 4096, 8).render(good["verts"][1:], good["textures"][1:], good["K"], good["Rt"],
                                                                                                  supersample=3)


# ------------------------------------------------------------------------------------------------ 6: four bodies through the C ABI
def four_bodies(seed=15):
    """Four 12-vertex, 4-face bodies (the ABI-level mesh of tests/test_render_aa_hip.py: vi = arange(12) in threes) on a 6 x 8 image at
    4 samples per axis, around z = 2 + 0.1 p.  Pixel (row 1, column 2 p + 1) holds the LAST face of body p in its left half and the
    FIRST face of body p + 1 in its right half, so every boundary of the global face numbering is decided inside one pixel; the
    other faces are larger, slightly tilted triangles in rows 3 to 5, one 0.03 behind and one 0.03 in front of the body's depth,
    where a nearer body hides part of the one behind it (no two faces intersect)."""
    f, cx, cy = 10.0, 4.0, 3.0
    K = np.array([[[f, 0, cx], [0, f, cy], [0, 0, 1]]], np.float32)
    Rt = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)[None].astype(np.float32)
    rs = np.random.RandomState(seed)
    verts, meshes = [], []
    vi = np.arange(12).reshape(4, 3)
    for p in range(4):
        z = 2.0 + 0.1 * p
        left = lambda j: [(j + 0.031, 1.043), (j + 0.473, 1.067), (j + 0.057, 1.957)]         # the left half of pixel (1, j)
        right = lambda j: [(j + 0.527, 1.933), (j + 0.969, 1.041), (j + 0.947, 1.961)]        # the right half
        big = lambda a: [(a + 0.13, 3.07), (a + 2.71, 3.29), (a + 1.03, 5.83)]
        first = right(2 * p - 1) if p > 0 else big(4.6)
        last = left(2 * p + 1) if p < 3 else big(5.1)
        uv = np.array(first + big(0.4 + 1.3 * p) + big(1.1 + 0.9 * p)[::-1] + last) + rs.uniform(-0.01, 0.01, (12, 2))
        zs = np.full((12, 1), z)
        zs[3:9, 0] += np.repeat([0.03, -0.03], 3) + rs.uniform(-0.01, 0.01, 6)
        pts = np.concatenate([(uv[:, :1] - cx) * zs / f, (uv[:, 1:] - cy) * zs / f, zs], 1)
        verts.append(pts.astype(np.float32)[None])
        meshes.append({"vi": vi, "vt": rs.rand(7 + p, 2).astype(np.float32), "vti": rs.randint(0, 7 + p, (4, 3)), "n_verts": 12})
    tex = [rs.randn(1, 2, 3 + p, 6 - p).astype(np.float32) for p in range(4)]
    return meshes, verts, tex, K, Rt, 6, 8, 4


def test_four_bodies_canaries_and_refusals_through_the_c_abi(dev):
    meshes, verts, tex, K, Rt, H, W, s = four_bodies()
    C, P, flips = 2, 4, [False, True, True, False]
    assert R.edge_clearance(SC.world_verts(verts), SC.merged_mesh(meshes)["vi"], A.scaled_camera(K, s), Rt, s * H, s * W) > 1e-3
    bg = np.random.RandomState(13).randn(2, C, H, W).astype(np.float32)
    ref = SC.render(meshes, verts, tex, K, Rt, H, W, s, flips=flips, background=bg[:1])
    ref32 = SC.render(meshes, verts, tex, K, Rt, H, W, s, flips=flips, background=bg[:1], dtype=np.float32)
    f64 = SC.sample_fragments(meshes, verts, None, K, Rt, H, W, s, runner_up=True)
    assert np.array_equal(ref32["body_count"], ref["body_count"]) and R.depth_clearance(f64) > 1e-3
    for p in range(3):                                                         # the last face of body p and the first of body p + 1 in one pixel
        block = f64["face"][0, s:2 * s, s * (2 * p + 1):s * (2 * p + 2)]
        assert (block == 4 * p + 3).sum() >= 2 and (block == 4 * p + 4).sum() >= 2, (p, block)
    assert (ref["body_count"] > 0).any(axis=(0, 2, 3)).all() and ((ref["body_count"] > 0).sum(1) > 1).sum() >= 6
    nan = float("nan")
    frames = [np.concatenate([v, np.full_like(v, np.nan)]) for v in verts]     # frame 1: NaN vertices, nothing is covered
    out, out_all = guarded(dev, (2, C, H, W), torch.float32, nan)
    alpha, alpha_all = guarded(dev, (2, 1, H, W), torch.float32, nan)
    depth, depth_all = guarded(dev, (2, 1, H, W), torch.float32, nan)
    share, share_all = guarded(dev, (2, P, H, W), torch.float32, nan)
    proj, proj_all = guarded(dev, (2, 48, 3), torch.float32, nan)
    key, key_all = guarded(dev, (2, s * H, s * W), torch.int64, -7)
    t = {"verts": ups(frames, dev), "tex": ups(tex, dev), "vt": [up(m["vt"], dev) for m in meshes], "vti": [up(m["vti"].astype(np.int32), dev) for m in meshes],
         "faces": up(SC.merged_mesh(meshes)["vi"].astype(np.int32), dev), "K": up(K, dev), "Rt": up(Rt, dev), "bg": up(bg, dev)}
    lib, p_, stream = _lib.load(), _lib.ptr, _lib.current_stream(dev)

    def desc(**kw):
        arr = (_lib.A2PSceneBody * P)()
        for p in range(P):
            arr[p] = _lib.A2PSceneBody(p_(t["verts"][p]), None, p_(t["tex"][p]), p_(t["vt"][p]), p_(t["vti"][p]), 12, 4, 7 + p, 3 + p, 6 - p, int(flips[p]), 0, 0)
            for name, value in kw.items():
                setattr(arr[p], name, value)
        return arr

    def call(b=None, P=P, S=s, H=H, W=W, C=C, N=2, out=out, depth=depth, share=share, key=key, faces=t["faces"]):
        return lib.a2p_scene_render(desc() if b is None else b, P, p_(faces), N, p_(t["K"]), 0, p_(t["Rt"]), 0, H, W, S, 1e-3, C, p_(t["bg"]), 1, p_(proj),
                                    p_(key), p_(out), p_(alpha), p_(depth), p_(share), stream)

    # refusals first: each returns A2P_ERR_ARG with a message, and nothing has been launched when they are done
    for kw, match in ((dict(S=0), "need 1 <= S <= 4"), (dict(S=5), "need 1 <= S <= 4"), (dict(P=0), "need 1 <= P <= 4"), (dict(P=5), "need 1 <= P <= 4"),
                      (dict(H=0), "need 1 <= H, W"), (dict(S=4, H=_lib.RENDER_MAX_SIZE // 4 + 1), "S H, S W <= 8192"), (dict(C=17), r"C=17 outside \[1, 16\]"),
                      (dict(out=None), "null argument"), (dict(share=None), "null argument"), (dict(b=desc(tex=None)), "body 0: null argument"),
                      (dict(b=desc(Wt=0)), "body 0: a 3 x 0 texture"), (dict(b=desc(F=0)), "need V, F, T >= 1"),
                      (dict(out=t["tex"][2]), "must not alias an input"), (dict(depth=t["verts"][3]), "must not alias an input"),
                      (dict(key=t["faces"]), "must not alias an input"), (dict(share=alpha), "must be distinct"), (dict(depth=out), "must be distinct")):
        rc = call(**kw)
        assert rc == -1, kw                                                    # A2P_ERR_ARG
        with pytest.raises(A2PError, match=match):
            _lib.check(rc, "a2p_scene_render")
    assert call(N=0, out=None) == -1 and call(N=0) == 0
    torch.cuda.synchronize()
    for whole in (out_all, alpha_all, depth_all, share_all, proj_all):
        assert bool(torch.isnan(whole).all())                                  # untouched: no refused call and no N = 0 call launched anything
    assert bool((key_all == -7).all())
    _lib.check(call(), "a2p_scene_render")
    torch.cuda.synchronize()
    pad = 4096
    for whole, x in ((out_all, out), (alpha_all, alpha), (depth_all, depth), (share_all, share), (proj_all, proj)):
        assert bool(torch.isnan(whole[:pad]).all()) and bool(torch.isnan(whole[pad + x.numel():]).all())
    assert bool((key_all[:pad] == -7).all()) and bool((key_all[pad + key.numel():] == -7).all())
    for x in (out, alpha, depth, share):
        assert bool(torch.isfinite(x).all())                                   # every element was overwritten
    assert bool((alpha[1] == 0).all()) and bool((share[1] == 0).all()) and bool((depth[1] == 0).all()) and torch.equal(out[1], t["bg"][1])
    got_p = np.rint(share[:1].cpu().numpy().astype(np.float64) * s * s).astype(np.int64)
    record("scene_four_bodies_coverage", differing_pixels=int((got_p != ref["body_count"]).any(1).sum()), excluded_pixels=0)
    assert np.array_equal(got_p, ref["body_count"])
    assert np.array_equal(share[:1].cpu().numpy(), ref["body_count"].astype(np.float32) / np.float32(s * s))
    assert np.array_equal(alpha[:1].cpu().numpy()[:, 0], ref["count"].astype(np.float32) / np.float32(s * s))
    gate("scene_four_bodies_colour", out[:1], ref["image"], 4 * R.nerr(ref32["image"], ref["image"]))
    gate("scene_four_bodies_depth", depth[:1], ref["depth"], 4 * R.nerr(ref32["depth"], ref["depth"]))
    # the same scene through SceneRasterizer: the bits of the direct call
    sc = SN.SceneRasterizer([((m["vi"], m["vt"], m["vti"], 12), f) for m, f in zip(meshes, flips)], H, W)
    again = sc.render(t["verts"], t["tex"], t["K"], t["Rt"], supersample=s, background=t["bg"])
    assert torch.equal(again["render"], out) and torch.equal(again["alpha"], alpha) and torch.equal(again["depth"], depth) and torch.equal(again["body_alpha"], share)


# ------------------------------------------------------------------------------------------------ 7: the pipeline
SMALL = (24, 32)


@pytest.fixture(scope="module")
def people(dev, scene, body):
    """Two avatars on the synthetic assets of tests/test_render_codes_hip.py: A is that file's `body`, B has the same mesh and skeleton
    and weights from other seeds (texture, encoders, face decoder), its own motion and face codes.  Cameras at 24 x 32."""
    sc = scene["sc"]
    face_enc_cfg = dict(ER.FACE_ENC, uv_size=ENC_UV, n_embs=sc["cfg"]["n_face_embs"])
    body_enc_cfg = dict(ER.BODY_ENC, uv_size=ENC_UV, n_embs=sc["cfg"]["n_embs"])
    tex_state, tex_assets = TR.texture_state(43, B.UV, n_init_ftrs=B.TEX_CFG["n_init_ftrs"], upscale_n_ftrs=B.TEX_CFG["upscale_n_ftrs"],
                                             pose_dims=B.TEX_CFG["pose_to_shadow_dims"])
    tex_assets["seam_data_1024"] = sc["assets"]["seam_data_1024"]
    state = {**{"decoder." + k: v for k, v in sc["params"].items()}, **tex_state,
             **{"decoder_face." + k: v for k, v in ER.face_decoder_params(ER.FACE_DEC, 61).items()},
             **{"encoder_face." + k: v for k, v in ER.face_encoder_params(face_enc_cfg, 3 * ER.FACE_DEC["V"], 62).items()},
             **{"encoder." + k: v for k, v in ER.body_encoder_params(body_enc_cfg, 63).items()}}
    assets = {**scene["assets"], **tex_assets}
    surface = body["rasterizer"].surface
    a = SN.Avatar(*nets(body)[:6], surface)
    b = SN.Avatar(E.FaceDecoder.from_state_dict(state, assets), E.FaceEncoder.from_state_dict(state, assets, uv_size=ENC_UV),
                  E.BodyEncoder.from_state_dict(state, assets, surface, uv_size=ENC_UV), D.BodyDecoder.from_state_dict(state, assets, surface, **sc["cfg"]),
                  T.BodyTexture.from_state_dict(state, assets, surface, **sc["tex_cfg"]), body["skeleton"], surface)
    rs = np.random.RandomState(64)
    motion_b = (sc["motion"][::-1] + 0.05 * rs.randn(*sc["motion"].shape)).astype(np.float32)
    codes_b = rs.randn(*scene["codes"].shape).astype(np.float32)
    K = sc["K"][:2].copy()
    K[:, :2] *= np.float32(SMALL[0] / sc["size"][0])
    assert SMALL[1] / sc["size"][1] == SMALL[0] / sc["size"][0]
    return {"avatars": [a, b], "poses": [body["frames"], up(motion_b, dev)], "codes": [body["codes"], up(codes_b, dev)], "K": up(K, dev),
            "Rt": up(sc["Rt"][:2], dev), "state_b": state, "assets_b": assets}


def test_a_partner_out_of_view_leaves_render_codes_motion(dev, body, people):
    """B stands 1000 units to the side of every camera: the frames are A's own, byte for byte.  With a background or supersample > 1
    render_codes_motion resolves through render_antialiased, which one unplaced body in view reproduces bit for bit."""
    pe, (H, W) = people, SMALL
    away = SN.placement(0.0, (1000.0, 0.0, 0.0), (0, 1, 0)).numpy()
    rz = RD.BodyRasterizer(body["rasterizer"].surface, H, W)
    with torch.cuda.device(dev):
        for s, bg in ((2, [12.0, 200.0, 77.0]), (1, [0.0, 0.0, 0.0]), (3, None)):
            got = SN.render_conversation_motion(pe["avatars"], pe["poses"], pe["codes"], [None, away], pe["K"], pe["Rt"], H, W, supersample=s, background=bg)
            ref = E.render_codes_motion(*nets(body)[:6], rz, pe["poses"][0], pe["codes"][0], pe["K"], pe["Rt"], supersample=s, background=bg)
            assert got.dtype == torch.uint8 and got.shape == (3, H, 2 * W, 3) and torch.equal(got, ref), (s, bg)
            covered = float((got != (torch.tensor(bg or [0, 0, 0], device=dev).to(torch.uint8))).any(-1).float().mean())
            record(f"scene_partner_away_s{s}", covered=covered)
            assert 0.05 < covered < 0.95


def by_hand(pe, placements, dev, H, W, s, bg):
    """Each person decoded on their own, then one SceneRasterizer.render per camera and display_frames' composition."""
    shown, linear = T.display_background(bg, H, W, dev)
    sc = SN.SceneRasterizer([a.surface for a in pe["avatars"]], H, W)
    cams = RD.camera_centre(pe["Rt"])
    verts, preds = [], []
    for a, frames, codes in zip(pe["avatars"], pe["poses"], pe["codes"]):
        enc = E.encode_motion(a.face_decoder, a.face_encoder, a.body_encoder, a.skeleton, frames, codes)
        pr = a.decoder.forward(frames, enc["embs"].contiguous(), enc["face_embs"].contiguous())
        verts.append(a.skeleton.pose_vertices(frames, verts_unposed=pr["geom_delta_rec"]))
        preds.append(pr)
    panels, shares = [], []
    for c in range(pe["K"].shape[0]):
        tex = []
        for p, a in enumerate(pe["avatars"]):
            cam = cams[c:c + 1]
            if placements[p] is not None:
                world = cam
                cam = SN.camera_in_body_frame(world, placements[p].to(dev))    # R^T (c - t), held against float64 here
                ref = SC.camera_in_body_frame(world.cpu().numpy().astype(np.float64), placements[p].numpy().astype(np.float64))
                scale = float(np.abs(world.cpu().numpy()).max() + np.abs(placements[p].numpy()[:, 3]).max())     # |c| + |t| bounds every term
                assert np.abs(cam.cpu().numpy() - ref).max() <= 8 * np.finfo(np.float32).eps * scale             # 1 difference, 3 products, 2 sums
            tex.append(a.texture.forward(verts[p], preds[p]["tex_mean_rec"], cam, motion=frames_of(pe, p) if a.texture.pose_shadow is not None else None)["tex_rec"])
        got = sc.render(verts, tex, pe["K"][c:c + 1], pe["Rt"][c:c + 1], [None if m is None else m.to(dev) for m in placements], supersample=s, background=linear)
        image = T.linear_to_display(got["render"])
        panels.append(image if shown is None else torch.where(got["alpha"] == 0, shown, image))
        shares.append(got["body_alpha"])
    return torch.cat(panels, dim=-1).permute(0, 2, 3, 1).clip(0, 255).to(torch.uint8), torch.cat(shares, dim=-1)


def frames_of(pe, p):
    return pe["poses"][p]


def in_view(pe):
    """B turned by 40 degrees about the vertical through the sheet's middle and moved a little towards the cameras and to the side."""
    verts = pe["avatars"][0].skeleton.pose_vertices(pe["poses"][0][:1]).cpu().numpy()[0]
    lo, hi = verts.min(0), verts.max(0)
    extent = float((hi - lo).max())
    return SN.placement(40.0, (0.25 * extent, 0.0, 0.1 * extent), (0, 1, 0), pivot=(lo + hi) / 2)


def test_two_people_in_view_are_the_stages_by_hand(dev, people):
    pe, (H, W) = people, SMALL
    M = in_view(pe)
    with torch.cuda.device(dev):
        for s, bg in ((2, [12.0, 200.0, 77.0]), (1, None)):
            got = SN.render_conversation_motion(pe["avatars"], pe["poses"], pe["codes"], [None, M.numpy()], pe["K"], pe["Rt"], H, W, supersample=s, background=bg)
            ref, shares = by_hand(pe, [None, M], dev, H, W, s, bg)
            assert got.shape == (3, H, 2 * W, 3) and torch.equal(got, ref), (s, bg)
            seen = [float((shares[:, p] > 0).float().mean()) for p in range(2)]
            mixed = int(((shares[:, 0] > 0) & (shares[:, 1] > 0)).sum())
            record(f"scene_two_people_s{s}", person0=seen[0], person1=seen[1], pixels_with_both=mixed)
            assert min(seen) > 0.02 and (s == 1 or mixed > 0)
            assert torch.equal(got, SN.render_conversation_motion(pe["avatars"], pe["poses"], pe["codes"], [None, M], pe["K"], pe["Rt"], H, W, supersample=s,
                                                                  background=bg, max_bytes=1))                         # chunks of one frame
        # a placement per frame, and the [B, T, ..] layout
        per = np.stack([M.numpy()] * 3)
        lead = SN.render_conversation_motion(pe["avatars"], [x[None] for x in pe["poses"]], [x[None] for x in pe["codes"]], [None, per], pe["K"][:1],
                                             pe["Rt"][:1], H, W, supersample=2, background=[12.0, 200.0, 77.0])
        assert lead.shape == (1, 3, H, W, 3) and torch.equal(lead[0], got_panel(pe, M, dev, H, W))
    with pytest.raises(A2PError, match="face_codes must be"):
        SN.render_conversation_motion(pe["avatars"], [pe["poses"][0], pe["poses"][1][:2]], pe["codes"], [None, M], pe["K"], pe["Rt"], H, W)
    with pytest.raises(A2PError, match="cameras"):
        SN.render_conversation_motion(pe["avatars"], pe["poses"], pe["codes"], [None, M], pe["K"], pe["Rt"][:1], H, W)


def got_panel(pe, M, dev, H, W):
    return SN.render_conversation_motion(pe["avatars"], pe["poses"], pe["codes"], [None, M], pe["K"][:1], pe["Rt"][:1], H, W, supersample=2,
                                         background=[12.0, 200.0, 77.0])


def test_conversation_video_and_command_line(dev, scene, people, tmp_path):
    pe, (H, W), tmp = people, SMALL, tmp_path
    M = in_view(pe)
    rs = np.random.RandomState(65)
    audio = rs.uniform(-0.5, 0.5, (4800, 2))
    kw = dict(supersample=2, background=[12.0, 200.0, 77.0])
    with torch.cuda.device(dev):
        direct = SN.render_conversation_motion(pe["avatars"], pe["poses"], pe["codes"], [None, M], pe["K"], pe["Rt"], H, W, **kw)
        files = []
        for step in (32, 2, 1):
            path = tmp / f"clip{step}.avi"
            assert SN.render_conversation_video(pe["avatars"], pe["poses"], pe["codes"], [None, M], pe["K"], pe["Rt"], H, W, path, audio=audio,
                                                audio_rate=48000, slice_frames=step, **kw) == 3
            files.append(open(path, "rb").read())
        assert files[0] == files[1] == files[2]                               # a frame's bytes do not depend on the slicing
        clip = VD.read_video_frames(tmp / "clip2.avi")
        assert clip["frames"].shape == (3, H, 2 * W, 3) and clip["audio"].shape == (4800, 2) and clip["audio_rate"] == 48000
        assert np.array_equal(clip["audio"], VD.pcm16(audio))
        whole = tmp / "whole.avi"
        VD.write_video(whole, direct, audio=audio, audio_rate=48000)
        assert open(whole, "rb").read() == files[0]                            # the frames written are render_conversation_motion's
        # the command line on files
        sc, t = scene["sc"], torch.from_numpy
        s = sc["surf"]
        model, cfg = SR.as_model_dicts(sc["skel"])
        for name, assets, state, poses, codes in (("a", scene["assets"], scene["state"], pe["poses"][0], pe["codes"][0]),
                                                  ("b", pe["assets_b"], pe["state_b"], pe["poses"][1], pe["codes"][1])):
            full = {"lbs_model_json": model, "lbs_config_dict": cfg, "lbs_template_verts": t(sc["template"]), "lbs_scale": t(sc["lbs_scale"]),
                    "global_scaling": torch.tensor(float(sc["global_scaling"])), **assets,
                    "topology": {"vi": t(s["vi"]), "vt": t(s["vt"]), "vti": t(s["vti"]), "v2uv": t(s["v2uv"])}}
            torch.save(full, tmp / f"{name}_assets.pt")
            torch.save({k: t(np.ascontiguousarray(v)) for k, v in state.items()}, tmp / f"{name}.ckpt")
            np.save(tmp / f"{name}.npy", {"pose": poses.cpu().numpy()[None], "face": codes.cpu().numpy()[None]})
        json.dump({"K": pe["K"].cpu().numpy().tolist(), "Rt": pe["Rt"].cpu().numpy().tolist()}, open(tmp / "cameras.json", "w"))
        import wave
        with wave.open(str(tmp / "talk.wav"), "wb") as w:
            w.setnchannels(2), w.setsampwidth(2), w.setframerate(48000)
            w.writeframes(VD.pcm16(audio).tobytes())
        verts = pe["avatars"][0].skeleton.pose_vertices(pe["poses"][0][:1]).cpu().numpy()[0]
        pivot = (verts.min(0) + verts.max(0)) / 2
        extent = float((verts.max(0) - verts.min(0)).max())
        argv = ["--results", str(tmp / "a.npy"), str(tmp / "b.npy"), "--assets", str(tmp / "a_assets.pt"), str(tmp / "b_assets.pt"), "--checkpoint",
                str(tmp / "a.ckpt"), str(tmp / "b.ckpt"), "--yaw", "0", "40", "--position", "0", "0", "0", repr(0.25 * extent), "0", repr(0.1 * extent),
                "--pivot", "0", "0", "0", *[repr(float(x)) for x in pivot], "--size", str(H), str(W), "--supersample", "2", "--background", "12", "200", "77",
                "--camera-json", str(tmp / "cameras.json"), "--encoder-uv-size", str(ENC_UV), "--out", str(tmp / "frames.npy"), "--video",
                str(tmp / "cli.avi"), "--audio", str(tmp / "talk.wav")]
        for key, value in sc["tex_cfg"].items():
            argv += ["--" + key.replace("_", "-"), str(value)]
        for key in ("n_pose_enc_channels", "n_embs", "n_embs_enc_channels", "n_face_embs", "n_init_channels", "n_min_channels"):
            argv += ["--" + key.replace("_", "-"), str(sc["cfg"][key])]
        assert SN.main(argv) == 0
        identity = SN.placement(0.0, (0, 0, 0), (0, 1, 0))
        want = SN.render_conversation_motion(pe["avatars"], pe["poses"], pe["codes"], [identity, M], pe["K"], pe["Rt"], H, W, **kw)
    frames = np.load(tmp / "frames.npy")
    assert frames.dtype == np.uint8 and np.array_equal(frames, want.cpu().numpy()) and np.array_equal(frames, direct.cpu().numpy())
    assert open(tmp / "cli.avi", "rb").read() == files[0]
