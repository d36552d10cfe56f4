"""Anti-aliased rendered images on the MI355X (csrc/kernels_render_aa.h, audio2photoreal_amd/render.py render_antialiased /
interpolate_antialiased and what is built on them) against the float64 restatement (tests/render_aa_restatement.py) on the fixture
tests/golden/golden_render_aa_v1.npz: the two-layer scene of golden_render_v1 through four cameras that keep every SAMPLE centre
clear of every edge and every winner clear of its runner-up by 8 x the float32 error (tests/golden/make_golden_render_aa.py).

Gate: coverage is compared exactly (counts with array_equal, alpha bit for bit), no pixel excluded.  The normalised error of every
float output (max |difference| / max |value|) is at most 4 x the error of the float32 restatement against the float64 one on the
same input, the rule of tests/test_render_hip.py; the factor 4 pays for the device's fused multiply-adds and division.  Exact
branches (uncovered and fully covered pixels, call shapes, chunking, streams) are compared with ==.  Every measured value goes to
record(...) beside its allowance under render_aa_* names."""
import json
import os

import numpy as np
import pytest
import torch

import render_aa_restatement as A
import render_restatement as R
from audio2photoreal_amd import _lib
from audio2photoreal_amd import encoder as E
from audio2photoreal_amd import render as RD
from audio2photoreal_amd import skinning as SK
from audio2photoreal_amd import surface as S
from audio2photoreal_amd import texture as T
from conftest import record
from test_render_codes_hip import ENC_UV, body, nets, scene  # noqa: F401  (body, scene: fixtures, the smallest synthetic assets)
from test_render_hip import framing, guarded, skinned  # noqa: F401  (skinned is a fixture: the synthetic skinned mesh)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V = 874
EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def gold():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_render_aa_v1.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def gold1():
    g = np.load(os.path.join(ROOT, "tests", "golden", "golden_render_v1.npz"))
    return {k: g[k] for k in g.files}


@pytest.fixture(scope="module")
def mesh(gold1):
    return {"vi": gold1["vi"].astype(np.int64), "vt": gold1["vt"], "vti": gold1["vti"].astype(np.int64)}


@pytest.fixture(scope="module")
def want(gold, gold1, mesh):
    """Per fixture frame: its inputs and the restatement's sample fragments in float64 and float32, computed once and not changed."""
    out = []
    for k, (kind, s, H, W) in enumerate(A.FRAMES):
        f = {"verts": gold1["verts"][kind:kind + 1], "K": gold[f"K{k}"][None], "Rt": gold[f"Rt{k}"][None], "s": s, "H": H, "W": W,
             "tex": gold[f"tex{k}"][None], "bg": gold[f"bg{k}"][None]}
        args = (f["verts"], mesh["vi"], f["K"], f["Rt"], H, W, s)
        f["f64"], f["f32"] = A.sample_fragments(*args), A.sample_fragments(*args, dtype=np.float32)
        assert np.array_equal(f["f64"]["face"][0], gold[f"face{k}"]) and np.array_equal(f["f32"]["face"], f["f64"]["face"])
        f["count"] = A.block_count(f["f64"]["face"] >= 0, s)
        out.append(f)
    return out


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def gate(name, got, ref, allowance):
    """Record and assert one output: got (device tensor or array) against ref (float64) within `allowance` (normalised)."""
    err = R.nerr(got.cpu().numpy() if torch.is_tensor(got) else got, ref)
    record(name, err=err, allowance=float(allowance))
    assert np.isfinite(err) and err <= allowance, (name, err, allowance)


def rasterizer(mesh, H, W, **kw):
    return RD.BodyRasterizer.from_arrays(mesh["vi"], mesh["vt"], mesh["vti"], H, W, **kw)


def references(f, mesh, tex, flip, bg):
    """(float64 reference, allowance) of one fixture frame's render with texture `tex` [N or 1, C, 40, 56]; N follows tex / bg."""
    n = max(len(tex), 1 if bg is None else len(bg))
    rep = lambda x: np.repeat(x, n, axis=0)
    verts, K, Rt = rep(f["verts"]), f["K"], f["Rt"]
    frag = lambda d: {k: rep(v) for k, v in d.items()}
    ref = A.render_antialiased(verts, mesh, K, Rt, f["H"], f["W"], f["s"], tex, flip, bg, fragments=frag(f["f64"]))
    ref32 = A.render_antialiased(verts, mesh, K, Rt, f["H"], f["W"], f["s"], tex, flip, bg, dtype=np.float32, fragments=frag(f["f32"]))
    return ref, 4 * R.nerr(ref32["image"], ref["image"])


# ------------------------------------------------------------------------------------------------ 1: coverage
def test_fixture_coverage_is_exact(dev, mesh, want):
    for k, f in enumerate(want):
        s, H, W = f["s"], f["H"], f["W"]
        out = rasterizer(mesh, H, W).render_antialiased(up(f["verts"], dev), up(f["tex"], dev), up(f["K"], dev), up(f["Rt"], dev), supersample=s)
        assert set(out) == {"render", "alpha"} and out["render"].shape == (1, 3, H, W) and out["alpha"].shape == (1, 1, H, W)
        assert out["render"].dtype == out["alpha"].dtype == torch.float32
        alpha = out["alpha"].cpu().numpy()[:, 0]
        got = np.rint(alpha.astype(np.float64) * s * s).astype(np.int64)
        partly = int(((f["count"] > 0) & (f["count"] < s * s)).sum())
        record(f"render_aa_coverage{k}", differing_pixels=int((got != f["count"]).sum()), excluded_pixels=0, partly_covered=partly)
        assert np.array_equal(got, f["count"]) and partly >= 20
        assert np.array_equal(alpha, f["count"].astype(np.float32) / np.float32(s * s))     # the bits of (float)n / (float)(s s)


# ------------------------------------------------------------------------------------------------ 2: colours
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("C", [1, 3, 16])
def test_fixture_colours(dev, mesh, want, C, flip):
    rs = np.random.RandomState(100 + C)
    for k, f in enumerate(want):
        s, H, W = f["s"], f["H"], f["W"]
        tex = f["tex"] if C == 3 else rs.randn(1, C, 40, 56).astype(np.float32)
        bg = f["bg"] if C == 3 else rs.randn(1, C, H, W).astype(np.float32)
        rz = rasterizer(mesh, H, W, flip_uv=flip)
        cam = (up(f["K"], dev), up(f["Rt"], dev))
        plain = rz.render_antialiased(up(f["verts"], dev), up(tex, dev), *cam, supersample=s)
        over = rz.render_antialiased(up(f["verts"], dev), up(tex, dev), *cam, supersample=s, background=up(bg, dev))
        for name, got, back in (("plain", plain, None), ("over", over, bg)):
            ref, allow = references(f, mesh, tex, flip, back)
            gate(f"render_aa_colour{k}_C{C}_flip{int(flip)}_{name}", got["render"], ref["image"], allow)
        assert torch.equal(plain["alpha"], over["alpha"])
        none, full = (plain["alpha"] == 0).expand(-1, C, -1, -1), (plain["alpha"] == 1).expand(-1, C, -1, -1)
        assert bool(none.any()) and bool(full.any())
        assert bool((plain["render"][none] == 0).all()) and torch.equal(over["render"][none], up(bg, dev)[none])
        # a fully covered pixel does not read the background: NaN behind it changes nothing
        holed = up(bg, dev).clone()
        holed[full] = float("nan")
        again = rz.render_antialiased(up(f["verts"], dev), up(tex, dev), *cam, supersample=s, background=holed)
        assert torch.equal(again["render"], over["render"]) and torch.equal(over["render"][full], plain["render"][full])
        # a colour [C] is the constant image
        colour = up(rs.randn(C).astype(np.float32), dev)
        flat = rz.render_antialiased(up(f["verts"], dev), up(tex, dev), *cam, supersample=s, background=colour)
        assert torch.equal(flat["render"], rz.render_antialiased(up(f["verts"], dev), up(tex, dev), *cam, supersample=s,
                                                                 background=colour.reshape(1, C, 1, 1).expand(1, C, H, W).contiguous())["render"])
    # the last frame three times: a texture and a background per frame, and one of each shared by the three
    f = want[3]
    s, H, W = f["s"], f["H"], f["W"]
    tex3, bg3 = rs.randn(3, C, 40, 56).astype(np.float32), rs.randn(3, C, H, W).astype(np.float32)
    rz = rasterizer(mesh, H, W, flip_uv=flip)
    verts3, cam = up(np.repeat(f["verts"], 3, axis=0), dev), (up(f["K"], dev), up(f["Rt"], dev))
    per_frame = rz.render_antialiased(verts3, up(tex3, dev), *cam, supersample=s, background=up(bg3, dev))
    ref, allow = references(f, mesh, tex3, flip, bg3)
    gate(f"render_aa_colour_per_frame_C{C}_flip{int(flip)}", per_frame["render"], ref["image"], allow)
    shared = rz.render_antialiased(verts3, up(tex3[1:2], dev), *cam, supersample=s, background=up(bg3[1:2], dev))
    assert torch.equal(shared["render"][0], per_frame["render"][1]) and torch.equal(shared["render"][2], per_frame["render"][1])
    assert not torch.equal(per_frame["render"][0], per_frame["render"][1])


@pytest.mark.parametrize("C", [1, 7, 16])
def test_fixture_attributes_and_depth(dev, mesh, want, C):
    f = want[C % 4]
    s, H, W = f["s"], f["H"], f["W"]
    values = np.random.RandomState(120 + C).randn(1, V, C).astype(np.float32)
    args = (f["verts"], mesh, f["K"], f["Rt"], H, W, s, values)
    ref, ref32 = A.interpolate_antialiased(*args, fragments=f["f64"]), A.interpolate_antialiased(*args, dtype=np.float32, fragments=f["f32"])
    got = rasterizer(mesh, H, W).interpolate_antialiased(up(f["verts"], dev), up(values, dev), up(f["K"], dev), up(f["Rt"], dev), supersample=s)
    assert set(got) == {"values", "alpha", "depth"} and got["values"].shape == (1, C, H, W) and got["depth"].shape == (1, 1, H, W)
    gate(f"render_aa_values_C{C}", got["values"], ref["image"], 4 * R.nerr(ref32["image"], ref["image"]))
    gate(f"render_aa_depth_C{C}", got["depth"], ref["depth"], 4 * R.nerr(ref32["depth"], ref["depth"]))
    assert np.array_equal(got["alpha"].cpu().numpy()[:, 0], f["count"].astype(np.float32) / np.float32(s * s))
    none = got["alpha"] == 0
    assert bool((got["values"][none.expand(-1, C, -1, -1)] == 0).all()) and bool((got["depth"][none] == 0).all())


# ------------------------------------------------------------------------------------------------ 3: the single-sample path
def test_against_the_single_sample_path_at_the_sample_grid(dev, gold, mesh, want):
    for k, f in enumerate(want):
        s, H, W = f["s"], f["H"], f["W"]
        verts, tex, Rt = up(f["verts"], dev), up(f["tex"], dev), up(f["Rt"], dev)
        Ks = up(A.scaled_camera(f["K"], s), dev)
        big = rasterizer(mesh, s * H, s * W)
        frag = big.rasterize(verts, Ks, Rt)
        assert np.array_equal(frag["face"][0].cpu().numpy(), gold[f"face{k}"])                # the sample faces, no sample excluded
        got = rasterizer(mesh, H, W).render_antialiased(verts, tex, up(f["K"], dev), Rt, supersample=s)
        blocks = big.mask(frag).reshape(1, H, s, W, s).sum(dim=(2, 4))
        assert torch.equal(blocks, got["alpha"][:, 0] * (s * s))
        _, allow = references(f, mesh, f["tex"], False, None)
        mean = A.block_mean(big.sample_texture(frag, tex).cpu().numpy(), s)
        gate(f"render_aa_block_mean{k}", got["render"], mean, allow)


# ------------------------------------------------------------------------------------------------ 4: S = 1 through the fused kernel
def test_one_sample_through_the_fused_kernel(dev, gold1, mesh):
    """Reached with a background.  On a frame of golden_render_v1, whose camera clears every pixel centre at one sample per pixel."""
    k = 2
    H, W = R.SIZES[k]
    v, K, Rt, tex = gold1["verts"][k:k + 1], gold1["K"][k:k + 1], gold1["Rt"][k:k + 1], gold1["tex"][k:k + 1]
    bg = np.random.RandomState(130).randn(1, 3, H, W).astype(np.float32)
    rz = rasterizer(mesh, H, W)
    frag = rz.rasterize(up(v, dev), up(K, dev), up(Rt, dev))
    single = rz.sample_texture(frag, up(tex, dev))
    got = rz.render_antialiased(up(v, dev), up(tex, dev), up(K, dev), up(Rt, dev), supersample=1, background=up(bg, dev))
    assert torch.equal(got["alpha"], rz.mask(frag))                            # 0 or 1 exactly
    f64, f32 = R.rasterize(v, mesh["vi"], K, Rt, H, W), R.rasterize(v, mesh["vi"], K, Rt, H, W, dtype=np.float32)
    ref = A.render_antialiased(v, mesh, K, Rt, H, W, 1, tex, background=bg, fragments=f64)
    ref32 = A.render_antialiased(v, mesh, K, Rt, H, W, 1, tex, background=bg, dtype=np.float32, fragments=f32)
    allow = 4 * R.nerr(ref32["image"], ref["image"])
    gate("render_aa_one_sample", got["render"], ref["image"], allow)
    hit = (got["alpha"] == 1).expand(-1, 3, -1, -1)
    gate("render_aa_one_sample_vs_render", torch.where(hit, got["render"], single), single.cpu().numpy().astype(np.float64), allow)
    assert torch.equal(got["render"][~hit], up(bg, dev)[~hit])                 # not bits of `single` on covered pixels: contraction may differ
    plain = rz.render_antialiased(up(v, dev), up(tex, dev), up(K, dev), up(Rt, dev), supersample=1)
    assert torch.equal(plain["render"][hit], got["render"][hit]) and bool((plain["render"][~hit] == 0).all())


# ------------------------------------------------------------------------------------------------ 5: call shapes
@pytest.fixture(scope="module")
def nineteen(dev, gold1):
    """19 frames of the scene with a camera, a background and attribute values each."""
    rs = np.random.RandomState(70)
    H, W = R.SIZES[2]
    verts = gold1["verts"][rs.randint(0, 3, 19)] + rs.randn(19, 1, 3).astype(np.float32) * 0.02
    Rt = gold1["Rt"][[2] * 19].copy()
    Rt[:, :, 3] += rs.randn(19, 3).astype(np.float32) * 0.03
    K = gold1["K"][[2] * 19].copy()
    K[:, 0, 0] *= (1 + rs.rand(19).astype(np.float32) * 0.1)
    return {"verts": up(verts, dev), "K": up(K, dev), "Rt": up(Rt, dev), "values": up(rs.randn(19, V, 2).astype(np.float32), dev),
            "tex": up(gold1["tex"][:1], dev), "bg": up(rs.randn(19, 3, H, W).astype(np.float32), dev)}


def run_all(rz, n, s, lo=0, hi=19, **kw):
    a = rz.render_antialiased(n["verts"][lo:hi], n["tex"], n["K"][lo:hi], n["Rt"][lo:hi], supersample=s, background=n["bg"][lo:hi], **kw)
    b = rz.interpolate_antialiased(n["verts"][lo:hi], n["values"][lo:hi], n["K"][lo:hi], n["Rt"][lo:hi], supersample=s, **kw)
    return {**a, **{"v_" + k: v for k, v in b.items()}}


def same(a: dict, b: dict):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


@pytest.mark.parametrize("s", [2, 3])
def test_a_frames_bits_do_not_depend_on_the_call(dev, mesh, nineteen, s):
    H, W = R.SIZES[2]
    rz = rasterizer(mesh, H, W)
    full = run_all(rz, nineteen, s)
    assert full["render"].shape == (19, 3, H, W) and full["v_values"].shape == (19, 2, H, W) and full["v_depth"].shape == (19, 1, H, W)
    assert len({float(full["alpha"][n].sum()) for n in range(19)}) > 5         # the frames do differ
    assert bool(((full["alpha"] > 0) & (full["alpha"] < 1)).any())
    assert same(full, run_all(rz, nineteen, s)), "two identical runs differ"
    for lo, hi in ((0, 1), (7, 9), (18, 19)):
        alone = run_all(rz, nineteen, s, lo, hi)
        assert all(torch.equal(alone[k], full[k][lo:hi]) for k in full), (lo, hi)
    assert same(full, run_all(rz, nineteen, s, max_bytes=1))                   # one frame per chunk
    assert same(full, run_all(rz, nineteen, s, max_bytes=3 * (12 * V + 8 * s * s * H * W) + 5))    # three per chunk: 6 x 3 + 1
    torch.cuda.synchronize()
    side = torch.cuda.Stream(device=dev)
    with torch.cuda.stream(side):
        got = run_all(rasterizer(mesh, H, W), nineteen, s)
    side.synchronize()
    assert same(full, got)
    # one camera for all frames: [1, 3, .], [3, .] and the same camera repeated give the same bits
    n = nineteen
    K, Rt = n["K"][4:5], n["Rt"][4:5]
    call = lambda K, Rt: rz.render_antialiased(n["verts"], n["tex"], K, Rt, supersample=s, background=n["bg"][:1])
    shared = call(K, Rt)
    assert same(shared, call(K.repeat(19, 1, 1), Rt.repeat(19, 1, 1))) and same(shared, call(K[0], Rt.repeat(19, 1, 1)))
    assert torch.equal(shared["render"][4], rz.render_antialiased(n["verts"][4:5], n["tex"], K, Rt, supersample=s, background=n["bg"][:1])["render"][0])
    empty = rz.render_antialiased(n["verts"][:0], n["tex"], K, Rt, supersample=s)
    assert empty["render"].shape == (0, 3, H, W) and empty["alpha"].shape == (0, 1, H, W)


# ------------------------------------------------------------------------------------------------ 6: the C ABI, exact branches
def test_large_faces_dropped_faces_and_prefilled_outputs_through_the_c_abi(dev):
    """A 24 x 40 image at s = 4.  Face 0 fills the screen (its box holds all 96 x 160 samples: the listed-face path of the cover
    pass), face 1 is a small triangle in front of it, face 2 has a corner nearer than `near`, face 3 is a point and has no area.
    Frame 1 is frame 0 with NaN vertices.  Outputs and scratch start as NaN between guards."""
    H, W, s, C = 24, 40, 4, 2
    K = np.array([[[30.0, 0, 20.0], [0, 30, 12.0], [0, 0, 1]]], np.float32)
    Rt = np.concatenate([np.eye(3), np.zeros((3, 1))], 1)[None].astype(np.float32)
    one = np.array([[-9.13, -7.31, 3], [9.77, -7.03, 3.4], [0.21, 14.9, 3.1],               # the whole screen and more
                    [-0.3171, -0.2113, 2], [0.4077, -0.1219, 2.1], [0.0533, 0.3391, 2.2],   # in front, near the middle
                    [0.1, 0.1, 5e-4], [0.5, 0.1, 2], [0.1, 0.5, 2],                         # a corner at half of `near`
                    [-0.5, 0.1, 2.5], [-0.3, 0.2, 2.5], [-0.1, 0.3, 2.5]], np.float32)      # face 3 uses the first of these three times
    verts = np.stack([one, np.full_like(one, np.nan)])
    vi = np.array([[0, 1, 2], [3, 4, 5], [6, 7, 8], [9, 9, 9]])
    mesh = {"vi": vi, "vt": np.random.RandomState(4).rand(12, 2).astype(np.float32), "vti": vi}
    Ks = A.scaled_camera(K, s)
    assert R.edge_clearance(verts[:1], vi[:2], Ks, Rt, s * H, s * W) > 1e-3     # the scene itself: no sample centre near an edge
    tex = np.random.RandomState(5).randn(1, C, 6, 7).astype(np.float32)
    bg = np.random.RandomState(6).randn(2, C, H, W).astype(np.float32)
    args = (verts[:1], mesh, K, Rt, H, W, s, tex)
    ref, ref32 = A.render_antialiased(*args, background=bg[:1]), A.render_antialiased(*args, background=bg[:1], dtype=np.float32)
    f64 = A.sample_fragments(verts[:1], vi, K, Rt, H, W, s)
    assert set(np.unique(f64["face"])) == {0, 1} and np.array_equal(ref32["count"], ref["count"]) and (ref["count"] == s * s).all()
    several = int((A.winning_faces(f64["face"][0], s) > 1).sum())
    assert several >= 8                                                        # the small face's outline crosses pixels
    nan = float("nan")
    out, out_all = guarded(dev, (2, C, H, W), torch.float32, nan)
    alpha, alpha_all = guarded(dev, (2, 1, H, W), torch.float32, nan)
    proj, proj_all = guarded(dev, (2, 12, 3), torch.float32, nan)
    key, key_all = guarded(dev, (2, s * H, s * W), torch.int64, -7)
    t = {k: up(v, dev) for k, v in (("verts", verts), ("vi", vi.astype(np.int32)), ("vt", mesh["vt"]), ("K", K), ("Rt", Rt), ("tex", tex), ("bg", bg))}
    lib, p, stream = _lib.load(), _lib.ptr, _lib.current_stream(dev)

    def texture(S=s, H=H, W=W, C=C, out=out, bg=t["bg"], N=2):
        return lib.a2p_render_antialiased_texture(p(t["verts"]), N, 12, p(t["vi"]), 4, p(t["vt"]), 12, p(t["vi"]), p(t["K"]), 0, p(t["Rt"]), 0, H, W, S,
                                                  1e-3, p(t["tex"]), 0, C, 6, 7, 0, p(bg), 1, p(proj), p(key), p(out), p(alpha), stream)

    _lib.check(texture(), "a2p_render_antialiased_texture")
    torch.cuda.synchronize()
    pad = 4096
    for whole, n in ((out_all, out.numel()), (alpha_all, alpha.numel()), (proj_all, proj.numel())):
        assert bool(torch.isnan(whole[:pad]).all()) and bool(torch.isnan(whole[pad + n:]).all())
    assert bool((key_all[:pad] == -7).all()) and bool((key_all[pad + key.numel():] == -7).all())
    assert bool(torch.isfinite(out).all()) and bool(torch.isfinite(alpha).all())              # every element was overwritten
    assert bool((alpha[0] == 1).all()) and bool((alpha[1] == 0).all())
    assert torch.equal(out[1], t["bg"][1])                                     # NaN vertices: nothing is covered, the background is exact
    gate("render_aa_large_face", out[:1], ref["image"], 4 * R.nerr(ref32["image"], ref["image"]))
    # the values export with its depth, and without: the same bits
    values = up(np.random.RandomState(7).randn(2, 12, 5).astype(np.float32), dev)
    vout, vout_all = guarded(dev, (2, 5, H, W), torch.float32, nan)
    depth, depth_all = guarded(dev, (2, 1, H, W), torch.float32, nan)

    def attributes(S=s, H=H, depth=depth, out=vout, C=5):
        return lib.a2p_render_antialiased_values(p(t["verts"]), 2, 12, p(t["vi"]), 4, p(t["K"]), 0, p(t["Rt"]), 0, H, W, S, 1e-3, p(values), C,
                                                 None, 0, p(proj), p(key), p(out), p(alpha), p(depth), stream)

    _lib.check(attributes(), "a2p_render_antialiased_values")
    torch.cuda.synchronize()
    vref = A.interpolate_antialiased(verts[:1], mesh, K, Rt, H, W, s, values[:1].cpu().numpy())
    vref32 = A.interpolate_antialiased(verts[:1], mesh, K, Rt, H, W, s, values[:1].cpu().numpy(), dtype=np.float32)
    gate("render_aa_large_face_values", vout[:1], vref["image"], 4 * R.nerr(vref32["image"], vref["image"]))
    gate("render_aa_large_face_depth", depth[:1], vref["depth"], 4 * R.nerr(vref32["depth"], vref["depth"]))
    assert bool((vout[1] == 0).all()) and bool((depth[1] == 0).all()) and bool((alpha[1] == 0).all())
    for whole, n in ((vout_all, vout.numel()), (depth_all, depth.numel())):
        assert bool(torch.isnan(whole[:pad]).all()) and bool(torch.isnan(whole[pad + n:]).all())
    first = vout.clone()
    vout.fill_(nan)
    _lib.check(attributes(depth=None), "a2p_render_antialiased_values")
    assert torch.equal(vout, first)
    # bad arguments are refused before any launch
    for call, match in ((lambda: texture(S=0), "need 1 <= S <= 4"), (lambda: texture(S=5), "need 1 <= S <= 4"),
                        (lambda: texture(S=4, H=_lib.RENDER_MAX_SIZE // 4 + 1), "S H, S W <= 8192"), (lambda: texture(H=0), "need 1 <= H, W"),
                        (lambda: texture(C=17), r"C=17 outside \[1, 16\]"), (lambda: texture(out=None), "null argument"),
                        (lambda: texture(out=t["tex"]), "must not alias an input"), (lambda: texture(out=alpha), "must be distinct"),
                        (lambda: attributes(S=-1), "need 1 <= S <= 4"), (lambda: attributes(out=None), "null argument"),
                        (lambda: attributes(depth=vout), "must be distinct"), (lambda: attributes(C=0), r"C=0 outside \[1, 16\]")):
        rc = call()
        assert rc == -1                                                        # A2P_ERR_ARG
        with pytest.raises(_lib.A2PError, match=match):
            _lib.check(rc, "a2p_render_antialiased")
    assert texture(N=0, out=None) == -1 and texture(N=0) == 0


# ------------------------------------------------------------------------------------------------ 7: render_motion
def test_render_motion_supersampled_is_the_block_mean(dev, skinned):
    """render_motion(..., supersample=2) against the block mean (float64) of the single-sample call at (2 H, 2 W) through K'.
    Allowance 16 float32 epsilons of the largest value: a sample's barycentrics and depth are the same bits on both sides
    (render_pixel, uncontracted), its three-term interpolation may be contracted differently in the two kernels (at most 3
    roundings of half an epsilon each, on either side), and the sum of four samples adds 3 roundings of partial sums at most 4 x as
    large before the exact division by 4: under 8 epsilons, doubled."""
    sk, topo = skinned
    H, W, s = 20, 26, 2
    sf = S.BodySurface.from_arrays(topo["vi"], topo["vt"], topo["vti"], uv_size=32)
    pose = np.random.RandomState(60).randn(2, 3, 104) * 0.6
    names = ("depth", "normals", "view_cos", "positions", "mask")
    with torch.cuda.device(dev):
        verts = SK.pose_motion(sk, pose)["vertices"]
        K, Rt = framing(verts.cpu().numpy(), H, W, dev)
        Ks = up(A.scaled_camera(K.cpu().numpy(), s), dev)
        fine = RD.render_motion(RD.BodyRasterizer(sf, s * H, s * W), sf, verts, Ks, Rt, outputs=names)
        rz = RD.BodyRasterizer(sf, H, W)
        got = RD.render_motion(rz, sf, verts, K, Rt, outputs=names, supersample=s)
        assert {k: tuple(v.shape) for k, v in got.items()} == {"depth": (2, 3, 1, H, W), "normals": (2, 3, 3, H, W), "view_cos": (2, 3, 1, H, W),
                                                             "positions": (2, 3, 3, H, W), "mask": (2, 3, 1, H, W)}
        for k in names:
            mean = A.block_mean(fine[k].cpu().numpy(), s)
            if k == "mask":
                assert np.array_equal(got[k].cpu().numpy(), mean.astype(np.float32))          # the coverage, exactly
                assert bool(((got[k] > 0) & (got[k] < 1)).any())
            else:
                gate(f"render_aa_motion_{k}", got[k], mean, 16 * EPS)
        # only depth and mask; chunked by a tiny budget; the flat layout; the default is today's call
        few = RD.render_motion(rz, sf, verts, K, Rt, outputs=("depth", "mask"), supersample=s)
        assert torch.equal(few["depth"], got["depth"]) and torch.equal(few["mask"], got["mask"])
        tiny = RD.render_motion(rz, sf, verts.reshape(6, 500, 3), K, Rt, outputs=names, supersample=s, max_bytes=1)
        assert all(torch.equal(tiny[k], got[k].reshape(tiny[k].shape)) for k in names)
        one = RD.render_motion(rz, sf, verts, K, Rt, outputs=names, supersample=1)
        assert all(torch.equal(one[k], v) for k, v in RD.render_motion(rz, sf, verts, K, Rt, outputs=names).items())


# ------------------------------------------------------------------------------------------------ 8: RGB frames and video frames
def stages_by_hand(b, frames, embs, face_embs, K, Rt, s, shown):
    """decode, pose, texture, render_antialiased, linear_to_display, select: display RGB [N, 3, H, W] and alpha of one camera."""
    preds = b["decoder"].forward(frames, embs.contiguous(), face_embs.contiguous())
    verts = b["skeleton"].pose_vertices(frames, verts_unposed=preds["geom_delta_rec"])
    tex = b["texture"].forward(verts, preds["tex_mean_rec"], RD.camera_centre(Rt), motion=frames if b["texture"].pose_shadow is not None else None)
    linear = T.display_to_linear(shown.cpu()).reshape(3).to(shown.device)     # converted once, on the host
    got = b["rasterizer"].render_antialiased(verts, tex["tex_rec"], K, Rt, s, linear)
    return torch.where(got["alpha"] == 0, shown, T.linear_to_display(got["render"])), got["alpha"]


def test_rgb_and_video_frames_with_a_background(dev, body):
    b = body
    H, W = b["rasterizer"].height, b["rasterizer"].width
    colour = [12.0, 200.0, 77.0]
    with torch.cuda.device(dev):
        shown = torch.tensor(colour, device=dev).reshape(3, 1, 1)
        enc = E.encode_motion(b["face_decoder"], b["face_encoder"], b["body_encoder"], b["skeleton"], b["frames"], b["codes"])
        args = (b["decoder"], b["texture"], b["skeleton"], b["rasterizer"], b["frames"], enc["embs"], enc["face_embs"])
        rgb = T.render_rgb_motion(*args, b["K"][:1], b["Rt"][:1], supersample=2, background=colour)
        want, alpha = stages_by_hand(b, b["frames"], enc["embs"], enc["face_embs"], b["K"][:1], b["Rt"][:1], 2, shown)
        assert rgb.shape == (3, 3, H, W) and torch.equal(rgb, want)
        none = (alpha == 0).expand(-1, 3, -1, -1)
        partly = float(((alpha > 0) & (alpha < 1)).float().mean())
        record("render_aa_rgb_frames", uncovered=float((alpha == 0).float().mean()), partly_covered=partly)
        assert bool(none.any()) and partly > 0 and torch.equal(rgb[none], shown.expand(3, 3, H, W)[none])
        panel = torch.tensor(np.random.RandomState(140).uniform(0, 255, (H, W, 3)).astype(np.float32))
        over = T.render_rgb_motion(*args, b["K"][:1], b["Rt"][:1], supersample=2, background=panel)
        assert torch.equal(over[none], panel.permute(2, 0, 1).to(dev).expand(3, 3, H, W)[none]) and torch.equal(over[alpha.expand(-1, 3, -1, -1) == 1],
                                                                                                                rgb[alpha.expand(-1, 3, -1, -1) == 1])
        assert torch.equal(over, T.render_rgb_motion(*args, b["K"][:1], b["Rt"][:1], supersample=2, background=panel.permute(2, 0, 1), max_bytes=1))
        # with the defaults: today's call
        assert torch.equal(T.render_rgb_motion(*args, b["K"][:1], b["Rt"][:1], supersample=1, background=None),
                           T.render_rgb_motion(*args, b["K"][:1], b["Rt"][:1]))
        # the uint8 frames: both cameras over the same colour
        frames = E.render_codes_motion(*nets(b), b["frames"], b["codes"], b["K"], b["Rt"], supersample=2, background=colour)
        assert frames.dtype == torch.uint8 and frames.shape == (3, H, 2 * W, 3)
        for c in range(2):
            want, alpha = stages_by_hand(b, b["frames"], enc["embs"], enc["face_embs"], b["K"][c:c + 1], b["Rt"][c:c + 1], 2, shown)
            assert torch.equal(frames[:, :, c * W:(c + 1) * W], want.permute(0, 2, 3, 1).clip(0, 255).to(torch.uint8))
            none = (alpha[:, 0] == 0)
            assert bool(none.any()) and bool((frames[:, :, c * W:(c + 1) * W][none] == torch.tensor([12, 200, 77], dtype=torch.uint8, device=dev)).all())
        assert torch.equal(E.render_codes_motion(*nets(b), b["frames"], b["codes"], b["K"], b["Rt"], supersample=1, background=None),
                           E.render_codes_motion(*nets(b), b["frames"], b["codes"], b["K"], b["Rt"]))
    with pytest.raises(ValueError, match="supersample=7"):
        E.render_codes_motion(*nets(b), b["frames"], b["codes"], b["K"], b["Rt"], supersample=7)
    with pytest.raises(ValueError, match="three numbers"):
        T.render_rgb_motion(*args, b["K"][:1], b["Rt"][:1], background=[1.0, 2.0])


# ------------------------------------------------------------------------------------------------ 9: command lines
def test_the_command_lines_take_the_new_flags(dev, skinned, scene, body, tmp_path):
    import skinning_restatement as SR
    _, topo = skinned
    rs = np.random.RandomState(61)
    ii, jj = np.meshgrid(np.arange(25), np.arange(20))
    sheet = np.stack([ii * 0.1, jj * 0.1, 0.2 * np.sin(ii * 0.5)], -1).reshape(500, 3)
    verts = (sheet + rs.randn(1, 2, 500, 3) * 0.01).astype(np.float32)
    v2uv = S.compute_v2uv(500, topo["vi"], topo["vti"])
    t = torch.from_numpy
    torch.save({"topology": {"vi": t(topo["vi"]), "vt": t(topo["vt"]), "vti": t(topo["vti"]), "v2uv": t(v2uv)}}, tmp_path / "topology.pt")
    np.save(tmp_path / "geometry.npy", {"vertices": verts})
    sf = S.BodySurface.from_arrays(topo["vi"], topo["vt"], topo["vti"], v2uv=v2uv)
    with torch.cuda.device(dev):
        assert RD.main(["--geometry", str(tmp_path / "geometry.npy"), "--assets", str(tmp_path / "topology.pt"), "--size", "30", "44", "--eye", "1.0",
                        "0.5", "4.0", "--target", "1.2", "0.9", "0.0", "--fov", "38", "--out", str(tmp_path / "maps.npy"), "--supersample", "3"]) == 0
        K, Rt = RD.look_at([1.0, 0.5, 4.0], [1.2, 0.9, 0.0], [0, 1, 0], 30, 44, 38.0, device=dev)
        want = RD.render_motion(RD.BodyRasterizer(sf, 30, 44), sf, up(verts, dev), K[None], Rt[None], outputs=("depth", "normals", "view_cos", "mask"),
                                supersample=3)
    got = np.load(tmp_path / "maps.npy", allow_pickle=True).item()
    assert set(got) == set(want) and all(np.array_equal(got[k], want[k].cpu().numpy()) for k in want)
    assert ((got["mask"] > 0) & (got["mask"] < 1)).any()
    # the video frames' command line (the files of tests/test_render_codes_hip.py)
    sc, tmp = scene["sc"], tmp_path
    s = sc["surf"]
    model, cfg = SR.as_model_dicts(sc["skel"])
    assets = {"lbs_model_json": model, "lbs_config_dict": cfg, "lbs_template_verts": t(sc["template"]), "lbs_scale": t(sc["lbs_scale"]),
              "global_scaling": torch.tensor(float(sc["global_scaling"])), **scene["assets"],
              "topology": {"vi": t(s["vi"]), "vt": t(s["vt"]), "vti": t(s["vti"]), "v2uv": t(s["v2uv"])}}
    torch.save(assets, tmp / "static_assets.pt")
    torch.save({k: t(np.ascontiguousarray(v)) for k, v in scene["state"].items()}, tmp / "body_dec.ckpt")
    np.save(tmp / "results.npy", {"pose": sc["motion"][None].astype(np.float32), "face": scene["codes"][None]})
    json.dump({"K": sc["K"][:2].tolist(), "Rt": sc["Rt"][:2].tolist()}, open(tmp / "cameras.json", "w"))
    common = ["--assets", str(tmp / "static_assets.pt"), "--checkpoint", str(tmp / "body_dec.ckpt"), "--size", "96", "128",
              "--supersample", "2", "--background", "12", "200", "77"]
    for key, value in sc["tex_cfg"].items():
        common += ["--" + key.replace("_", "-"), str(value)]
    for key in ("n_pose_enc_channels", "n_embs", "n_embs_enc_channels", "n_face_embs", "n_init_channels", "n_min_channels"):
        common += ["--" + key.replace("_", "-"), str(sc["cfg"][key])]
    argv = common + ["--results", str(tmp / "results.npy"), "--encoder-uv-size", str(ENC_UV), "--camera-json", str(tmp / "cameras.json"),
                     "--out", str(tmp / "frames.npy")]
    with torch.cuda.device(dev):
        assert E.main(argv) == 0
        direct = E.render_codes_motion(*nets(body), body["frames"], body["codes"], body["K"], body["Rt"], supersample=2, background=[12.0, 200.0, 77.0])
    frames = np.load(tmp / "frames.npy")
    assert frames.dtype == np.uint8 and np.array_equal(frames[0], direct.cpu().numpy())
    # the RGB frames' command line: the same checkpoint and assets, the scene's own embeddings, one camera
    np.save(tmp / "motions.npy", {"motions": np.ascontiguousarray(sc["motion"].astype(np.float32).T[None, :, None, :])})          # [1, P, 1, 3]
    np.savez(tmp / "embs.npz", embs=sc["embs"][None], face_embs=sc["face_embs"][None])
    json.dump({"K": sc["K"][0].tolist(), "Rt": sc["Rt"][0].tolist()}, open(tmp / "camera.json", "w"))
    rgb_argv = common + ["--results", str(tmp / "motions.npy"), "--embeddings", str(tmp / "embs.npz"), "--camera-json", str(tmp / "camera.json"),
                         "--out", str(tmp / "rgb.npy")]
    with torch.cuda.device(dev):
        assert T.main(rgb_argv) == 0
        b = body
        direct = T.render_rgb_motion(b["decoder"], b["texture"], b["skeleton"], b["rasterizer"], b["frames"][None], up(sc["embs"], dev)[None],
                                     up(sc["face_embs"], dev)[None], up(sc["K"][:1], dev), up(sc["Rt"][:1], dev), supersample=2,
                                     background=[12.0, 200.0, 77.0])
    rgb = np.load(tmp / "rgb.npy")
    assert rgb.dtype == np.float32 and rgb.shape == (1, 3, 3, 96, 128) and np.array_equal(rgb, direct.cpu().numpy())
