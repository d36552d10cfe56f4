"""A numpy restatement of the anti-aliased rendered images (audio2photoreal_amd/render.py render_antialiased and
interpolate_antialiased), written from the rule in INTEGRATION.md "Rendered images" on top of tests/render_restatement.py, which is
imported and not changed.  Test infrastructure: the yardstick of tests/test_render_aa_hip.py and tests/test_render_aa_cpu.py, and what
tests/golden/make_golden_render_aa.py builds its fixture with.

The rule.  s samples per axis, 1 <= s <= 4.  Sample (a, b) of pixel (i, j) is pixel (s i + a, s j + b) of the s H x s W image seen
through K' = K with its first two rows multiplied by s in float32; a sample's face, barycentrics and depth are what
render_restatement.rasterize gives there, its colour what sample_texture / interpolate give.  Resolve: a outer, b inner, accumulators
that start at 0; every covered sample adds its value and n counts them; alpha = n / (s s), mean = acc / (s s); with a background
the pixel is mean when n == s s, the background itself when n == 0, and mean + (1 - alpha) background otherwise; without one, mean.

Every numeric function takes `dtype` (float64 by default); the float32 run sums in the kernel's order, so that its distance to the
float64 run is the rounding error float32 arithmetic makes on the input: the allowance of the GPU tests."""
import numpy as np

import render_restatement as R

MAX_SUPERSAMPLE = 4


def scaled_camera(K, s):
    """K' [.., 3, 3] float32: K as float32 with its first two rows multiplied by s in float32, whatever dtype the caller runs in."""
    Ks = np.array(K, np.float32)
    Ks[..., :2, :] = Ks[..., :2, :] * np.float32(s)
    return Ks


def sample_fragments(verts, vi, K, Rt, H, W, s, near=R.NEAR, dtype=np.float64, runner_up=False):
    """The fragments of every sample: render_restatement.rasterize at (s H, s W) through K'; arrays [N, s H, s W, ..]."""
    return R.rasterize(verts, vi, scaled_camera(K, s), Rt, s * H, s * W, near=near, dtype=dtype, runner_up=runner_up)


def resolve(samples, covered, s, background=None, dtype=np.float64):
    """samples [N, C, s H, s W] (the value of each sample), covered [N, s H, s W] bool -> {"image" [N, C, H, W], "alpha" [N, 1, H, W],
    "count" [N, H, W] int64}.  background: None or [N or 1, C, H, W] / [C]."""
    samples, covered = np.asarray(samples, dtype), np.asarray(covered, bool)
    N, C, sH, sW = samples.shape
    H, W = sH // s, sW // s
    acc = np.zeros((N, C, H, W), dtype)
    count = np.zeros((N, H, W), np.int64)
    for a in range(s):                                                        # the stated order: rows of samples outer, columns inner
        for b in range(s):
            hit = covered[:, a::s, b::s]
            acc = np.where(hit[:, None], acc + samples[:, :, a::s, b::s], acc)
            count += hit
    ss = dtype(s * s)
    alpha = (count.astype(dtype) / ss)[:, None]
    image = acc / ss
    if background is not None:
        bg = np.asarray(background, dtype)
        bg = np.broadcast_to(bg.reshape(1, C, 1, 1) if bg.ndim == 1 else bg, image.shape)
        n = count[:, None]
        image = np.where(n == s * s, image, np.where(n == 0, bg, image + (dtype(1) - alpha) * bg))
    return {"image": image, "alpha": alpha, "count": count}


def render_antialiased(verts, mesh, K, Rt, H, W, s, tex, flip_uv=False, background=None, near=R.NEAR, dtype=np.float64, fragments=None):
    """{"image" [N, C, H, W], "alpha", "count"} of tex [N or 1, C, Ht, Wt] seen through the camera with s x s samples per pixel.
    mesh: {"vi", "vt", "vti"}.  fragments: sample_fragments of the same arguments, when the caller has them already."""
    frag = sample_fragments(verts, mesh["vi"], K, Rt, H, W, s, near, dtype) if fragments is None else fragments
    colour = R.sample_texture(tex, mesh["vt"], mesh["vti"], frag["face"], frag["bary"], flip_uv, dtype)
    return resolve(colour, frag["face"] >= 0, s, background, dtype)


def interpolate_antialiased(verts, mesh, K, Rt, H, W, s, values, near=R.NEAR, dtype=np.float64, fragments=None):
    """{"image" [N, C, H, W], "alpha", "count", "depth" [N, 1, H, W]} of values [N, V, C]; depth is resolved like a channel."""
    frag = sample_fragments(verts, mesh["vi"], K, Rt, H, W, s, near, dtype) if fragments is None else fragments
    covered = frag["face"] >= 0
    out = resolve(R.interpolate(values, mesh["vi"], frag["face"], frag["bary"], dtype), covered, s, None, dtype)
    out["depth"] = resolve(np.asarray(frag["depth"], dtype)[:, None], covered, s, None, dtype)["image"]
    return out


def block_mean(x, s):
    """[.., s H, s W] -> [.., H, W] float64: the mean of each s x s block."""
    x = np.asarray(x, np.float64)
    H, W = x.shape[-2] // s, x.shape[-1] // s
    return x.reshape(*x.shape[:-2], H, s, W, s).mean(axis=(-3, -1))


def block_count(covered, s):
    """[.., s H, s W] bool -> [.., H, W] int64: the covered samples of each pixel."""
    c = np.asarray(covered, bool)
    H, W = c.shape[-2] // s, c.shape[-1] // s
    return c.reshape(*c.shape[:-2], H, s, W, s).sum(axis=(-3, -1)).astype(np.int64)


def winning_faces(face, s):
    """[H, W] int64: how many different faces win a sample of each pixel of one frame's sample-face image [s H, s W]."""
    H, W = face.shape[0] // s, face.shape[1] // s
    blocks = np.asarray(face).reshape(H, s, W, s).transpose(0, 2, 1, 3).reshape(H, W, s * s)
    return np.array([[len(set(p[p >= 0])) for p in row] for row in blocks], np.int64)


# ------------------------------------------------------------------------------------------------ the fixture
FRAMES = ((0, 2, 24, 32), (1, 3, 21, 16), (2, 4, 9, 13), (0, 4, 12, 16))       # (camera type, s, H, W) of golden_render_aa_v1


def clearances(verts, vi, K, Rt, H, W, s):
    """The fixture's statement about one frame on its s H x s W sample grid through K': {"e_proj", "edge_clearance", "e_depth",
    "depth_clearance", "same_faces", "f64", "f32"} -- the float32 projection and depth errors, the clearances they are compared
    with (render_restatement.edge_clearance / depth_clearance), and whether float32 and float64 give the same sample faces."""
    Ks = scaled_camera(K, s)
    p64, p32 = R.project(verts, Ks, Rt), R.project(verts, Ks, Rt, np.float32)
    out = {"e_proj": float(np.abs(p32[..., :2].astype(np.float64) - p64[..., :2]).max()),
           "edge_clearance": R.edge_clearance(verts, vi, Ks, Rt, s * H, s * W)}
    f64 = sample_fragments(verts, vi, K, Rt, H, W, s, runner_up=True)
    f32 = sample_fragments(verts, vi, K, Rt, H, W, s, dtype=np.float32)
    hit = f64["face"] >= 0
    out["same_faces"] = bool(np.array_equal(f32["face"], f64["face"]))
    out["e_depth"] = float((np.abs(f32["depth"][hit].astype(np.float64) - f64["depth"][hit]) / f64["depth"][hit]).max()) if hit.any() else 0.0
    out["depth_clearance"] = R.depth_clearance(f64)
    out["f64"], out["f32"] = f64, f32
    return out
