"""A numpy restatement of the rendering formulas (audio2photoreal_amd/render.py), written from the mathematics: the pinhole
projection, the z-buffer rasterisation rule, perspective-correct barycentrics, attribute interpolation and the border-padded
bilinear texture sample.  Test infrastructure: the yardstick of tests/test_render_hip.py and tests/test_render_cpu.py, and what
tests/golden/make_golden_render.py builds its scene with.

Every numeric function takes `dtype` (float64 by default): all inputs are cast to it and every operation runs in it.  The float32
run against the float64 run is the rounding error float32 arithmetic makes on a scene: the allowance of the GPU tests.

The rule.  p = R x + t; u = fx (x / z) + skew (y / z) + cx, v = fy (y / z) + cy.  The pixel at row i, column j has centre (j + 0.5,
i + 0.5).  A face with a corner at z < near is dropped whole; a face of zero screen area covers nothing; otherwise it covers a
centre that is inside or on the boundary of the projected triangle (edge functions all >= 0 or all <= 0).  With w_k the edge
function opposite corner k and q_k = w_k / z_k, the depth at the centre is area / (q0 + q1 + q2) and the perspective-correct
barycentrics are q_k / (q0 + q1 + q2).  A depth that is not a positive finite number covers nothing.  The smallest depth wins; of
equal depths the lowest face index."""
import numpy as np

from surface_restatement import make_frames, make_surface, nerr  # noqa: F401  (re-exported for the tests)

NEAR = 1e-3


# ------------------------------------------------------------------------------------------------ cameras
def look_at(eye, target, up, height, width, fov_degrees, dtype=np.float64):
    """(K [3, 3], Rt [3, 4]) of a pinhole camera at `eye` looking at `target`, OpenCV axes (x right, y down, z forward); the
    vertical field of view is fov_degrees, the principal point the image centre (width / 2, height / 2), square pixels."""
    eye, target, up = (np.asarray(a, np.float64) for a in (eye, target, up))
    z = target - eye
    z = z / np.linalg.norm(z)
    x = np.cross(z, up)
    x = x / np.linalg.norm(x)
    y = np.cross(z, x)
    R = np.stack([x, y, z])
    f = 0.5 * height / np.tan(np.radians(fov_degrees) / 2)
    K = np.array([[f, 0, width / 2], [0, f, height / 2], [0, 0, 1]])
    return K.astype(dtype), np.concatenate([R, (-R @ eye)[:, None]], 1).astype(dtype)


def project(verts, K, Rt, dtype=np.float64):
    """verts [N, V, 3], K [N or 1, 3, 3], Rt [N or 1, 3, 4] -> [N, V, 3] holding (u, v, z_camera)."""
    x, K, Rt = np.asarray(verts, dtype), np.asarray(K, dtype), np.asarray(Rt, dtype)
    K, Rt = np.broadcast_to(K, (len(x), 3, 3)), np.broadcast_to(Rt, (len(x), 3, 4))
    row = lambda r: ((Rt[:, r, 0, None] * x[..., 0] + Rt[:, r, 1, None] * x[..., 1]) + Rt[:, r, 2, None] * x[..., 2]) + Rt[:, r, 3, None]
    xc, yc, zc = row(0), row(1), row(2)
    with np.errstate(divide="ignore", invalid="ignore"):
        xn, yn = xc / zc, yc / zc
        u = (K[:, 0, 0, None] * xn + K[:, 0, 1, None] * yn) + K[:, 0, 2, None]
        v = K[:, 1, 1, None] * yn + K[:, 1, 2, None]
    return np.stack([u, v, zc], -1)


def camera_centre(Rt, dtype=np.float64):
    """[N, 3] = -R^T t of Rt [N, 3, 4]: the camera position in world coordinates."""
    Rt = np.asarray(Rt, dtype).reshape(-1, 3, 4)
    return -np.einsum("nrc,nr->nc", Rt[:, :, :3], Rt[:, :, 3]).astype(dtype)


# ------------------------------------------------------------------------------------------------ the z-buffer
def _face_pixels(a, b, c, H, W, dtype):
    """(rows, columns, w0, w1, w2, inside) over the pixels whose centre lies in the corners' box; None when there are none."""
    cj, ci = np.arange(W).astype(dtype) + dtype(0.5), np.arange(H).astype(dtype) + dtype(0.5)
    lo, hi = np.minimum(np.minimum(a, b), c), np.maximum(np.maximum(a, b), c)
    js, is_ = np.nonzero((cj >= lo[0]) & (cj <= hi[0]))[0], np.nonzero((ci >= lo[1]) & (ci <= hi[1]))[0]
    if not js.size or not is_.size:
        return None
    px, py = cj[js][None, :], ci[is_][:, None]
    w0 = (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])            # edge a-b: the weight of c
    w1 = (c[0] - b[0]) * (py - b[1]) - (c[1] - b[1]) * (px - b[0])            # edge b-c: the weight of a
    w2 = (a[0] - c[0]) * (py - c[1]) - (a[1] - c[1]) * (px - c[0])            # edge c-a: the weight of b
    inside = ((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0))
    return is_, js, w0, w1, w2, inside


def kept_faces(proj_n, vi, near=NEAR):
    """The faces of one frame that can cover anything: every corner at z >= near and a screen area other than 0."""
    p = proj_n[np.asarray(vi)]
    a, b, c = p[:, 0], p[:, 1], p[:, 2]
    area = (b[:, 0] - a[:, 0]) * (c[:, 1] - a[:, 1]) - (b[:, 1] - a[:, 1]) * (c[:, 0] - a[:, 0])
    with np.errstate(invalid="ignore"):
        return np.nonzero((p[:, :, 2] >= proj_n.dtype.type(near)).all(1) & (np.abs(area) > 0))[0]


def rasterize(verts, vi, K, Rt, H, W, near=NEAR, dtype=np.float64, runner_up=False):
    """{"face" [N, H, W] int64 (-1: background), "bary" [N, H, W, 3] perspective-correct (0), "depth" [N, H, W] (0)}; with
    runner_up also "second" [N, H, W]: the depth of the nearest other covering face (inf where there is none)."""
    vi = np.asarray(vi)
    proj = project(verts, K, Rt, dtype)
    N = len(proj)
    face = np.full((N, H, W), -1, np.int64)
    depth, second = np.full((N, H, W), np.inf, dtype), np.full((N, H, W), np.inf, dtype)
    bary = np.zeros((N, H, W, 3), dtype)
    for n in range(N):
        for f in kept_faces(proj[n], vi, near):
            a, b, c = proj[n, vi[f, 0]], proj[n, vi[f, 1]], proj[n, vi[f, 2]]
            got = _face_pixels(a, b, c, H, W, dtype)
            if got is None:
                continue
            is_, js, w0, w1, w2, inside = got
            area = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
            q = np.stack([w1 / a[2], w2 / b[2], w0 / c[2]], -1)
            s = (q[..., 0] + q[..., 1]) + q[..., 2]
            with np.errstate(divide="ignore", invalid="ignore"):
                z = area / s
                hit = inside & (z > 0) & np.isfinite(z)
                block = (n, slice(is_[0], is_[-1] + 1), slice(js[0], js[-1] + 1))
                wins = hit & (z < depth[block])                               # ascending faces, strict: the lowest index keeps a tie
                loses = hit & ~wins
                second[block] = np.where(wins, depth[block], np.where(loses, np.minimum(second[block], z), second[block]))
                depth[block] = np.where(wins, z, depth[block])
                face[block] = np.where(wins, f, face[block])
                bary[block] = np.where(wins[..., None], q / s[..., None], bary[block])
    out = {"face": face, "bary": bary, "depth": np.where(face >= 0, depth, dtype(0))}
    if runner_up:
        out["second"] = second
    return out


def screen_barycentrics(verts, vi, K, Rt, face, H, W, dtype=np.float64):
    """[N, H, W, 3]: the affine (screen-space) barycentrics w_k / (w0 + w1 + w2) of each pixel centre in its face, 0 on background:
    what perspective correction starts from."""
    proj = project(verts, K, Rt, dtype)
    out = np.zeros(face.shape + (3,), dtype)
    for n, i, j in np.argwhere(face >= 0):
        a, b, c = proj[n, np.asarray(vi)[face[n, i, j]]]
        px, py = dtype(j) + dtype(0.5), dtype(i) + dtype(0.5)
        w0 = (b[0] - a[0]) * (py - a[1]) - (b[1] - a[1]) * (px - a[0])
        w1 = (c[0] - b[0]) * (py - b[1]) - (c[1] - b[1]) * (px - b[0])
        w2 = (a[0] - c[0]) * (py - c[1]) - (a[1] - c[1]) * (px - c[0])
        out[n, i, j] = np.array([w1, w2, w0]) / ((w0 + w1) + w2)
    return out


# ------------------------------------------------------------------------------------------------ per-pixel passes
def interpolate(values, vi, face, bary, dtype=np.float64):
    """values [N, V, C] -> [N, C, H, W]: b0 x[i0] + b1 x[i1] + b2 x[i2] with (i0, i1, i2) = vi[face]; 0 on background."""
    values, bary, face = np.asarray(values, dtype), np.asarray(bary, dtype), np.asarray(face)
    hit = face >= 0
    idx = np.asarray(vi)[np.where(hit, face, 0)]                              # [N, H, W, 3]
    n = np.arange(len(values))[:, None, None]
    x = [values[n, idx[..., k]] for k in range(3)]                            # each [N, H, W, C]
    out = (bary[..., 0, None] * x[0] + bary[..., 1, None] * x[1]) + bary[..., 2, None] * x[2]
    return np.ascontiguousarray(np.where(hit[..., None], out, dtype(0)).transpose(0, 3, 1, 2))


def sample_texture(tex, vt, vti, face, bary, flip_uv=False, dtype=np.float64):
    """tex [N or 1, C, Ht, Wt] -> [N, C, H, W]: the bilinear sample (border padding) at x = u (Wt - 1), y = v (Ht - 1) with the
    pixel's uv = b0 vt[t0] + b1 vt[t1] + b2 vt[t2], (t0, t1, t2) = vti[face], v <- 1 - v when flip_uv; taps nw, ne, sw, se summed
    in that order; 0 on background."""
    tex, vt, bary, face = np.asarray(tex, dtype), np.asarray(vt, dtype), np.asarray(bary, dtype), np.asarray(face)
    N = len(face)
    tex = np.broadcast_to(tex, (N,) + tex.shape[1:])
    Ht, Wt = tex.shape[2:]
    hit = face >= 0
    t = vt[np.asarray(vti)[np.where(hit, face, 0)]]                           # [N, H, W, 3, 2]
    uv = (bary[..., 0, None] * t[..., 0, :] + bary[..., 1, None] * t[..., 1, :]) + bary[..., 2, None] * t[..., 2, :]
    u, v = uv[..., 0], uv[..., 1]
    if flip_uv:
        v = dtype(1) - v
    x = np.minimum(np.maximum(u * dtype(Wt - 1), dtype(0)), dtype(Wt - 1))
    y = np.minimum(np.maximum(v * dtype(Ht - 1), dtype(0)), dtype(Ht - 1))
    xw, yn = np.floor(x), np.floor(y)
    w, s = x - xw, y - yn
    e, nn = dtype(1) - w, dtype(1) - s
    n = np.arange(N)[:, None, None]
    out = None
    for dy, dx, wt in ((0, 0, nn * e), (0, 1, nn * w), (1, 0, s * e), (1, 1, s * w)):
        xi, yi = (xw + dx).astype(np.int64), (yn + dy).astype(np.int64)
        ok = (xi <= Wt - 1) & (yi <= Ht - 1)
        tap = np.where(ok[..., None], tex[n, :, np.minimum(yi, Ht - 1), np.minimum(xi, Wt - 1)], dtype(0)) * wt[..., None]
        out = tap if out is None else out + tap
    return np.ascontiguousarray(np.where(hit[..., None], out, dtype(0)).transpose(0, 3, 1, 2))


# ------------------------------------------------------------------------------------------------ clearances
def edge_distance(verts, vi, K, Rt, H, W, near=NEAR):
    """[N, H, W] float64: the distance in pixels from each pixel centre to the nearest projected edge of a kept face of its frame;
    inf for a centre more than a pixel outside the box of every edge (it is then at least a pixel away from all of them)."""
    vi = np.asarray(vi)
    proj = project(verts, K, Rt)
    out = np.full((len(proj), H, W), np.inf)
    cj, ci = np.arange(W) + 0.5, np.arange(H) + 0.5
    for n in range(len(proj)):
        t = vi[kept_faces(proj[n], vi, near)]
        edges = np.unique(np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), axis=1), axis=0)
        for a, b in proj[n, edges][:, :, :2]:
            lo, hi = np.minimum(a, b) - 1, np.maximum(a, b) + 1
            js, is_ = np.nonzero((cj >= lo[0]) & (cj <= hi[0]))[0], np.nonzero((ci >= lo[1]) & (ci <= hi[1]))[0]
            if not js.size or not is_.size:
                continue
            px, py = cj[js][None, :], ci[is_][:, None]
            ab = b - a
            s = np.clip(((px - a[0]) * ab[0] + (py - a[1]) * ab[1]) / (ab @ ab), 0, 1)
            block = (n, slice(is_[0], is_[-1] + 1), slice(js[0], js[-1] + 1))
            out[block] = np.minimum(out[block], np.sqrt((px - a[0] - s * ab[0]) ** 2 + (py - a[1] - s * ab[1]) ** 2))
    return out


def edge_clearance(verts, vi, K, Rt, H, W, near=NEAR):
    """The smallest distance in pixels (float64) from any pixel centre of the H x W image to any projected edge of a kept face of
    any frame.  Above the float32 error of the projected coordinates, no rule and no precision can disagree on a pixel's cover."""
    return float(edge_distance(verts, vi, K, Rt, H, W, near).min())


def depth_clearance(fragments):
    """The smallest relative gap (second - depth) / depth between the winning face and the runner-up at any covered pixel of a
    rasterize(..., runner_up=True) result; inf when no pixel is covered twice."""
    hit = fragments["face"] >= 0
    if not hit.any():
        return np.inf
    d, s = fragments["depth"][hit].astype(np.float64), fragments["second"][hit].astype(np.float64)
    return float(((s - d) / d).min())


# ------------------------------------------------------------------------------------------------ the fixture scene
SIZES = ((48, 64), (64, 48), (37, 53))      # (H, W) of the three fixture frames, each with its own camera
LAYER_OFFSET = (0.03, -0.02, -0.45)         # the second copy of the sheet, behind the first as the cameras see it
CLEARANCE_FACTOR = 8                        # clearances are this multiple of the measured float32 error


def two_layers(surf):
    """The fixture surface listed twice: {"vi" [2 F, 3], "vt", "vti" [2 F, 3], "n_verts" 2 V}; the copy's vertices follow the
    original's, its faces follow the original's faces and use the same texture coordinates."""
    V = surf["n_verts"]
    return {"vi": np.concatenate([surf["vi"], surf["vi"] + V]), "vt": surf["vt"], "vti": np.concatenate([surf["vti"], surf["vti"]]),
            "n_verts": 2 * V}


def layered_frames(surf, seed, N):
    """[N, 2 V, 3] float32: make_frames of the sheet and the same vertices displaced by LAYER_OFFSET."""
    front = make_frames(surf, seed, N)
    return np.concatenate([front, front + np.asarray(LAYER_OFFSET, np.float32)], 1)
