"""The encode path restated in numpy, dtype-parametrised (float64 is the reference of the GPU tests, float32 measures what the same
formulas lose in single precision): la.LinearWN, ConvDownBlock, FaceDecoderFrontal, FaceEncoder, Encoder, LinearBlendSkinning.
unskinning / LBSModule.unpose -- and, in float32 only, the summation order that a2p_linear_f32 documents.  Layers that earlier
restatements already hold are taken from them."""
import numpy as np

import decoder_restatement as DR
import skinning_restatement as SR
import surface_restatement as SFR
import texture_restatement as TR
from surface_restatement import nerr  # noqa: F401  (part of this module's surface)

SLOPE = 0.2
KSLICE = 256


# ------------------------------------------------------------------------------------------------ the linear layer
def linear(x, w, bias=None, slope=None, dtype=np.float64):
    """act(x w^T + bias)."""
    v = np.asarray(x, dtype) @ np.asarray(w, dtype).T
    if bias is not None:
        v = v + np.asarray(bias, dtype)
    return v if slope is None else DR.lrelu(v, slope, dtype)


def _fma32(a, b, c):
    """float32 fmaf(a, b, c): the product of two float32 is exact in float64; the sum is rounded to float64 and then to float32
    (a double rounding that differs from the fused result in rare ties only)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def linear_rule32(x, w, bias=None, slope=None):
    """a2p_linear_f32's documented order in float32: per slice of 256 inputs one fmaf chain from 0 with i ascending; the slices
    added in ascending order starting from slice 0; then the bias; then LeakyReLU."""
    x, w = np.asarray(x, np.float32), np.asarray(w, np.float32)
    N, I = x.shape
    v = None
    for s0 in range(0, I, KSLICE):
        a = np.zeros((N, w.shape[0]), np.float32)
        for i in range(s0, min(I, s0 + KSLICE)):
            a = _fma32(x[:, i:i + 1], w[None, :, i], a)
        v = a if v is None else (v + a).astype(np.float32)
    if bias is not None:
        v = (v + np.asarray(bias, np.float32)).astype(np.float32)
    if slope is not None:
        v = np.where(v >= 0, v, (np.float32(slope) * v).astype(np.float32))
    return v


# ------------------------------------------------------------------------------------------------ ConvDownBlock
def down3(h, x, w2, b2, wr, br=None, slope=SLOPE, dtype=np.float64, resize_offset=0):
    """lrelu(conv2(h) + b2) + conv_resize(x): conv2 3 x 3, stride 2, padding 1 (the stride-1 convolution at the even positions);
    conv_resize 1 x 1, stride 2.  In float32 the sums run in the order a2p_conv2d_down3_ub documents (down3_rule32): what that
    order loses is the yardstick, not what numpy's blocked einsum loses.  resize_offset = 1 is a deliberate miswiring for the
    vacuity checks."""
    if dtype is np.float32 and not resize_offset:
        return down3_rule32(h, x, w2, b2, wr, br, slope)
    v = DR.conv2d(h, w2, 1, dtype)[:, :, ::2, ::2] + np.asarray(b2, dtype)[None]
    v = DR.lrelu(v, slope, dtype)
    wr = np.asarray(wr, dtype).reshape(np.shape(wr)[0], -1)
    xs = np.asarray(x, dtype)[:, :, resize_offset::2, resize_offset::2]
    r = np.zeros_like(v)
    r[:, :, :xs.shape[2], :xs.shape[3]] = np.einsum("oc,nchw->nohw", wr, xs)
    if br is not None:
        r = r + np.asarray(br, dtype)[None, :, None, None]
    return v + r


def down3_rule32(h, x, w2, b2, wr, br=None, slope=SLOPE):
    """a2p_conv2d_down3_ub's documented order in float32, every product and sum rounded: one chain over ci ascending, then ky, kx
    row-major; + b2; LeakyReLU; the 1 x 1 branch as its own chain over ci ascending; + (br + that)."""
    f32 = np.float32
    h, x, w2 = np.asarray(h, f32), np.asarray(x, f32), np.asarray(w2, f32)
    wr = np.asarray(wr, f32).reshape(w2.shape[0], -1)
    N, C, Hs, Ws = h.shape
    H, W = (Hs - 1) // 2 + 1, (Ws - 1) // 2 + 1
    hp = np.zeros((N, C, Hs + 2, Ws + 2), f32)
    hp[:, :, 1:1 + Hs, 1:1 + Ws] = h
    v, r = np.zeros((N, w2.shape[0], H, W), f32), np.zeros((N, w2.shape[0], H, W), f32)
    for ci in range(C):
        for ky in range(3):
            for kx in range(3):
                v = v + w2[None, :, ci, ky, kx, None, None] * hp[:, None, ci, ky:ky + 2 * H:2, kx:kx + 2 * W:2]
        r = r + wr[None, :, ci, None, None] * x[:, None, ci, ::2, ::2]
    v = v + np.asarray(b2, f32)[None]
    v = np.where(v >= 0, v, f32(slope) * v)
    if br is not None:
        r = np.asarray(br, f32)[None, :, None, None] + r
    assert v.dtype == f32 and r.dtype == f32
    return v + r


def down_block(params, name, x, dtype=np.float64, **kw):
    """ConvDownBlock.forward."""
    h = DR.layer(x, DR.weight_of(params, f"{name}.conv1", dtype), params[f"{name}.conv1.bias"], slope=SLOPE, dtype=dtype)
    return down3(h, x, DR.weight_of(params, f"{name}.conv2", dtype), params[f"{name}.conv2.bias"],
                 DR.weight_of(params, f"{name}.conv_resize", dtype), params[f"{name}.conv_resize.bias"], SLOPE, dtype, **kw)


def lin(params, name, x, slope=None, dtype=np.float64):
    return linear(x, DR.weight_of(params, name, dtype), params[f"{name}.bias"], slope, dtype)


# ------------------------------------------------------------------------------------------------ the networks
def resize_corners(m, size, dtype=np.float64):
    """F.interpolate(m[None, None], size, mode="bilinear", align_corners=True) of a map [H, W]."""
    return DR.upsample(np.asarray(m, dtype)[None, None], size, dtype)[0, 0]


def face_decoder(params, layers, frontal_view, codes, dtype=np.float64):
    """FaceDecoderFrontal.forward; layers: the names of the transposed layers in order."""
    N = len(codes)
    enc = lin(params, "encmod.0", codes, SLOPE, dtype)
    geom = lin(params, "geommod.0", enc, None, dtype)
    view = lin(params, "viewmod.0", np.broadcast_to(np.asarray(frontal_view, dtype), (N, np.size(frontal_view))), SLOPE, dtype)
    y = lin(params, "texmod2.0", np.concatenate([enc, view], 1), SLOPE, dtype)
    c0 = np.shape(params[f"{layers[0]}.weight_v"])[0]
    s0 = int(round(np.sqrt(y.shape[1] / c0)))
    y = y.reshape(N, c0, s0, s0)
    for i, name in enumerate(layers):
        y = TR.up_layer(y, TR.weight_of(params, name, dtype), params[f"{name}.bias"], SLOPE if i + 1 < len(layers) else None, dtype=dtype)
    tex = dtype(255) * ((y + np.asarray(params["bias"], dtype)[None]) + dtype(0.5))
    return {"face_geom": geom.reshape(N, -1, 3), "face_tex_raw": y, "face_tex": tex}


def tex_cond(raw, bias, mask, dtype=np.float64, wiring=""):
    """(F.interpolate(255 (raw + bias + 0.5), mask.shape, "bilinear") / 255 - 0.5) * mask.  wiring: a deliberate miswiring --
    "corners" (align_corners=True), "no_half" (- 0.5 missing) or "no_mask"."""
    tex = dtype(255) * ((np.asarray(raw, dtype) + np.asarray(bias, dtype)[None]) + dtype(0.5))
    mask = np.asarray(mask, dtype)
    r = DR.upsample(tex, mask.shape, dtype) if wiring == "corners" else TR.resize(tex, mask.shape, dtype)
    v = r / dtype(255) - (dtype(0) if wiring == "no_half" else dtype(0.5))
    return v if wiring == "no_mask" else v * mask


def face_encoder(params, blocks, mask, face_geom, raw, bias, logvar_scale=0.1, dtype=np.float64, wiring=""):
    """FaceEncoder.forward in eval mode; mask: the resized tex_cond_mask.  wiring "swap" exchanges mu and logvar; "resize_odd"
    reads conv_resize at [2 y + 1]; the others are tex_cond's."""
    N = len(raw)
    cond = tex_cond(raw, bias, mask, dtype, wiring)
    x = cond
    for name in blocks:
        x = down_block(params, name, x, dtype, resize_offset=int(wiring == "resize_odd"))
    g = lin(params, "geommod.0", np.asarray(face_geom, dtype).reshape(N, -1), SLOPE, dtype)
    j = lin(params, "jointmod.0", np.concatenate([x.reshape(N, -1), g], 1), SLOPE, dtype)
    mu_name, lv_name = ("logvar", "mu") if wiring == "swap" else ("mu", "logvar")
    mu = lin(params, mu_name, j, None, dtype)
    return {"face_embs": mu, "face_embs_mu": mu, "face_embs_logvar": dtype(logvar_scale) * lin(params, lv_name, j, None, dtype),
            "face_tex_cond": cond}


def body_encoder(params, blocks, mask, index_image, bary_image, uv_size, verts_unposed, logvar_scale=0.1, dtype=np.float64):
    """Encoder.forward in eval mode; mask: the 0 / 1 map at uv_size."""
    N = len(verts_unposed)
    x = TR.resize(SFR.to_uv(verts_unposed, index_image, bary_image, dtype), (uv_size, uv_size), dtype) * np.asarray(mask, dtype)
    for name in blocks:
        x = down_block(params, name, x, dtype)
    x = x.reshape(N, -1)
    mu = lin(params, "mu", x, None, dtype)
    return {"embs": mu, "embs_mu": mu, "embs_logvar": dtype(logvar_scale) * lin(params, "logvar", x, None, dtype)}


# ------------------------------------------------------------------------------------------------ unposing
def blended(skel, mats, dtype=np.float64):
    """[N, V, 3, 4]: sum_k w[v, k] mats[n, idx[v, k]]."""
    idx, w = np.asarray(skel["skin_indices"]), np.asarray(skel["skin_weights"], dtype)
    return (np.asarray(mats, dtype)[:, idx] * w[None, :, :, None, None]).sum(2)


def unpose(skel, poses, scales, verts, template_verts=None, global_scaling=1.0, dtype=np.float64, subtract=True):
    """LBSModule.unpose: unskinning(verts / global_scaling) - template, the inverse by numpy's LU like the reference's
    Tensor.inverse().  subtract=False is a deliberate miswiring."""
    base = np.asarray(skel["rest_vertices"] if template_verts is None else template_verts, dtype)
    M = blended(skel, SR.transforms(skel, poses, scales, dtype), dtype)
    p = np.asarray(verts, dtype) / np.asarray(global_scaling, dtype)
    out = np.einsum("nvrc,nvc->nvr", np.linalg.inv(M[..., :3]).astype(dtype), p - M[..., 3]).astype(dtype)
    return out - base if subtract else out


def blend_determinants(skel, poses, scales):
    """float64 [N, V]: det of the 3 x 3 part of every blended matrix."""
    return np.linalg.det(blended(skel, SR.transforms(skel, poses, scales))[..., :3])


# ------------------------------------------------------------------------------------------------ the fixture
def random_layer(rs, params, name, shape, bias_shape, g_axis=0):
    TR.random_layer(rs, params, name, shape, bias_shape, g_axis)


def down_params(rs, params, name, c_in, c_out, size):
    random_layer(rs, params, f"{name}.conv_resize", (c_out, c_in, 1, 1), (c_out,))
    random_layer(rs, params, f"{name}.conv1", (c_in, c_in, 3, 3), (c_in, size, size))
    random_layer(rs, params, f"{name}.conv2", (c_out, c_in, 3, 3), (c_out, size // 2, size // 2))


FACE_DEC = dict(n_latent=12, n_hidden=10, V=7, n_view=3, ladder=((6, 5), (5, 4), (4, 3)), s0=4)       # texture 4 -> 32
FACE_ENC = dict(uv_size=16, ladder=((3, 4), (4, 6)), n_geom=9, n_joint=11, n_embs=5)                   # 16 -> 4
BODY_ENC = dict(uv_size=16, ladder=((3, 8), (8, 6)), n_embs=7, surface_uv=24)                           # 16 -> 4
N_FRAMES = 2


def face_decoder_params(cfg, seed):
    rs, p = np.random.RandomState(seed), {}
    H, c0, s = cfg["n_hidden"], cfg["ladder"][0][0], cfg["s0"]
    random_layer(rs, p, "encmod.0", (H, cfg["n_latent"]), (H,))
    random_layer(rs, p, "geommod.0", (3 * cfg["V"], H), (3 * cfg["V"],))
    random_layer(rs, p, "viewmod.0", (cfg["n_view"], 3), (cfg["n_view"],))
    random_layer(rs, p, "texmod2.0", (c0 * s * s, H + cfg["n_view"]), (c0 * s * s,))
    for i, (a, b) in enumerate(cfg["ladder"]):
        random_layer(rs, p, f"texmod.{2 * i}", (a, b, 4, 4), (b, 2 * s, 2 * s), g_axis=1)
        s *= 2
    p["bias"] = (0.1 * rs.randn(cfg["ladder"][-1][1], s, s)).astype(np.float32)
    return p


def face_encoder_params(cfg, n_vert_in, seed):
    rs, p = np.random.RandomState(seed), {}
    s = cfg["uv_size"]
    for i, (a, b) in enumerate(cfg["ladder"]):
        down_params(rs, p, f"conv_blocks.{i}", a, b, s)
        s //= 2
    n_tex = cfg["ladder"][-1][1] * s * s
    random_layer(rs, p, "geommod.0", (cfg["n_geom"], n_vert_in), (cfg["n_geom"],))
    random_layer(rs, p, "jointmod.0", (cfg["n_joint"], n_tex + cfg["n_geom"]), (cfg["n_joint"],))
    random_layer(rs, p, "mu", (cfg["n_embs"], cfg["n_joint"]), (cfg["n_embs"],))
    random_layer(rs, p, "logvar", (cfg["n_embs"], cfg["n_joint"]), (cfg["n_embs"],))
    return p


def body_encoder_params(cfg, seed):
    rs, p = np.random.RandomState(seed), {}
    s = cfg["uv_size"]
    for i, (a, b) in enumerate(cfg["ladder"]):
        down_params(rs, p, "verts_conv" if i == 0 else f"joint_conv_blocks.{i - 1}", a, b, s)
        s //= 2
    n_flat = cfg["ladder"][-1][1] * s * s
    random_layer(rs, p, "mu", (cfg["n_embs"], n_flat), (cfg["n_embs"],))
    random_layer(rs, p, "logvar", (cfg["n_embs"], n_flat), (cfg["n_embs"],))
    return p


def face_layers(cfg):
    return [f"texmod.{2 * i}" for i in range(len(cfg["ladder"]))]


def face_blocks(cfg):
    return [f"conv_blocks.{i}" for i in range(len(cfg["ladder"]))]


def body_blocks(cfg):
    return ["verts_conv"] + [f"joint_conv_blocks.{i}" for i in range(len(cfg["ladder"]) - 1)]


def make_fixture(seed=31):
    """Small ladders of the three networks (the depth is read from the state dict), the fixture mesh of surface_restatement, a
    random skeleton over its vertices with moderate poses, and 2 frames of inputs."""
    rs = np.random.RandomState(seed)
    surf = SFR.make_surface()
    surf["v2uv"] = SFR.compute_v2uv(surf["n_verts"], surf["vi"], surf["vti"])
    V = surf["n_verts"]
    skel = SR.make_skeleton(seed + 4, 6, V, 4, P_pos=16, P_scale=3)
    yy, xx = np.mgrid[0:20, 0:20]
    soft = np.clip(1.5 - np.hypot(yy - 9.5, xx - 9.5) / 6.0, 0.0, 1.0)
    assets = {"face_frontal_view": rs.randn(3).astype(np.float32),
              "mugsy_face_mask": np.repeat(soft[:, :, None], 3, 2).astype(np.float32),
              "face_mask": (rs.rand(24, 24) < 0.3).astype(np.float32)}
    return {"face_dec": face_decoder_params(FACE_DEC, seed + 1), "face_enc": face_encoder_params(FACE_ENC, 3 * FACE_DEC["V"], seed + 2),
            "body_enc": body_encoder_params(BODY_ENC, seed + 3), "assets": assets, "surf": surf, "skel": skel,
            "template": surf["rest"].astype(np.float32), "global_scaling": np.float32(10.0),
            "poses": (rs.randn(N_FRAMES, 16) * 0.3).astype(np.float32), "scales": np.zeros((1, 3), np.float32),
            "codes": rs.randn(N_FRAMES, FACE_DEC["n_latent"]).astype(np.float32),
            "displacement": (0.05 * rs.randn(N_FRAMES, V, 3)).astype(np.float32)}


# ------------------------------------------------------------------------------------------------ the reference-size fixture
# The reference's classes fix the texture at 1024 x 1024, the hidden width at 256 and both encoders at 512 x 512 with their full
# ladders; what they leave free is small here: 16 face codes, 24 face vertices, 6 and 5 embedding values, 2 frames.
_TEX_LADDER = ((256, 256), (256, 128), (128, 128), (128, 64), (64, 64), (64, 32), (32, 8), (8, 3))
REF_FACE_DEC = dict(n_latent=16, n_hidden=256, V=24, n_view=8, ladder=_TEX_LADDER, s0=4)
REF_FACE_ENC = dict(uv_size=512, ladder=((3, 4), (4, 8), (8, 16), (16, 32), (32, 64), (64, 128), (128, 128)), n_geom=256, n_joint=512, n_embs=6)
REF_BODY_ENC = dict(uv_size=512, ladder=((3, 8), (8, 16), (16, 32), (32, 32), (32, 64), (64, 128), (128, 128)), n_embs=5, surface_uv=64)
REF_ROWS = slice(37, None, 128)     # the rows kept of a map with 128 rows or more


def make_reference_fixture(seed=41):
    """The networks at the sizes the reference's classes fix, as data: seeded state dicts (legacy RandomState streams, which numpy
    freezes), assets, the fixture mesh with its UV images at 64 x 64, a 12-joint skeleton with moderate poses and 2 frames."""
    rs = np.random.RandomState(seed)
    surf = SFR.make_surface()
    surf["v2uv"] = SFR.compute_v2uv(surf["n_verts"], surf["vi"], surf["vti"])
    V, U = surf["n_verts"], REF_BODY_ENC["surface_uv"]
    index_image, bary_image, _ = SFR.uv_images(surf, U)
    yy, xx = np.mgrid[0:64, 0:64]
    soft = np.clip(1.5 - np.hypot(yy - 31.5, xx - 31.5) / 20.0, 0.0, 1.0)
    assets = {"face_frontal_view": rs.randn(3).astype(np.float32), "mugsy_face_mask": np.repeat(soft[:, :, None], 3, 2).astype(np.float32),
              "face_mask": (rs.rand(32, 32) < 0.3).astype(np.float32)}
    return {"face_dec": face_decoder_params(REF_FACE_DEC, seed + 1), "face_enc": face_encoder_params(REF_FACE_ENC, 3 * REF_FACE_DEC["V"], seed + 2),
            "body_enc": body_encoder_params(REF_BODY_ENC, seed + 3), "assets": assets, "surf": surf,
            "index_image": index_image.astype(np.int32), "bary_image": bary_image.astype(np.float32),
            "skel": SR.make_skeleton(seed + 4, 12, V, 4, P_pos=104, P_scale=12), "template": surf["rest"].astype(np.float32),
            "global_scaling": np.array([10.0, 9.5, 10.5], np.float32), "poses": (rs.randn(N_FRAMES, 104) * 0.3).astype(np.float32),
            "scales": (rs.randn(1, 12) * 0.1).astype(np.float32), "codes": rs.randn(N_FRAMES, REF_FACE_DEC["n_latent"]).astype(np.float32),
            "displacement": (0.05 * rs.randn(N_FRAMES, V, 3)).astype(np.float32)}


def reference_forward(fx, dtype=np.float64):
    """Every output the golden file stores, restated: {"face_dec/..", "face_enc/..", "body_enc/..", "unpose/verts_unposed"}.  The
    face encoder reads the face decoder's own outputs rounded to float32, as the reference's modules pass them on."""
    a, out = fx["assets"], {}
    dec = face_decoder(fx["face_dec"], face_layers(REF_FACE_DEC), a["face_frontal_view"], fx["codes"], dtype)
    out.update({f"face_dec/{k}": v for k, v in dec.items()})
    geom32, raw32 = fx.get("face_geom32"), fx.get("face_tex_raw32")
    if geom32 is None:                                                         # the golden file's choice: this decoder's float64 outputs, rounded
        dec64 = dec if dtype is np.float64 else face_decoder(fx["face_dec"], face_layers(REF_FACE_DEC), a["face_frontal_view"], fx["codes"])
        geom32, raw32 = dec64["face_geom"].astype(np.float32), dec64["face_tex_raw"].astype(np.float32)
    mask = resize_corners(a["mugsy_face_mask"][..., 0], (512, 512))
    enc = face_encoder(fx["face_enc"], face_blocks(REF_FACE_ENC), mask, geom32, raw32, fx["face_dec"]["bias"], dtype=dtype)
    out.update({f"face_enc/{k}": v for k, v in enc.items()})
    body_mask = (TR.resize(1.0 - a["face_mask"].astype(np.float64), (512, 512)) != 0).astype(np.float64)
    body = body_encoder(fx["body_enc"], body_blocks(REF_BODY_ENC), body_mask, fx["index_image"], fx["bary_image"], 512, fx["displacement"], dtype=dtype)
    out.update({f"body_enc/{k}": v for k, v in body.items()})
    posed32 = fx.get("posed32")
    if posed32 is None:
        posed32 = SR.pose_vertices(fx["skel"], fx["poses"], fx["scales"], fx["displacement"], fx["template"], fx["global_scaling"]).astype(np.float32)
    out["unpose/verts_unposed"] = unpose(fx["skel"], fx["poses"], fx["scales"], posed32, fx["template"], fx["global_scaling"], dtype)
    return out


def fingerprint(params):
    """{key: float64 sum of the array}: what the golden file stores of a generated state dict."""
    return {k: float(np.asarray(v, np.float64).sum()) for k, v in params.items()}
