"""The body renderer end to end on the MI355X -- BodyDecoder.forward, pose_vertices, BodyTexture.forward, BodyRasterizer,
linear_to_display, render_rgb_motion and the command line of audio2photoreal_amd/texture.py -- against the float64 chain of
tests/body_chain_restatement.py on the scene of tests/golden/golden_body_chain_v1.npz.

Gate: the normalised error of every output (max |difference| / max |value|) is at most 4 x max(e, 2^-24), as in
test_texture_hip.py.  e is the reference's own float32 error on the stage (e_ref/*) where its modules provide the stage, else the
float32 chain's error against the float64 chain (e/*), both from the golden file.  Images (depth, render, rgb) are gated over the
kept pixels: covered in the float64 chain and outside its `excluded` mask, which holds the pixels within 8 x e_proj of a projected
edge or with a runner-up within 8 x e_depth of the winner; outside that mask the face images must be equal.  No tolerance is
written down; every measured value goes to record("chain_...") beside its allowance."""
import json
import os

import numpy as np
import pytest
import torch

import body_chain_restatement as B
import skinning_restatement as SR
from audio2photoreal_amd import decoder as D
from audio2photoreal_amd import render as RD
from audio2photoreal_amd import skinning as SK
from audio2photoreal_amd import surface as S
from audio2photoreal_amd import texture as T
from conftest import record

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def want():
    """The golden file, the scene, its float64 chain (once, about 15 s on the CPU), the kept pixels and the allowances."""
    gold = np.load(os.path.join(ROOT, "tests", "golden", "golden_body_chain_v1.npz"))
    scene = B.draw_scene(int(gold["seed"]), int(gold["draw"]))
    c64 = B.chain(scene)
    assert np.array_equal(gold["face"], c64["face"].astype(np.int16)), "the float64 chain here is not the one the golden file was made from"
    ex = np.unpackbits(gold["excluded"])[:c64["face"].size].reshape(c64["face"].shape).astype(bool)
    return {"gold": gold, "scene": scene, "c64": c64, "excluded": ex, "kept": (c64["face"] >= 0) & ~ex, "allowance": B.allowances(gold)}


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


@pytest.fixture(scope="module")
def body(dev, want):
    """The product's objects on the scene and one run of the stages by hand."""
    sc = want["scene"]
    s, skel = sc["surf"], sc["skel"]
    surface = S.BodySurface.from_arrays(s["vi"], s["vt"], s["vti"], n_verts=s["n_verts"], v2uv=s["v2uv"], uv_size=B.UV)
    state = {**{"decoder." + k: v for k, v in sc["params"].items()}, **sc["tex_state"]}
    assets = {**sc["assets"], **sc["tex_assets"]}
    decoder = D.BodyDecoder.from_state_dict(state, assets, surface, **sc["cfg"])
    texture = T.BodyTexture.from_state_dict(state, assets, surface, **sc["tex_cfg"])
    sk = SK.BodySkeleton.from_arrays(skel["parents"], skel["pre_rotation"], skel["joint_offset"], skel["transform"], skel["transform_offsets"],
                                     16, 3, skel["rest_vertices"], skel["skin_indices"], skel["skin_weights"], template_verts=sc["template"],
                                     lbs_scale=sc["lbs_scale"], global_scaling=sc["global_scaling"])
    H, W = sc["size"]
    b = {"decoder": decoder, "texture": texture, "skeleton": sk, "surface": surface, "rasterizer": RD.BodyRasterizer(surface, H, W),
         "state": state, "assets": assets, "frames": up(sc["motion"], dev), "embs": up(sc["embs"], dev), "face": up(sc["face_embs"], dev),
         "K": up(sc["K"], dev), "Rt": up(sc["Rt"], dev)}
    with torch.cuda.device(dev):
        b["preds"] = decoder.forward(b["frames"], b["embs"], b["face"])
        b["verts"] = sk.pose_vertices(b["frames"], verts_unposed=b["preds"]["geom_delta_rec"])
        b["tex"] = texture.forward(b["verts"], b["preds"]["tex_mean_rec"], RD.camera_centre(b["Rt"]), motion=b["frames"])
        b["frag"] = b["rasterizer"].rasterize(b["verts"], b["K"], b["Rt"])
        b["render"] = b["rasterizer"].sample_texture(b["frag"], b["tex"]["tex_rec"])
        b["rgb"] = T.render_rgb_motion(decoder, texture, sk, b["rasterizer"], b["frames"], b["embs"], b["face"], b["K"], b["Rt"])
    return b


def measure(name, got, wanted, allowance, mask=None):
    """Record one output's normalised error beside its allowance and return it; images over the pixels of `mask` only."""
    got = got.detach().cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == wanted.shape, (name, got.shape, wanted.shape)
    err = B.nerr(got, wanted) if mask is None else B.nerr(B.over(got, mask), B.over(wanted, mask))
    record(name, err=err, allowance=allowance)
    return err


def gate(name, got, wanted, allowance, mask=None):
    err = measure(name, got, wanted, allowance, mask)
    assert np.isfinite(err) and err <= allowance, (name, err, allowance)


# ------------------------------------------------------------------------------------------------ the stages
def test_stages_against_the_chain(want, body):
    c, a = want["c64"], want["allowance"]
    gate("chain_geom_delta_rec", body["preds"]["geom_delta_rec"], c["geom_delta_rec"], a["geom_delta_rec"])
    gate("chain_verts", body["verts"], c["verts"], a["verts"])
    tex = body["tex"]
    assert set(tex) == {"tex_rec", "tex_view_rec", "cond_view", "shadow_map"}
    gate("chain_cond_view", tex["cond_view"], c["cond_view"], a["cond_view"])
    gate("chain_cond_view_cos", tex["cond_view"][:, :1], c["cond_view"][:, :1], a["view_cos_uv"])
    gate("chain_cond_view_mean", tex["cond_view"][:, 1:], c["tex_mean_rec"], a["tex_mean_rec"])
    gate("chain_tex_view_rec", tex["tex_view_rec"], c["tex_view_rec"], a["tex_view_rec"])
    gate("chain_shadow_map", tex["shadow_map"], c["shadow_map"], a["shadow_map"])
    gate("chain_tex_rec", tex["tex_rec"], c["tex_rec"], a["tex_rec"])


def test_rasteriser_on_the_gpu_vertices(want, body):
    c, a, ex, kept = want["c64"], want["allowance"], want["excluded"], want["kept"]
    face = body["frag"]["face"].cpu().numpy()
    differ = face != c["face"]
    for n in range(len(face)):
        record(f"chain_face_frame{n}", differing_inside_excluded=int((differ[n] & ex[n]).sum()), excluded=int(ex[n].sum()),
               excluded_share_of_covered=float((ex[n] & (c["face"][n] >= 0)).sum() / (c["face"][n] >= 0).sum()))
    assert np.array_equal(face[~ex], c["face"][~ex]), f"{int((differ & ~ex).sum())} pixels outside `excluded` show another face"
    gate("chain_depth", body["frag"]["depth"], c["depth"], a["depth"], kept)
    gate("chain_render", body["render"], c["render"], a["render"], kept)
    gate("chain_display", T.linear_to_display(body["render"]), c["rgb"], a["rgb"], kept)
    background = torch.from_numpy(face < 0).to(body["render"].device)
    assert not bool(body["render"].permute(0, 2, 3, 1)[background].any()), "a background pixel of render is not exactly 0"
    assert bool(background.any()) and float(body["render"].abs().max()) > 0


# ------------------------------------------------------------------------------------------------ render_rgb_motion
def rgb_of(body, K=None, Rt=None, frames=slice(None), **kw):
    b = body
    K, Rt = b["K"] if K is None else K, b["Rt"] if Rt is None else Rt
    with torch.cuda.device(b["frames"].device):
        return T.render_rgb_motion(b["decoder"], b["texture"], b["skeleton"], b["rasterizer"], b["frames"][frames], b["embs"][frames], b["face"][frames],
                                   K, Rt, **kw)


def test_render_rgb_motion_with_per_frame_cameras(want, body):
    c, a, kept = want["c64"], want["allowance"], want["kept"]
    whole = body["rgb"]
    assert whole.shape == (3, 3, 96, 128) and whole.dtype == torch.float32
    gate("chain_rgb", whole, c["rgb"], a["rgb"], kept)
    assert float(whole.min()) >= 0 and float(whole.max()) <= 255
    explicit = rgb_of(body, camera_pos=RD.camera_centre(body["Rt"]))          # [3, 3]: one camera position per frame
    gate("chain_rgb_camera_pos", explicit, c["rgb"], a["rgb"], kept)
    assert torch.equal(explicit, whole)
    assert torch.equal(whole, T.linear_to_display(body["render"]))            # and it is the stages by hand, bit for bit


def test_render_rgb_motion_in_chunks_of_one_frame(body):
    calls = []
    forward = body["texture"].forward
    body["texture"].forward = lambda *x, **k: (calls.append((x[0].shape[0], x[2].cpu().numpy().copy())), forward(*x, **k))[1]
    try:
        chunked = rgb_of(body, max_bytes=1)
    finally:
        del body["texture"].forward
    assert [n for n, _ in calls] == [1, 1, 1]
    cams = RD.camera_centre(body["Rt"]).cpu().numpy()
    for n, (_, cam) in enumerate(calls):
        assert np.array_equal(cam, cams[n:n + 1]), f"chunk {n} got another frame's camera position"
    assert torch.equal(chunked, body["rgb"])


def test_rotated_cameras_fail_the_gate(want, body):
    """The GPU test sees what the mutant table claims: each frame with its neighbour's camera misses the gate of rgb."""
    got = rgb_of(body, K=body["K"].roll(1, 0), Rt=body["Rt"].roll(1, 0))
    err = measure("chain_rgb_cameras_rotated", got, want["c64"]["rgb"], want["allowance"]["rgb"], want["kept"])
    assert not err <= want["allowance"]["rgb"], (err, want["allowance"]["rgb"])


@pytest.mark.parametrize("n", [0, 1, 2])
def test_a_frame_alone_gives_the_bits_it_has_inside_the_batch(body, n):
    alone = rgb_of(body, K=body["K"][n:n + 1], Rt=body["Rt"][n:n + 1], frames=slice(n, n + 1))
    assert alone.shape == (1, 3, 96, 128) and torch.equal(alone[0], body["rgb"][n])


# ------------------------------------------------------------------------------------------------ the command line
@pytest.fixture(scope="module")
def files(want, body, tmp_path_factory):
    """static_assets.pt, the checkpoint, results.npy (5 frames, the scene's at 1:4), embs.npz and the three cameras as JSON."""
    sc, t, tmp = want["scene"], torch.from_numpy, tmp_path_factory.mktemp("body_chain")
    s = sc["surf"]
    model, cfg = SR.as_model_dicts(sc["skel"])
    assets = {"lbs_model_json": model, "lbs_config_dict": cfg, "lbs_template_verts": t(sc["template"]), "lbs_scale": t(sc["lbs_scale"]),
              "global_scaling": torch.tensor(float(sc["global_scaling"])), **body["assets"],
              "topology": {"vi": t(s["vi"]), "vt": t(s["vt"]), "vti": t(s["vti"]), "v2uv": t(s["v2uv"])}}
    torch.save(assets, tmp / "static_assets.pt")
    torch.save({k: t(np.ascontiguousarray(v)) for k, v in body["state"].items()}, tmp / "body_dec.ckpt")
    rs = np.random.RandomState(17)
    pad = lambda x, scale: np.concatenate([scale * rs.randn(1, x.shape[1]), x, scale * rs.randn(1, x.shape[1])]).astype(np.float32)
    np.save(tmp / "results.npy", {"motions": np.ascontiguousarray(pad(sc["motion"], 0.1).T[None, :, None, :])})      # [1, P, 1, 5]
    np.savez(tmp / "embs.npz", embs=pad(sc["embs"], 1.0)[None], face_embs=pad(sc["face_embs"], 1.0)[None])
    json.dump({"K": sc["K"].tolist(), "Rt": sc["Rt"].tolist()}, open(tmp / "cameras.json", "w"))
    argv = ["--results", str(tmp / "results.npy"), "--embeddings", str(tmp / "embs.npz"), "--assets", str(tmp / "static_assets.pt"),
            "--checkpoint", str(tmp / "body_dec.ckpt"), "--size", "96", "128", "--frames", "1:4"]
    for key, value in sc["tex_cfg"].items():                                  # the four configuration flags of the texture
        argv += ["--" + key.replace("_", "-"), str(value)]
    for key in ("n_pose_enc_channels", "n_embs", "n_embs_enc_channels", "n_face_embs", "n_init_channels", "n_min_channels"):
        argv += ["--" + key.replace("_", "-"), str(sc["cfg"][key])]
    return tmp, argv


def test_command_line_matches_the_direct_call(dev, want, body, files):
    from PIL import Image
    tmp, argv = files
    with torch.cuda.device(dev):
        assert T.main(argv + ["--camera-json", str(tmp / "cameras.json"), "--out", str(tmp / "frames.npy"), "--png-dir", str(tmp / "png")]) == 0
    got = np.load(tmp / "frames.npy")
    direct = body["rgb"].cpu().numpy()
    assert got.dtype == np.float32 and got.shape == (1, 3, 3, 96, 128) and np.array_equal(got[0], direct)
    gate("chain_rgb_command_line", got[0], want["c64"]["rgb"], want["allowance"]["rgb"], want["kept"])
    assert sorted(os.listdir(tmp / "png")) == [f"rgb_00_{n:05d}.png" for n in range(3)]
    for n in range(3):
        pix = np.asarray(Image.open(tmp / "png" / f"rgb_00_{n:05d}.png"))
        assert pix.dtype == np.uint8 and np.array_equal(pix, np.rint(direct[n]).astype(np.uint8).transpose(1, 2, 0)), n


@pytest.mark.parametrize("camera", ["eye_target", "default"])
def test_command_line_cameras_from_arguments(dev, want, files, camera):
    tmp, argv = files
    if camera == "eye_target":
        lo, hi = want["c64"]["verts"].reshape(-1, 3).min(0), want["c64"]["verts"].reshape(-1, 3).max(0)
        centre = (lo + hi) / 2
        eye = centre + np.array([2.0, 1.5, 1.6 * float((hi - lo).max())])
        argv = argv + ["--eye", *map(str, eye), "--target", *map(str, centre), "--fov", "36"]
    out = tmp / f"frames_{camera}.npy"
    with torch.cuda.device(dev):
        assert T.main(argv + ["--out", str(out)]) == 0
    got = np.load(out)
    assert got.dtype == np.float32 and got.shape == (1, 3, 3, 96, 128) and np.isfinite(got).all()
    assert got.min() >= 0 and got.max() <= 255
    for n in range(3):                                                        # linear_to_display maps a covered pixel to 0 in all channels only by luck
        covered = float((got[0, n] > 0).any(0).mean())
        record(f"chain_command_line_{camera}_frame{n}", covered=covered)
        assert 0.05 < covered < 0.95, (camera, n, covered)
