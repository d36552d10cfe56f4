"""From sampler output to uint8 frames on the MI355X: encoder.render_codes_motion and the command line of audio2photoreal_amd/
encoder.py on the scene of tests/body_chain_restatement.py (decoder, texture, skeleton, cameras) with small encoders in front.
Every comparison here is exact: the loop must give the bits of its pieces composed by hand -- encode_motion, then
texture.render_rgb_motion per camera, concatenated along the width, clipped and truncated to uint8."""
import json
import os

import numpy as np
import pytest
import torch

import body_chain_restatement as B
import encoder_restatement as R
import skinning_restatement as SR
from audio2photoreal_amd import decoder as D
from audio2photoreal_amd import encoder as E
from audio2photoreal_amd import render as RD
from audio2photoreal_amd import skinning as SK
from audio2photoreal_amd import surface as S
from audio2photoreal_amd import texture as T
from audio2photoreal_amd._lib import A2PError
from conftest import record

pytestmark = pytest.mark.gpu
ENC_UV = 16


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)


@pytest.fixture(scope="module")
def scene():
    """The body chain's scene plus encoder weights whose embedding widths are the decoder's, and 3 frames of face codes."""
    sc = B.draw_scene(B.SEED, 0)
    face_enc_cfg = dict(R.FACE_ENC, uv_size=ENC_UV, n_embs=sc["cfg"]["n_face_embs"])
    body_enc_cfg = dict(R.BODY_ENC, uv_size=ENC_UV, n_embs=sc["cfg"]["n_embs"])
    fx = R.make_fixture()
    state = {**{"decoder." + k: v for k, v in sc["params"].items()}, **sc["tex_state"],
             **{"decoder_face." + k: v for k, v in R.face_decoder_params(R.FACE_DEC, 51).items()},
             **{"encoder_face." + k: v for k, v in R.face_encoder_params(face_enc_cfg, 3 * R.FACE_DEC["V"], 52).items()},
             **{"encoder." + k: v for k, v in R.body_encoder_params(body_enc_cfg, 53).items()}}
    assets = {**sc["assets"], **sc["tex_assets"], **fx["assets"]}
    return {"sc": sc, "state": state, "assets": assets, "codes": np.random.RandomState(54).randn(len(sc["motion"]), R.FACE_DEC["n_latent"]).astype(np.float32)}


@pytest.fixture(scope="module")
def body(dev, scene):
    sc = scene["sc"]
    s, skel = sc["surf"], sc["skel"]
    surface = S.BodySurface.from_arrays(s["vi"], s["vt"], s["vti"], n_verts=s["n_verts"], v2uv=s["v2uv"], uv_size=B.UV)
    H, W = sc["size"]
    return {"face_decoder": E.FaceDecoder.from_state_dict(scene["state"], scene["assets"]),
            "face_encoder": E.FaceEncoder.from_state_dict(scene["state"], scene["assets"], uv_size=ENC_UV),
            "body_encoder": E.BodyEncoder.from_state_dict(scene["state"], scene["assets"], surface, uv_size=ENC_UV),
            "decoder": D.BodyDecoder.from_state_dict(scene["state"], scene["assets"], surface, **sc["cfg"]),
            "texture": T.BodyTexture.from_state_dict(scene["state"], scene["assets"], surface, **sc["tex_cfg"]),
            "skeleton": SK.BodySkeleton.from_arrays(skel["parents"], skel["pre_rotation"], skel["joint_offset"], skel["transform"],
                                                    skel["transform_offsets"], 16, 3, skel["rest_vertices"], skel["skin_indices"], skel["skin_weights"],
                                                    template_verts=sc["template"], lbs_scale=sc["lbs_scale"], global_scaling=sc["global_scaling"]),
            "rasterizer": RD.BodyRasterizer(surface, H, W), "frames": up(sc["motion"], dev), "codes": up(scene["codes"], dev),
            "K": up(sc["K"][:2], dev), "Rt": up(sc["Rt"][:2], dev)}


def nets(b):
    return (b["face_decoder"], b["face_encoder"], b["body_encoder"], b["decoder"], b["texture"], b["skeleton"], b["rasterizer"])


def by_hand(b, frames, codes, K, Rt, **kw):
    """encode_motion, render_rgb_motion per camera, the reference's concatenation, clip and truncation."""
    enc = E.encode_motion(b["face_decoder"], b["face_encoder"], b["body_encoder"], b["skeleton"], frames, codes, **kw)
    panels = [T.render_rgb_motion(b["decoder"], b["texture"], b["skeleton"], b["rasterizer"], frames, enc["embs"], enc["face_embs"],
                                  K[c:c + 1], Rt[c:c + 1]) for c in range(K.shape[0])]
    return torch.cat(panels, dim=-1).permute(0, 2, 3, 1).clip(0, 255).to(torch.uint8)


def test_render_codes_motion_is_its_pieces_composed_by_hand(dev, body):
    b = body
    H, W = b["rasterizer"].height, b["rasterizer"].width
    with torch.cuda.device(dev):
        got = E.render_codes_motion(*nets(b), b["frames"], b["codes"], b["K"], b["Rt"])
        assert got.dtype == torch.uint8 and got.shape == (3, H, 2 * W, 3)
        want = by_hand(b, b["frames"], b["codes"], b["K"], b["Rt"])
        assert torch.equal(got, want)
        for c in range(2):                                                     # both panels show the body, from different cameras
            covered = float((got[:, :, c * W:(c + 1) * W] > 0).any(-1).float().mean())
            record(f"enc_render_codes_panel{c}", covered=covered)
            assert 0.05 < covered < 0.95, (c, covered)
        assert not torch.equal(got[:, :, :W], got[:, :, W:])
        assert torch.equal(E.render_codes_motion(*nets(b), b["frames"], b["codes"], b["K"], b["Rt"], max_bytes=1), got)       # chunks of one frame
        lead = E.render_codes_motion(*nets(b), b["frames"][None], b["codes"][None], b["K"][:1], b["Rt"][:1])                 # [B, T, ..], one camera
        assert lead.shape == (1, 3, H, W, 3) and torch.equal(lead[0], got[:, :, :W])
        rest = E.render_codes_motion(*nets(b), b["frames"], b["codes"], b["K"], b["Rt"], body_embs="rest")
        assert torch.equal(rest, by_hand(b, b["frames"], b["codes"], b["K"], b["Rt"], body_embs="rest"))
        record("enc_render_codes_rest_vs_per_frame", differing_values=int((rest != got).sum()), values=got.numel(),
               max_abs_diff=int((rest.int() - got.int()).abs().max()))
    with pytest.raises(A2PError, match="cameras"):
        E.render_codes_motion(*nets(b), b["frames"], b["codes"], b["K"], b["Rt"][:1])
    with pytest.raises(A2PError, match="face_codes"):
        E.render_codes_motion(*nets(b), b["frames"], b["codes"][:2], b["K"], b["Rt"])


def test_command_line_matches_the_direct_call(dev, scene, body, tmp_path):
    from PIL import Image
    sc, t, tmp = scene["sc"], torch.from_numpy, tmp_path
    s = sc["surf"]
    model, cfg = SR.as_model_dicts(sc["skel"])
    assets = {"lbs_model_json": model, "lbs_config_dict": cfg, "lbs_template_verts": t(sc["template"]), "lbs_scale": t(sc["lbs_scale"]),
              "global_scaling": torch.tensor(float(sc["global_scaling"])), **scene["assets"],
              "topology": {"vi": t(s["vi"]), "vt": t(s["vt"]), "vti": t(s["vti"]), "v2uv": t(s["v2uv"])}}
    torch.save(assets, tmp / "static_assets.pt")
    torch.save({k: t(np.ascontiguousarray(v)) for k, v in scene["state"].items()}, tmp / "body_dec.ckpt")
    rs = np.random.RandomState(17)
    pad = lambda x, scale: np.concatenate([scale * rs.randn(1, x.shape[1]), x, scale * rs.randn(1, x.shape[1])]).astype(np.float32)
    np.save(tmp / "results.npy", {"pose": pad(sc["motion"], 0.1)[None], "face": pad(scene["codes"], 1.0)[None]})              # [1, 5, .]
    json.dump({"K": sc["K"][:2].tolist(), "Rt": sc["Rt"][:2].tolist()}, open(tmp / "cameras.json", "w"))
    torch.save({"K": t(sc["K"][:2]), "Rt": t(sc["Rt"][:2])}, tmp / "render_defaults.pth")
    argv = ["--results", str(tmp / "results.npy"), "--assets", str(tmp / "static_assets.pt"), "--checkpoint", str(tmp / "body_dec.ckpt"),
            "--size", "96", "128", "--frames", "1:4", "--encoder-uv-size", str(ENC_UV)]
    for key, value in sc["tex_cfg"].items():
        argv += ["--" + key.replace("_", "-"), str(value)]
    for key in ("n_pose_enc_channels", "n_embs", "n_embs_enc_channels", "n_face_embs", "n_init_channels", "n_min_channels"):
        argv += ["--" + key.replace("_", "-"), str(sc["cfg"][key])]
    with torch.cuda.device(dev):
        direct = E.render_codes_motion(*nets(body), body["frames"], body["codes"], body["K"], body["Rt"]).cpu().numpy()
        assert E.main(argv + ["--camera-json", str(tmp / "cameras.json"), "--out", str(tmp / "frames.npy"), "--png-dir", str(tmp / "png")]) == 0
        assert E.main(argv + ["--defaults", str(tmp / "render_defaults.pth"), "--out", str(tmp / "frames_defaults.npy")]) == 0
    got = np.load(tmp / "frames.npy")
    assert got.dtype == np.uint8 and got.shape == (1, 3, 96, 256, 3) and np.array_equal(got[0], direct)
    assert np.array_equal(np.load(tmp / "frames_defaults.npy"), got)
    assert sorted(os.listdir(tmp / "png")) == [f"frame_00_{n:05d}.png" for n in range(3)]
    for n in range(3):
        assert np.array_equal(np.asarray(Image.open(tmp / "png" / f"frame_00_{n:05d}.png")), direct[n]), n
    np.save(tmp / "no_face.npy", {"pose": pad(sc["motion"], 0.1)[None]})
    with pytest.raises(A2PError, match="holds no `face`"):
        E.main(["--results", str(tmp / "no_face.npy")] + argv[2:] + ["--out", str(tmp / "x.npy")])
