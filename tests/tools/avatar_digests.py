"""SHA-256 digests of what the avatar stages' clip entry points return, for comparing two trees bit for bit on one GPU.

    python tests/tools/avatar_digests.py [--out digests.txt]

The person is the smallest synthetic one of tests/test_render_codes_hip.py (3 frames), the image 24 x 32, the scene two of that
person with motions of their own and one placement.  pose_motion, decode_motion, render_rgb_motion, encode_motion,
render_codes_motion (2 cameras) and render_conversation_motion (2 people) run at max_bytes=1 (chunks of one frame) and at the
default, the three rendering entries at supersample 1 and 2.  One line per returned array: name, dtype, shape, digest.  The tool
imports the package of the tree it lies in and uses only names both sides of a refactor of the stages' front ends have."""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import body_chain_restatement as B  # noqa: E402
import encoder_restatement as R  # noqa: E402
from audio2photoreal_amd import decoder as D, encoder as E, render as RD, scene as SN, skinning as SK, surface as S, texture as T  # noqa: E402

ENC_UV, SIZE = 16, (24, 32)


def person(dev):
    sc = B.draw_scene(B.SEED, 0)
    face_enc_cfg = dict(R.FACE_ENC, uv_size=ENC_UV, n_embs=sc["cfg"]["n_face_embs"])
    body_enc_cfg = dict(R.BODY_ENC, uv_size=ENC_UV, n_embs=sc["cfg"]["n_embs"])
    state = {**{"decoder." + k: v for k, v in sc["params"].items()}, **sc["tex_state"],
             **{"decoder_face." + k: v for k, v in R.face_decoder_params(R.FACE_DEC, 51).items()},
             **{"encoder_face." + k: v for k, v in R.face_encoder_params(face_enc_cfg, 3 * R.FACE_DEC["V"], 52).items()},
             **{"encoder." + k: v for k, v in R.body_encoder_params(body_enc_cfg, 53).items()}}
    assets = {**sc["assets"], **sc["tex_assets"], **R.make_fixture()["assets"]}
    s, skel = sc["surf"], sc["skel"]
    surface = S.BodySurface.from_arrays(s["vi"], s["vt"], s["vti"], n_verts=s["n_verts"], v2uv=s["v2uv"], uv_size=B.UV)
    skeleton = SK.BodySkeleton.from_arrays(skel["parents"], skel["pre_rotation"], skel["joint_offset"], skel["transform"],
                                           skel["transform_offsets"], 16, 3, skel["rest_vertices"], skel["skin_indices"], skel["skin_weights"],
                                           template_verts=sc["template"], lbs_scale=sc["lbs_scale"], global_scaling=sc["global_scaling"])
    avatar = SN.Avatar(E.FaceDecoder.from_state_dict(state, assets), E.FaceEncoder.from_state_dict(state, assets, uv_size=ENC_UV),
                       E.BodyEncoder.from_state_dict(state, assets, surface, uv_size=ENC_UV), D.BodyDecoder.from_state_dict(state, assets, surface, **sc["cfg"]),
                       T.BodyTexture.from_state_dict(state, assets, surface, **sc["tex_cfg"]), skeleton, surface)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(dev)
    K = sc["K"][:2].copy()
    K[:, :2] *= np.float32(SIZE[0] / sc["size"][0])
    assert SIZE[1] / sc["size"][1] == SIZE[0] / sc["size"][0]
    rs = np.random.RandomState(64)
    codes = np.random.RandomState(54).randn(len(sc["motion"]), R.FACE_DEC["n_latent"]).astype(np.float32)
    motion_b = (sc["motion"][::-1] + 0.05 * rs.randn(*sc["motion"].shape)).astype(np.float32)
    return {"avatar": avatar, "poses": [up(sc["motion"]), up(motion_b)], "codes": [up(codes), up(rs.randn(*codes.shape))], "K": up(K),
            "Rt": up(sc["Rt"][:2])}


def digests(dev) -> list:
    p = person(dev)
    a, (H, W) = p["avatar"], SIZE
    rz = RD.BodyRasterizer(a.surface, H, W)
    poses, codes, K, Rt = p["poses"][0], p["codes"][0], p["K"], p["Rt"]
    verts = a.skeleton.pose_vertices(poses[:1]).cpu().numpy()[0]
    lo, hi = verts.min(0), verts.max(0)
    extent = float((hi - lo).max())
    M = SN.placement(40.0, (0.25 * extent, 0.0, 0.1 * extent), (0, 1, 0), pivot=(lo + hi) / 2).numpy()
    lines = []

    def note(name, out):
        for key, x in sorted((out if isinstance(out, dict) else {"": out}).items()):
            x = x.cpu().numpy()
            lines.append(f"{name}{'.' + key if key else ''} {x.dtype} {list(x.shape)} {hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest()}")

    note("pose_motion", SK.pose_motion(a.skeleton, poses))
    for label, kw in (("max_bytes=1", {"max_bytes": 1}), ("default", {})):
        enc = E.encode_motion(a.face_decoder, a.face_encoder, a.body_encoder, a.skeleton, poses, codes, **kw)
        note(f"encode_motion[{label}]", enc)
        note(f"decode_motion[{label}]", D.decode_motion(a.decoder, a.skeleton, poses, enc["embs"], enc["face_embs"], **kw))
        for s in (1, 2):
            note(f"render_rgb_motion[{label}, supersample={s}]",
                 T.render_rgb_motion(a.decoder, a.texture, a.skeleton, rz, poses, enc["embs"], enc["face_embs"], K[:1], Rt[:1], supersample=s, **kw))
            note(f"render_codes_motion[{label}, supersample={s}]", E.render_codes_motion(*a[:6], rz, poses, codes, K, Rt, supersample=s, **kw))
            note(f"render_conversation_motion[{label}, supersample={s}]",
                 SN.render_conversation_motion([a, a], p["poses"], p["codes"], [None, M], K, Rt, H, W, supersample=s, **kw))
    return lines


if __name__ == "__main__":
    cli = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    cli.add_argument("--out", default=None, help="also write the lines to this file")
    out = cli.parse_args().out
    assert torch.cuda.is_available(), "the digests are computed on the MI355X"
    with torch.cuda.device(0):
        text = "\n".join(digests(torch.device("cuda:0"))) + "\n"
    sys.stdout.write(text)
    if out is not None:
        with open(out, "w") as f:
            f.write(text)
