"""Fixture for the encode path (audio2photoreal_amd/encoder.py, BodySkeleton.unpose_vertices): the reference's own
FaceDecoderFrontal (visualize/ca_body/nn/face.py), FaceEncoder and Encoder (models/mesh_vae_drivable.py, with ConvDownBlock of
nn/blocks.py and values_to_uv of utils/geom.py) and LBSModule.unpose (utils/lbs.py) in float32 on the CPU, on the state dicts,
assets and inputs that tests/encoder_restatement.make_reference_fixture builds as data.  Build container only:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_encoder.py

The absent modules the reference imports are stubbed by the finder of make_golden_decoder.py, so the reference's modules THEMSELVES
run; LBSModule is built as in make_golden_skinning.py.  The classes fix 1024 for the face texture and 512 for both encoders; the
free sizes are small (16 codes, 24 face vertices, 6 and 5 embedding values, 2 frames).

Stored, as data only (below 1 MiB):
  * fingerprint/<net>/<key>: the float64 sum of every array of the seeded state dicts, and input/<name> sums of the large inputs;
  * the small inputs whole (codes, poses, scales) and posed32, the reference's own posed vertices that unpose reads; the face
    encoder reads the float64 restatement's decoder outputs rounded to float32, which the fixture alone reproduces;
  * ref/<output>: the reference's outputs -- small ones whole, maps with 128 rows or more on every 128th row;
  * e_ref/<output>: the reference's own float32 error against the float64 restatement over EVERY element, max |difference| / max
    |value| -- what the GPU tests multiply by 4."""
import os
import sys
import time
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_import as ri  # noqa: E402
import encoder_restatement as R  # noqa: E402
import skinning_restatement as SR  # noqa: E402
from make_golden_decoder import _StubFinder  # noqa: E402
from make_golden_texture import load  # noqa: E402


def main():
    sys.dont_write_bytecode = True
    assert os.path.isdir(ri.REF), "reference tree not present (only in the build container)"
    sys.meta_path.insert(0, _StubFinder())
    sys.path.insert(0, ri.REF)
    import visualize.ca_body.models.mesh_vae_drivable as mvd
    import visualize.ca_body.utils.geom as geom
    import visualize.ca_body.utils.lbs as lbs
    from visualize.ca_body.nn.face import FaceDecoderFrontal

    fx, t = R.make_reference_fixture(), torch.from_numpy
    a = types.SimpleNamespace(**fx["assets"])
    out = {"rows_start": np.int64(R.REF_ROWS.start), "rows_step": np.int64(R.REF_ROWS.step), "codes": fx["codes"], "poses": fx["poses"],
           "scales": fx["scales"]}
    for net in ("face_dec", "face_enc", "body_enc"):
        for k, v in R.fingerprint(fx[net]).items():
            out[f"fingerprint/{net}/{k}"] = np.float64(v)
    for k in ("displacement", "index_image", "bary_image", "template"):
        out[f"input/{k}"] = np.float64(np.asarray(fx[k], np.float64).sum())
    ref = {}
    with torch.no_grad():
        cfg = R.REF_FACE_DEC
        dec = load(FaceDecoderFrontal(a, n_latent=cfg["n_latent"], n_vert_out=3 * cfg["V"]), fx["face_dec"])
        got = dec(t(fx["codes"]))
        ref.update({f"face_dec/{k}": v.numpy() for k, v in got.items()})
        cfg = R.REF_FACE_ENC
        enc = load(mvd.FaceEncoder(1.0, a, n_embs=cfg["n_embs"], n_vert_in=3 * R.REF_FACE_DEC["V"]), fx["face_enc"])
        # the face encoder reads the float64 restatement's decoder outputs rounded to float32 (reproducible from the fixture alone; the
        # reference's own 1024 x 1024 output is too large to store); face_tex from them by the reference's own line
        want_dec = R.face_decoder(fx["face_dec"], R.face_layers(R.REF_FACE_DEC), fx["assets"]["face_frontal_view"], fx["codes"])
        geom32, raw32 = t(want_dec["face_geom"].astype(np.float32)), t(want_dec["face_tex_raw"].astype(np.float32))
        got_e = enc(geom32, 255 * (raw32 + dec.bias[None] + 0.5))
        ref.update({f"face_enc/{k}": v.numpy() for k, v in got_e.items()})
        index_image, bary_image = t(fx["index_image"]).long(), t(fx["bary_image"])
        geo_fn = types.SimpleNamespace(to_uv=lambda values: geom.values_to_uv(values, index_image, bary_image))
        body = load(mvd.Encoder(geo_fn, R.REF_BODY_ENC["n_embs"], 1.0, 1.0 - fx["assets"]["face_mask"]), fx["body_enc"])
        ref.update({f"body_enc/{k}": v.numpy() for k, v in body(t(fx["poses"]), t(fx["displacement"])).items()})

        skel, V = fx["skel"], fx["surf"]["n_verts"]
        det = np.abs(R.blend_determinants(skel, fx["poses"], fx["scales"]))
        s3 = SR.joint_states(skel, fx["poses"], fx["scales"])[:, :, 7] ** 3
        print("blend |det|:", det.min(), det.max(), "joint scale^3:", s3.min(), s3.max())
        assert det.min() >= 0.5 * s3.min() and det.max() <= 2.0 * s3.max(), "a blended matrix is badly conditioned: gentler poses"
        counts = (skel["skin_weights"] > 0).sum(axis=1)
        offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        flat_i = np.concatenate([skel["skin_indices"][v, :counts[v]] for v in range(V)])
        flat_w = np.concatenate([skel["skin_weights"][v, :counts[v]] for v in range(V)])
        J = len(skel["parents"])
        model_json = {
            "Skeleton": {"Bones": [{"Name": f"b{j}", "Parent": int(skel["parents"][j]) if skel["parents"][j] >= 0 else 2 ** 31,
                                    "PreRotation": skel["pre_rotation"][j].tolist(), "TranslationOffset": skel["joint_offset"][j].tolist()}
                                   for j in range(J)]},
            "SkinnedModel": {"RestPositions": skel["rest_vertices"].tolist(), "RestVertexNormals": np.zeros((V, 3)).tolist(),
                             "SkinningWeights": [[int(i), float(w)] for i, w in zip(flat_i, flat_w)], "SkinningOffsets": offsets.tolist(),
                             "Faces": {"Indices": [0, 1, 2], "TextureIndices": [0, 1, 2]}, "TextureCoordinates": [0.0] * 6}}
        lcfg = {"channel_names": ["tx", "ty", "tz", "rx", "ry", "rz", "sc"], "transform": skel["transform"].tolist(),
                "transform_offsets": skel["transform_offsets"].reshape(1, -1).tolist(), "limits": [],
                "nr_scaling_params": 12, "nr_position_params": 104}
        mod = lbs.LBSModule(model_json, lcfg, fx["template"], fx["scales"][0], fx["global_scaling"])
        posed = mod.pose(t(fx["displacement"]), t(fx["poses"]))
        out["posed32"] = posed.numpy()
        ref["unpose/verts_unposed"] = mod.unpose(posed, t(fx["poses"])).numpy()

    fx["posed32"] = out["posed32"]
    t0 = time.time()
    want = R.reference_forward(fx)
    print(f"float64 restatement: {time.time() - t0:.1f} s")
    assert set(ref) == set(want), sorted(set(ref) ^ set(want))
    for k, v in ref.items():
        assert v.dtype == np.float32 and v.shape == want[k].shape, (k, v.dtype, v.shape, want[k].shape)
        out[f"ref/{k}"] = v[..., R.REF_ROWS, :] if v.ndim == 4 and v.shape[-2] >= 128 else v
        out[f"e_ref/{k}"] = np.float64(R.nerr(v, want[k]))
    path = os.path.join(HERE, "golden_encoder_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    print({k: float(v) for k, v in out.items() if k.startswith("e_ref/")})
    t0 = time.time()
    low = R.reference_forward(fx, np.float32)
    print(f"float32 restatement vs float64 ({time.time() - t0:.1f} s):", {k: R.nerr(low[k], want[k]) for k in want})


if __name__ == "__main__":
    main()
