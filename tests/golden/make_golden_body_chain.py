"""Fixture for the body renderer end to end (audio2photoreal_amd/texture.py BodyTexture.forward and render_rgb_motion): the
reference's own modules in the order AutoEncoder.forward calls them (visualize/ca_body/models/mesh_vae_drivable.py:306-335) --
ConvDecoder, LBSModule.pose (utils/lbs.py), UNetViewDecoder.forward (which calls the reference's compute_view_cos and geo_fn.to_uv)
and PoseToShadow (nn/shadow.py) -- in float32 on the CPU, on the scene tests/body_chain_restatement.make_scene builds as data.
Build container only:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_body_chain.py

AutoEncoder.forward itself cannot be called: with encode=False it reads face_embs_body before assignment (:309), with encode=True
it needs the encoders.  forward_tex hard-codes 2048 and is pinned at full size by golden_texture_v1.npz; here the reference's three
inputs to it are stored.  RenderLayer needs pytorch3d, which is absent: render_restatement.py stays the contract, as the render
golden says.  The absent modules are stubbed by the finder of make_golden_decoder.py, so the reference's modules THEMSELVES run.
geo_fn.to_uv is the reference's values_to_uv on the face index image of the restatement's rule with the reference's bary_coords, as
in make_golden_surface.py.

Stored, as data only (below 1 MiB):
  * seed, draw: the draw of the scene that met the conditions; fingerprint/<name>: float64 sums of the scene's arrays;
  * ref/{geom, cond_view, tex_view_rec, shadow_map, tex_mean_rec}: the reference's outputs, maps on every 16th row (ROWS);
    e_ref/<the same>: the reference's float32 error against the float64 chain over EVERY element; e_ref/view_cos_uv: that of
    cond_view's first channel alone, on its own scale;
  * e/<stage>, e_proj (pixels), e_depth (relative): the float32 chain against the float64 chain; e/depth, e/render and e/rgb over
    the kept pixels;
  * face (int16), excluded (packed bits), rgb (the float64 chain's, as float32), cond/<name>: the scene's conditions;
  * mutant/<name>: how many allowances the named miswiring moves its most sensitive gated output, over the kept pixels.
Asserted: the conditions, equal float32 and float64 face images outside `excluded`, every mutant at 10 allowances or more."""
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
import body_chain_restatement as B  # noqa: E402
import skinning_restatement as SK  # noqa: E402
import surface_restatement as SU  # noqa: E402
from make_golden_decoder import _StubFinder  # noqa: E402
from make_golden_texture import load  # noqa: E402

ROWS = slice(5, None, 16)


def rows(a):
    return a[..., ROWS, :] if a.ndim == 4 and a.shape[-2] >= 128 else a


def reference(scene):
    """The reference's float32 geom, cond_view, tex_view_rec, shadow_map and tex_mean_rec on the scene."""
    import visualize.ca_body.models.mesh_vae_drivable as mvd
    import visualize.ca_body.utils.geom as geom
    import visualize.ca_body.utils.lbs as lbs
    from visualize.ca_body.nn.shadow import PoseToShadow
    from visualize.ca_body.utils.seams import SeamSampler

    t = torch.from_numpy
    surf, assets, cfg = scene["surf"], scene["assets"], scene["cfg"]
    for key, table in (("seam_data_1024", assets["seam_data_1024"]),):
        assert len({tuple(d) for d in table["dst_ij"]}) == len(table["dst_ij"]), "the reference leaves duplicates undefined"
    # geo_fn: the reference's functions on the fixture mesh; the index image by the restatement's rule, the barycentrics by the
    # reference's bary_coords on make_uv_barys' own grid
    index, _, face = SU.uv_images(surf, B.UV)
    c = torch.linspace(0.5, B.UV - 0.5, B.UV) / B.UV
    grid = torch.stack(torch.meshgrid(c, c, indexing="ij")[::-1], dim=2).reshape(-1, 2)
    tri = t(surf["vt"])[t(surf["vti"])[t(face).clamp(min=0)]].permute(2, 0, 1, 3)
    bary = geom.bary_coords(grid, tri.reshape(3, -1, 2)).permute(1, 0).reshape(B.UV, B.UV, 3)
    bary[t(face) < 0] = 0
    vt, v2uv, index = t(surf["vt"]), t(surf["v2uv"]).long(), t(index)
    geo_fn = types.SimpleNamespace(vi=t(surf["vi"]), from_uv=lambda values_uv: geom.sample_uv(values_uv, vt, v2uv),
                                   to_uv=lambda values: geom.values_to_uv(values, index, bary))
    seam = SeamSampler({k: t(np.ascontiguousarray(v)) for k, v in assets["seam_data_1024"].items()})
    masks = types.SimpleNamespace(**{k: assets[k] for k in ("pose_cond_mask", "head_cond_mask", "face_cond_mask", "body_cond_mask")})
    decoder = load(mvd.ConvDecoder(geo_fn, seam_sampler=seam, assets=masks, **cfg), scene["params"])
    model, lbs_cfg = SK.as_model_dicts(scene["skel"])
    model["SkinnedModel"].update(RestVertexNormals=np.zeros((437, 3)).tolist(), Faces={"Indices": [0, 1, 2], "TextureIndices": [0, 1, 2]},
                                 TextureCoordinates=[0.0] * 6)
    lbs_cfg = dict(lbs_cfg, channel_names=["tx", "ty", "tz", "rx", "ry", "rz", "sc"], transform=np.asarray(lbs_cfg["transform"]).tolist(),
                   transform_offsets=np.asarray(lbs_cfg["transform_offsets"]).tolist(), limits=[])
    lbs_fn = lbs.LBSModule(model, lbs_cfg, scene["template"], scene["lbs_scale"], scene["global_scaling"])
    view = mvd.UNetViewDecoder(geo_fn, net_uv_size=B.UV, seam_sampler=seam, n_init_ftrs=scene["tex_cfg"]["n_init_ftrs"])
    load(view.unet, B._sub(scene["tex_state"], "decoder_view.unet."))
    shadow = load(PoseToShadow(n_pose_dims=scene["tex_cfg"]["pose_to_shadow_dims"], uv_size=2 * B.UV), B._sub(scene["tex_state"], "pose_to_shadow."))
    with torch.no_grad():                                                     # mesh_vae_drivable.py:306-335, eval mode, pose_to_shadow enabled
        lbs_motion = t(scene["motion"])
        campos = -(t(scene["Rt"])[:, :, :3].transpose(1, 2) @ t(scene["Rt"])[:, :, 3:])[..., 0]
        dec_preds = decoder(motion=lbs_motion, embs=t(scene["embs"]), face_embs=t(scene["face_embs"]), embs_conv=None)
        geom_rec = lbs_fn.pose(dec_preds["geom_delta_rec"], lbs_motion)
        dec_view_preds = view.eval()(geom_rec=geom_rec, tex_mean_rec=dec_preds["tex_mean_rec"], camera_pos=campos)
        shadow_preds = shadow(lbs_motion)
    return {"geom": geom_rec.numpy(), "cond_view": dec_view_preds["cond_view"].numpy(), "tex_view_rec": dec_view_preds["tex_view_rec"].numpy(),
            "shadow_map": shadow_preds["shadow_map"].numpy(), "tex_mean_rec": dec_preds["tex_mean_rec"].numpy()}


def main():
    sys.dont_write_bytecode = True
    assert os.path.isdir(ri.REF), "reference tree not present (only in the build container)"
    sys.meta_path.insert(0, _StubFinder())
    sys.path.insert(0, ri.REF)

    t0 = time.time()
    scene, got = B.make_scene()
    c64, c32, y, ex, facts = got["c64"], got["c32"], got["yardsticks"], got["excluded"], got["conditions"]
    print(f"scene: draw {scene['draw']} after {time.time() - t0:.0f} s")
    assert not B.failed(facts), B.failed(facts)
    outside = ~ex
    assert np.array_equal(c32["face"][outside], c64["face"][outside]), "float32 and float64 disagree on a face outside `excluded`"
    hit = c64["face"] >= 0
    kept = hit & outside
    out = {"seed": np.int64(scene["seed"]), "draw": np.int64(scene["draw"]), "rows_start": np.int64(ROWS.start), "rows_step": np.int64(ROWS.step),
           "clearance_factor": np.int32(B.RR.CLEARANCE_FACTOR)}
    for k, v in B.fingerprints(scene).items():
        out[f"fingerprint/{k}"] = np.float64(v)
    for k, v in y.items():
        out[k] = np.float64(v)
    ref = reference(scene)
    want = {"geom": c64["verts"], "cond_view": c64["cond_view"], "tex_view_rec": c64["tex_view_rec"], "shadow_map": c64["shadow_map"],
            "tex_mean_rec": c64["tex_mean_rec"]}
    for k in ref:
        assert ref[k].dtype == np.float32 and ref[k].shape == want[k].shape, (k, ref[k].dtype, ref[k].shape, want[k].shape)
        out[f"ref/{k}"] = rows(ref[k])
        out[f"e_ref/{k}"] = np.float64(B.nerr(ref[k], want[k]))
    out["e_ref/view_cos_uv"] = np.float64(B.nerr(ref["cond_view"][:, :1], c64["cond_view"][:, :1]))     # the channel alone: its own scale
    assert c64["face"].max() < 2 ** 15
    out["face"], out["excluded"], out["rgb"] = c64["face"].astype(np.int16), np.packbits(ex), c64["rgb"].astype(np.float32)
    for k, v in facts.items():
        out[f"cond/{k}"] = np.asarray(v, np.float64)
    out["cond/excluded_pixels"] = ex.sum(axis=(1, 2)).astype(np.int64)
    out["cond/face_differences_inside"] = (c32["face"] != c64["face"]).sum(axis=(1, 2)).astype(np.int64)
    allowance = B.allowances(out)
    for name in B.MUTANTS:
        ratio, where = B.mutant_ratio(c64, B.chain(scene, mutant=name, base=c64), kept, allowance)
        print(f"mutant {name}: {ratio:.3g} allowances on {where}")
        assert ratio >= 10, f"mutant {name} moves no gated output by 10 allowances ({ratio:.3g} on {where}): change the scene"
        out[f"mutant/{name}"] = np.float64(ratio)
    path = os.path.join(HERE, "golden_body_chain_v1.npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    print(path, size, "bytes")
    assert size < 1 << 20, "the golden file has to stay below 1 MiB"
    print("conditions:", facts)
    print("excluded pixels per frame:", out["cond/excluded_pixels"], "float32 face differences (all inside):", out["cond/face_differences_inside"])
    print({k: float(v) for k, v in out.items() if k.startswith(("e_ref/", "e/", "e_"))})


if __name__ == "__main__":
    main()
