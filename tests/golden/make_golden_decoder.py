"""Fixture for the decoder layers (audio2photoreal_amd/decoder.py): the reference's own ConvDecoder (visualize/ca_body/models/
mesh_vae_drivable.py, with its ConvBlock / UpConvBlockDeep of nn/blocks.py, Conv2dWNUB / LinearWN of nn/layers.py and SeamSampler
of utils/seams.py) in float32 on the CPU, on the configuration, state dict, masks, seam table and inputs that
tests/decoder_restatement.make_fixture builds as data.  Build container only:
    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_decoder.py

mesh_vae_drivable.py imports torchvision, pytorch3d, attrdict and (through nn/blocks.py's stray `from turtle import forward`)
tkinter, all absent here; a module finder hands out empty stub modules for those names, so ConvDecoder ITSELF runs -- nothing of
it is re-composed.  Its geo_fn is the reference's sample_uv on the fixture mesh, exactly what GeometryModule.from_uv calls.

Stored, as data only (the file has to stay below 1 MiB, and float32 noise does not compress):
  * fingerprint/<key>: the float64 sum of every array of the state dict, which the seeded generator rebuilds bit for bit (3.7 M
    values -- 14 MB -- that cannot be stored), and the inputs motion, embs, face_embs;
  * ref/<output>: the reference's five outputs, the two [2, 3, 256, 256] maps on every 16th row (ROWS) of both frames, the others
    whole; ref/block/<name>: frame 0 of the block-level intermediates, the 128 x 128 and 256 x 256 ones on every 16th row;
  * e_ref/<output> and e_ref/block/<name>: the reference's own float32 error against the float64 restatement over EVERY element
    of both frames, max |difference| / max |value| -- what the GPU tests multiply by 4."""
import importlib.abc
import importlib.machinery
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_import as ri  # noqa: E402
import decoder_restatement as R  # noqa: E402

ABSENT = ("turtle", "torchvision", "pytorch3d", "attrdict", "drtk", "cv2", "igl", "trimesh")
ROWS = slice(5, None, 16)          # the rows kept of a map with 128 rows or more
BLOCKS = ("embs_conv_block.3", "face_embs_conv_block.2", "joint_conv_block", "conv_blocks.0", "conv_blocks.1")


class _Stub(types.ModuleType):
    __path__ = []

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return None


class _StubFinder(importlib.abc.MetaPathFinder, importlib.abc.Loader):
    def find_spec(self, name, path, target=None):
        if name.split(".")[0] in ABSENT:
            return importlib.machinery.ModuleSpec(name, self, is_package=True)

    def create_module(self, spec):
        return _Stub(spec.name)

    def exec_module(self, module):
        pass


def rows(a):
    return a[..., ROWS, :] if a.shape[-2] >= 128 else a


def main():
    sys.dont_write_bytecode = True
    assert os.path.isdir(ri.REF), "reference tree not present (only in the build container)"
    sys.meta_path.insert(0, _StubFinder())
    sys.path.insert(0, ri.REF)
    import visualize.ca_body.models.mesh_vae_drivable as mvd
    import visualize.ca_body.utils.geom as geom
    from visualize.ca_body.utils.seams import SeamSampler

    fx = R.make_fixture()
    cfg, params, assets, surf = fx["cfg"], fx["params"], fx["assets"], fx["surf"]
    seam = {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in assets["seam_data_1024"].items()}
    assert len({tuple(d) for d in assets["seam_data_1024"]["dst_ij"]}) == len(seam["dst_ij"]), "the reference leaves duplicates undefined"
    vt, v2uv = torch.from_numpy(surf["vt"]), torch.from_numpy(surf["v2uv"]).long()
    geo_fn = types.SimpleNamespace(from_uv=lambda values_uv: geom.sample_uv(values_uv, vt, v2uv))
    masks = types.SimpleNamespace(**{k: assets[k] for k in ("pose_cond_mask", "head_cond_mask", "face_cond_mask", "body_cond_mask")})
    dec = mvd.ConvDecoder(geo_fn, seam_sampler=SeamSampler(seam), assets=masks, **cfg).eval()
    own = dict(dec.named_parameters())
    assert set(own) == set(params), sorted(set(own) ^ set(params))
    with torch.no_grad():
        for k, p in own.items():
            assert tuple(p.shape) == params[k].shape, (k, tuple(p.shape), params[k].shape)
            p.copy_(torch.from_numpy(params[k]))
    got_blocks = {}
    for name in BLOCKS:
        dec.get_submodule(name).register_forward_hook(lambda m, i, o, name=name: got_blocks.__setitem__(name, o.detach().numpy().copy()))
    with torch.no_grad():
        ref = dec(torch.from_numpy(fx["motion"]), torch.from_numpy(fx["embs"]), torch.from_numpy(fx["face_embs"]))
    ref = {k: v.numpy() for k, v in ref.items()}
    keep = {}
    want = R.decoder_forward(params, cfg, assets, surf, fx["motion"], fx["embs"], fx["face_embs"], keep=keep)

    out = {"motion": fx["motion"], "embs": fx["embs"], "face_embs": fx["face_embs"], "rows_start": np.int64(ROWS.start),
           "rows_step": np.int64(ROWS.step)}
    for k, v in R.fingerprint(params).items():
        out[f"fingerprint/{k}"] = np.float64(v)
    for k in ref:
        assert ref[k].dtype == np.float32 and ref[k].shape == want[k].shape, k
        out[f"ref/{k}"] = rows(ref[k])
        out[f"e_ref/{k}"] = np.float64(R.nerr(ref[k], want[k]))
    for name in BLOCKS:
        assert got_blocks[name].shape == keep[name].shape, name
        out[f"ref/block/{name}"] = rows(got_blocks[name][:1])
        out[f"e_ref/block/{name}"] = np.float64(R.nerr(got_blocks[name], keep[name]))
    path = os.path.join(HERE, "golden_decoder_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    print({k: float(v) for k, v in out.items() if k.startswith("e_ref/")})
    low = R.decoder_forward(params, cfg, assets, surf, fx["motion"], fx["embs"], fx["face_embs"], dtype=np.float32)
    print("float32 restatement vs float64:", {k: R.nerr(low[k], want[k]) for k in want})


if __name__ == "__main__":
    main()
