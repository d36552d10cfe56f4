"""Fixture for the surface maps (audio2photoreal_amd/surface.py): the reference's own vert_normals, compute_view_cos, values_to_uv,
sample_uv, bary_coords and compute_v2uv (visualize/ca_body/utils/geom.py) in float32 on the CPU, on the fixture mesh built as data
by tests/surface_restatement.make_surface.  Build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_surface.py

geom.py imports pytorch3d's rasteriser and Meshes (absent here) for the two functions that build the UV images; stub modules stand
in for them, and the face index images come from the restatement's rule instead (the fixture keeps every texel centre away from
every UV edge, so that rule, a strict one and float32 against float64 agree on every texel).

Stored: the mesh, 3 frames of vertices, cameras, a UV input for from_uv, the face index images at uv_size 48 and 130 with the
reference's bary_coords on them, the reference's outputs, and e_ref/*: the reference's own float32 error against the float64
restatement, max |difference| / max |value| per output -- what the GPU tests multiply by 4."""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import ref_import as ri  # noqa: E402
import surface_restatement as R  # noqa: E402

N = 3


def main():
    sys.dont_write_bytecode = True
    assert os.path.isdir(ri.REF), "reference tree not present (only in the build container)"
    for name in ("pytorch3d", "pytorch3d.renderer", "pytorch3d.renderer.mesh", "pytorch3d.renderer.mesh.rasterize_meshes",
                 "pytorch3d.structures"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["pytorch3d.renderer.mesh.rasterize_meshes"].rasterize_meshes = None
    sys.modules["pytorch3d.structures"].Meshes = None
    sys.path.insert(0, ri.REF)
    import visualize.ca_body.utils.geom as geom   # the reference's own functions

    surf = R.make_surface()
    V, vi, vt, vti = surf["n_verts"], surf["vi"], surf["vt"], surf["vti"]
    verts = R.make_frames(surf, 5, N)
    rs = np.random.RandomState(6)
    camera = (np.array([1.1, 0.9, 2.5]) + rs.randn(N, 3) * 0.3).astype(np.float32)
    values_uv = rs.randn(N, 4, 33, 33).astype(np.float32)

    v2uv = geom.compute_v2uv(V, vi, vti)
    assert np.array_equal(v2uv, R.compute_v2uv(V, vi, vti))
    out = {"vi": vi.astype(np.int32), "vt": vt, "vti": vti.astype(np.int32), "rest": surf["rest"], "verts": verts, "camera": camera,
           "values_uv": values_uv, "ref/v2uv": v2uv.astype(np.int32)}
    ref, want = {}, {}
    with torch.no_grad():
        tv, tvi = torch.from_numpy(verts), torch.from_numpy(vi)
        ref["normals"] = geom.vert_normals(tv, tvi).numpy()
        ref["view_cos"] = geom.compute_view_cos(tv, tvi, torch.from_numpy(camera)).numpy()
        ref["view_cos_shared"] = geom.compute_view_cos(tv, tvi, torch.from_numpy(camera[:1])).numpy()
        ref["from_uv"] = geom.sample_uv(torch.from_numpy(values_uv), torch.from_numpy(vt), torch.from_numpy(v2uv).long()).numpy()
        want["normals"] = R.vert_normals(verts, vi)
        want["view_cos"] = R.view_cos(verts, vi, camera)
        want["view_cos_shared"] = R.view_cos(verts, vi, camera[:1])
        want["from_uv"] = R.from_uv(values_uv, vt, v2uv)
        for H in R.UV_SIZES:
            index, bary64, face = R.uv_images(surf, H)
            assert np.array_equal(face, R.raster_uv(vt, vti, H, dtype=np.float32)), "float32 and float64 disagree on a texel"
            c = torch.linspace(0.5, H - 0.5, H) / H                           # make_uv_barys' own grid
            grid = torch.stack(torch.meshgrid(c, c, indexing="ij")[::-1], dim=2).reshape(-1, 2)
            tri = torch.from_numpy(vt)[torch.from_numpy(vti)[torch.from_numpy(face).clamp(min=0)]].permute(2, 0, 1, 3)
            bary = geom.bary_coords(grid, tri.reshape(3, -1, 2)).permute(1, 0).reshape(H, H, 3)
            bary[torch.from_numpy(face) < 0] = 0
            out[f"face_image{H}"], out[f"index_image{H}"] = face.astype(np.int32), index.astype(np.int32)
            ref[f"bary{H}"], want[f"bary{H}"] = bary.numpy(), bary64
        index48, bary48 = torch.from_numpy(out["index_image48"]).long(), torch.from_numpy(ref["bary48"])
        ref["to_uv"] = geom.values_to_uv(tv, index48, bary48).numpy()
        want["to_uv"] = R.to_uv(verts, out["index_image48"], ref["bary48"])
    for k in ref:
        assert ref[k].dtype == np.float32 and ref[k].shape == want[k].shape, k
        out[f"ref/{k}"] = ref[k]
        out[f"e_ref/{k}"] = np.float64(R.nerr(ref[k], want[k]))
    path = os.path.join(HERE, "golden_surface_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    print({k: float(out[f"e_ref/{k}"]) for k in ref})
    print("float32 restatement vs float64:", {
        "normals": R.nerr(R.vert_normals(verts, vi, np.float32), want["normals"]),
        "view_cos": R.nerr(R.view_cos(verts, vi, camera, np.float32), want["view_cos"]),
        "from_uv": R.nerr(R.from_uv(values_uv, vt, v2uv, np.float32), want["from_uv"]),
        "to_uv": R.nerr(R.to_uv(verts, out["index_image48"], ref["bary48"], np.float32), want["to_uv"]),
        "bary130": R.nerr(R.uv_images(surf, 130, dtype=np.float32)[1], want["bary130"])})


if __name__ == "__main__":
    main()
