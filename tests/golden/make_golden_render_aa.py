"""Builds tests/golden/golden_render_aa_v1.npz: cameras, textures and backgrounds for the anti-aliasing tests, as data.

    python tests/golden/make_golden_render_aa.py

The scene is that of golden_render_v1 (make_golden_render.py): the 437-vertex fixture sheet and its copy behind it, 874 vertices, 1584
faces, layered_frames(surf, 5, 3).  Four frames (render_aa_restatement.FRAMES), each a camera type of make_golden_render.draw_camera
(0 frontal, 1 oblique, 2 grazing; frame k shows the scene's frame `type`), a number of samples per axis s and an image size:
(0, 2, 24, 32), (1, 3, 21, 16), (2, 4, 9, 13), (0, 4, 12, 16).

A camera is drawn again until, on its s H x s W sample grid seen through K' (K with its first two rows times s in float32), the two
clearances of golden_render_v1 hold with the same factor, CLEARANCE_FACTOR = 8, and no sample excluded:
  * edge: no sample centre lies within CLEARANCE_FACTOR x e_proj of a projected edge (e_proj: the largest float32 projection error);
  * depth: winner and runner-up of every covered sample differ by more than CLEARANCE_FACTOR x e_depth relative;
and float32 and float64 give the same sample-face image.  As there, every frame must clear the LARGEST error of the four.  The
cameras of golden_render_v1 itself do not clear on supersampled grids, which is why these are drawn anew.

Stored per frame k: K{k}, Rt{k}, a random texture tex{k} [3, 40, 56], a random background bg{k} [3, H, W], the float64 sample faces
face{k} [s H, s W] and the statistics (also: how many pixels are partly covered, and in how many more than one face wins a
sample -- silhouettes and occlusion edges inside pixels).  Nothing is read from the reference: pytorch3d, which its RenderLayer
calls, is not available, so the rule stated in render_aa_restatement.py is the contract."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import render_aa_restatement as A  # noqa: E402
import render_restatement as R  # noqa: E402
from make_golden_render import MAX_DRAWS, MAX_SWEEPS, draw_camera  # noqa: E402


def main():
    rs = np.random.RandomState(23)
    surf = R.make_surface()
    mesh = R.two_layers(surf)
    verts = R.layered_frames(surf, 5, 3)
    assert (mesh["n_verts"], len(mesh["vi"])) == (874, 1584) and verts.shape == (3, 874, 3)
    n = len(A.FRAMES)
    out = {"frames": np.asarray(A.FRAMES, np.int32), "clearance_factor": np.int32(R.CLEARANCE_FACTOR)}
    cams, stats = [None] * n, [None] * n
    largest = lambda name: max([st[name] for st in stats if st is not None], default=0.0)
    cleared = lambda st: (st["edge_clearance"] > R.CLEARANCE_FACTOR * largest("e_proj")
                          and st["depth_clearance"] > R.CLEARANCE_FACTOR * largest("e_depth"))
    for sweep in range(MAX_SWEEPS):
        todo = [k for k in range(n) if stats[k] is None or not cleared(stats[k])]
        if not todo:
            break
        for k in todo:
            kind, s, H, W = A.FRAMES[k]
            v = verts[kind:kind + 1]
            stats[k] = None
            for draw in range(1, MAX_DRAWS + 1):
                K, Rt = draw_camera(rs, kind, H, W)
                c = A.clearances(v, mesh["vi"], K[None], Rt[None], H, W, s)
                if (c["same_faces"] and c["edge_clearance"] > R.CLEARANCE_FACTOR * max(c["e_proj"], largest("e_proj"))
                        and c["depth_clearance"] > R.CLEARANCE_FACTOR * max(c["e_depth"], largest("e_depth"))):
                    break
            else:
                raise SystemExit(f"frame {k}: no draw out of {MAX_DRAWS} cleared every sample of its {s * H} x {s * W} grid")
            face = c["f64"]["face"][0]
            count = A.block_count(face >= 0, s)
            partly = int(((count > 0) & (count < s * s)).sum())
            several = int((A.winning_faces(face, s) > 1).sum())
            print(f"sweep {sweep} frame {k} (type {kind}, s {s}, {H} x {W}): draw {draw}, e_proj {c['e_proj']:.3e} px, edge clearance "
                  f"{c['edge_clearance']:.3e} px, e_depth {c['e_depth']:.3e}, depth clearance {c['depth_clearance']:.3e}, partly covered "
                  f"{partly}, more than one winning face {several} of {H * W}")
            assert partly > 0 and several > 0, "the frame must hold silhouettes and occlusion edges inside pixels"
            cams[k] = (K, Rt)
            out[f"face{k}"] = face.astype(np.int32)
            stats[k] = {name: c[name] for name in ("e_proj", "edge_clearance", "e_depth", "depth_clearance")}
            stats[k].update(draws=draw, partly=partly, several=several, covered=int((face >= 0).sum()))
    else:
        raise SystemExit(f"no set of cameras cleared the largest error of the {n} frames within {MAX_SWEEPS} sweeps")
    for k, (kind, s, H, W) in enumerate(A.FRAMES):
        out[f"K{k}"], out[f"Rt{k}"] = cams[k][0].astype(np.float32), cams[k][1].astype(np.float32)
        out[f"tex{k}"] = rs.randn(3, 40, 56).astype(np.float32)
        out[f"bg{k}"] = rs.randn(3, H, W).astype(np.float32)
    for name in stats[0]:
        out[name] = np.asarray([st[name] for st in stats])
    assert out["edge_clearance"].min() > R.CLEARANCE_FACTOR * out["e_proj"].max(), "edge clearance against the largest e_proj"
    assert out["depth_clearance"].min() > R.CLEARANCE_FACTOR * out["e_depth"].max(), "depth clearance against the largest e_depth"
    path = os.path.join(HERE, "golden_render_aa_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
