"""Builds tests/golden/golden_scene_v1.npz: cameras, placements, textures and backgrounds for the two-body scene tests, as data.

    python tests/golden/make_golden_scene.py

Body 0 is the scene of golden_render_v1: the 437-vertex fixture sheet and its copy behind it, 874 vertices, 1584 faces,
layered_frames(surf, 5, 3).  Body 1 is the single sheet, 437 vertices, 792 faces, with frames of its own (make_frames(surf,
scene_restatement.BODY1_SEED, 3)), a texture of another size and a placement that puts it partly in front of body 0.  Five frames
(scene_restatement.FRAMES), each a camera type of make_golden_render.draw_camera (frame k shows both bodies' frame `type`), a number
of samples per axis s and an image size.  The placement is chosen per frame (PLACEMENTS): body 1 turned by 35 degrees so that it
crosses both layers of body 0, except for the oblique camera, where the crossing lines leave no sample clear in depth and body 1
stands in front instead.  It is stored as float32: the float32 and the float64 run start from the same matrix.

A camera is drawn again until, on the merged scene's s H x s W sample grid through K', the two clearances hold with CLEARANCE_FACTOR =
8 against the largest float32 error over all frames, no sample excluded, and float32 and float64 give the same sample faces
(scene_restatement.clearances: the float32 run places the vertices in float32, so the placement's rounding is part of the error).
Every s > 1 frame must hold at least MIN_BOTH pixels with samples of both bodies and MIN_PARTLY partly covered pixels; a draw that
does not is drawn again.  The generator stops with an error rather than exclude a sample.

Stored per frame k: K{k}, Rt{k}, M{k} [3, 4], tex{k}_0 [3, 40, 56], tex{k}_1 [3, 23, 31], bg{k} [3, H, W], the float64 sample faces
face{k} [s H, s W] (global indices) and the statistics.  Nothing is read from the reference."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import render_aa_restatement as A  # noqa: E402
import scene_restatement as SC  # noqa: E402
from make_golden_render import MAX_SWEEPS, UP, draw_camera  # noqa: E402

MAX_DRAWS = 600
PIVOT = (1.1, 0.9, 0.0)
CROSSING = (35.0, (0.05, 0.03, -0.22))          # yaw in degrees about UP through PIVOT, then this offset
IN_FRONT = (20.0, (0.3, 0.1, 0.5))
PLACEMENTS = (CROSSING, CROSSING, CROSSING, IN_FRONT, CROSSING)               # per frame of scene_restatement.FRAMES


def main():
    rs = np.random.RandomState(29)
    bodies, verts = SC.fixture_bodies()
    assert [b["n_verts"] for b in bodies] == [874, 437] and [len(b["vi"]) for b in bodies] == [1584, 792]
    n = len(SC.FRAMES)
    out = {"frames": np.asarray(SC.FRAMES, np.int32), "clearance_factor": np.int32(SC.CLEARANCE_FACTOR)}
    cams, stats = [None] * n, [None] * n
    F = SC.CLEARANCE_FACTOR
    largest = lambda name: max([st[name] for st in stats if st is not None], default=0.0)
    cleared = lambda st: st["edge_clearance"] > F * largest("e_proj") and st["depth_clearance"] > F * largest("e_depth")
    for sweep in range(MAX_SWEEPS):
        todo = [k for k in range(n) if stats[k] is None or not cleared(stats[k])]
        if not todo:
            break
        for k in todo:
            kind, s, H, W = SC.FRAMES[k]
            v = [x[kind:kind + 1] for x in verts]
            M = SC.placement(PLACEMENTS[k][0], PLACEMENTS[k][1], UP, PIVOT).astype(np.float32)
            stats[k] = None
            for draw in range(1, MAX_DRAWS + 1):
                K, Rt = draw_camera(rs, kind, H, W)
                c = SC.clearances(bodies, v, [None, M], K[None], Rt[None], H, W, s)
                count = A.block_count(c["f64"]["face"] >= 0, s)
                partly, both = int(((count > 0) & (count < s * s)).sum()), int(SC.both_bodies(c["f64"], s).sum())
                if (c["same_faces"] and c["edge_clearance"] > F * max(c["e_proj"], largest("e_proj"))
                        and c["depth_clearance"] > F * max(c["e_depth"], largest("e_depth"))
                        and (s == 1 or (partly >= SC.MIN_PARTLY and both >= SC.MIN_BOTH))):
                    break
            else:
                raise SystemExit(f"frame {k}: no draw out of {MAX_DRAWS} cleared every sample of its {s * H} x {s * W} grid")
            face = c["f64"]["face"][0]
            print(f"sweep {sweep} frame {k} (type {kind}, s {s}, {H} x {W}): draw {draw}, e_proj {c['e_proj']:.3e} px, edge clearance "
                  f"{c['edge_clearance']:.3e} px, e_depth {c['e_depth']:.3e}, depth clearance {c['depth_clearance']:.3e}, partly covered "
                  f"{partly}, both bodies {both} of {H * W}", flush=True)
            cams[k] = (K, Rt, M)
            out[f"face{k}"] = face.astype(np.int32)
            stats[k] = {name: c[name] for name in ("e_proj", "edge_clearance", "e_depth", "depth_clearance")}
            stats[k].update(draws=draw, partly=partly, both=both, covered=int((face >= 0).sum()),
                            covered1=int((c["f64"]["body"][0] == 1).sum()))
    else:
        raise SystemExit(f"no set of cameras cleared the largest error of the {n} frames within {MAX_SWEEPS} sweeps")
    for k, (kind, s, H, W) in enumerate(SC.FRAMES):
        out[f"K{k}"], out[f"Rt{k}"], out[f"M{k}"] = cams[k][0].astype(np.float32), cams[k][1].astype(np.float32), cams[k][2]
        for p, (Ht, Wt) in enumerate(SC.TEX_SIZES):
            out[f"tex{k}_{p}"] = rs.randn(3, Ht, Wt).astype(np.float32)
        out[f"bg{k}"] = rs.randn(3, H, W).astype(np.float32)
    for name in stats[0]:
        out[name] = np.asarray([st[name] for st in stats])
    assert out["edge_clearance"].min() > F * out["e_proj"].max(), "edge clearance against the largest e_proj"
    assert out["depth_clearance"].min() > F * out["e_depth"].max(), "depth clearance against the largest e_depth"
    assert all(out["both"][k] >= SC.MIN_BOTH and out["partly"][k] >= SC.MIN_PARTLY for k in range(n) if SC.FRAMES[k][1] > 1)
    path = os.path.join(HERE, "golden_scene_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
