"""Builds tests/golden/golden_render_v1.npz: the scene of the rendering tests, as data.

    python tests/golden/make_golden_render.py

The scene is the 437-vertex surface fixture mesh (tests/surface_restatement.py make_surface) and a second copy displaced behind it:
two layers, 874 vertices, 1584 faces, so that most pixels are covered by at least two faces with a real depth gap.  Three frames,
each with its own camera and image size (48 x 64, 64 x 48, 37 x 53); the third camera looks along the sheet at a grazing angle, so
the sheet's bumps hide one another.

Every camera is drawn again until two clearances hold on its frame, with no pixel excluded:
  * edge: no pixel centre lies within CLEARANCE_FACTOR x e_proj of a projected edge, e_proj being the largest difference between
    the float32 and the float64 projection of any vertex of the fixture (pixels);
  * depth: the winner and the runner-up of every covered pixel differ by more than CLEARANCE_FACTOR x e_depth relative, e_depth
    being the largest relative difference between the float32 and the float64 depth image.
Then the inside-or-on-boundary rule, a strict rule, float32, float64 and the GPU cannot disagree on any pixel's face, and the tests
compare face images with array_equal.  Asserted here: float32 and float64 give the same face images.  Nothing is read from the
reference: pytorch3d, which its RenderLayer calls, is not available, so the rule stated in render_restatement.py is the contract."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import render_restatement as R  # noqa: E402

MAX_DRAWS = 400      # per camera and sweep
MAX_SWEEPS = 10
UP = (0.0, 1.0, 0.0)


def draw_camera(rs, k, H, W):
    """Camera k of the fixture: 0 frontal, 1 oblique, 2 grazing; every draw jitters the eye, the target and the field of view."""
    centre = np.array([1.1, 0.9, -0.2])
    eye = centre + [np.array([0.2, -0.15, 3.4]), np.array([1.9, 1.0, 2.3]), np.array([-2.7, 0.25, 0.62])][k] + rs.uniform(-0.1, 0.1, 3)
    target = centre + rs.uniform(-0.08, 0.08, 3)
    return R.look_at(eye, target, UP, H, W, (38.0, 44.0, 27.0)[k] + rs.uniform(-2, 2), np.float32)


def main():
    rs = np.random.RandomState(11)
    surf = R.make_surface()
    mesh = R.two_layers(surf)
    verts = R.layered_frames(surf, 5, 3)
    assert (mesh["n_verts"], len(mesh["vi"])) == (874, 1584) and verts.shape == (3, 874, 3)
    out = {"vi": mesh["vi"].astype(np.int32), "vt": mesh["vt"], "vti": mesh["vti"].astype(np.int32), "verts": verts,
           "sizes": np.asarray(R.SIZES, np.int32), "clearance_factor": np.int32(R.CLEARANCE_FACTOR),
           "tex": rs.randn(3, 3, 40, 56).astype(np.float32)}
    cams, stats = [None] * 3, [None] * 3
    largest = lambda name: max([st[name] for st in stats if st is not None], default=0.0)
    for sweep in range(MAX_SWEEPS):
        # a frame is drawn again while it misses CLEARANCE_FACTOR x the LARGEST error of the three frames, not only its own
        todo = [k for k in range(3) if stats[k] is None or not (stats[k]["edge_clearance"] > R.CLEARANCE_FACTOR * largest("e_proj")
                                                                and stats[k]["depth_clearance"] > R.CLEARANCE_FACTOR * largest("e_depth"))]
        if not todo:
            break
        for k in todo:
            H, W = R.SIZES[k]
            v = verts[k:k + 1]
            stats[k] = None
            for draw in range(1, MAX_DRAWS + 1):
                K, Rt = draw_camera(rs, k, H, W)
                p64, p32 = R.project(v, K[None], Rt[None]), R.project(v, K[None], Rt[None], np.float32)
                e_proj = float(np.abs(p32[..., :2].astype(np.float64) - p64[..., :2]).max())
                edge = R.edge_clearance(v, mesh["vi"], K[None], Rt[None], H, W)
                if not edge > R.CLEARANCE_FACTOR * max(e_proj, largest("e_proj")):
                    continue
                f64 = R.rasterize(v, mesh["vi"], K[None], Rt[None], H, W, runner_up=True)
                f32 = R.rasterize(v, mesh["vi"], K[None], Rt[None], H, W, dtype=np.float32)
                if not np.array_equal(f32["face"], f64["face"]):
                    continue
                hit = f64["face"] >= 0
                e_depth = float((np.abs(f32["depth"][hit].astype(np.float64) - f64["depth"][hit]) / f64["depth"][hit]).max())
                gap = R.depth_clearance(f64)
                if gap > R.CLEARANCE_FACTOR * max(e_depth, largest("e_depth")):
                    break
            else:
                raise SystemExit(f"camera {k}: no draw out of {MAX_DRAWS} cleared every pixel of its {H} x {W} image")
            twice = np.isfinite(f64["second"]) & hit
            print(f"sweep {sweep} camera {k} ({H} x {W}): draw {draw}, e_proj {e_proj:.3e} px, edge clearance {edge:.3e} px, e_depth "
                  f"{e_depth:.3e}, depth clearance {gap:.3e}, covered {hit.mean():.2f}, covered twice {twice.mean():.2f}")
            assert hit.mean() > 0.3 and twice.sum() > 0.5 * hit.sum(), "most covered pixels must see both layers"
            cams[k] = (K, Rt)
            out[f"face{k}"], out[f"second{k}"] = f64["face"][0].astype(np.int32), f64["second"][0]
            stats[k] = {"e_proj": e_proj, "edge_clearance": edge, "e_depth": e_depth, "depth_clearance": gap, "draws": draw,
                        "covered": int(hit.sum()), "twice": int(twice.sum())}
    else:
        raise SystemExit(f"no set of three cameras cleared the largest error of the three within {MAX_SWEEPS} sweeps")
    Ks, Rts = [c[0] for c in cams], [c[1] for c in cams]
    stats = {name: [st[name] for st in stats] for name in stats[0]}
    out["K"], out["Rt"] = np.asarray(Ks, np.float32), np.asarray(Rts, np.float32)
    for name, vals in stats.items():
        out[name] = np.asarray(vals)
    # the fixture-wide statement the tests rely on: every frame clears CLEARANCE_FACTOR x the LARGEST error of the three
    assert out["edge_clearance"].min() > R.CLEARANCE_FACTOR * out["e_proj"].max(), "edge clearance against the largest e_proj"
    assert out["depth_clearance"].min() > R.CLEARANCE_FACTOR * out["e_depth"].max(), "depth clearance against the largest e_depth"
    path = os.path.join(HERE, "golden_render_v1.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
