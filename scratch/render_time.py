"""Time the rendering exports (audio2photoreal_amd/render.py) with device events.

    python scratch/render_time.py [--out profiles/render_time.json] [--frames 600] [--reps 20]

Workload: 600 frames of a body-sized stand-in at 1024 x 667 and at 256 x 256.  No measured asset is on hand, so the mesh is an
ellipsoid of body proportions (0.5 x 1.7 x 0.3) cut into 61 x 120 vertices = 7320 vertices and 14400 triangles (the reference's
body mesh has about 7300 vertices), swaying a little from frame to frame, seen whole from the front with a 35 degree camera.  It
is closed, so every covered pixel is covered twice, by a front and a back triangle.

After warm-up each export is timed alone, `--reps` times, between two events on the current stream: a2p_render_rasterize (its four
launches together: project, key fill, cover, resolve; all three outputs), a2p_render_interpolate at C = 3 and C = 7, and
a2p_render_texture with a shared 3 x 1024 x 1024 texture.  Median, minimum and maximum are reported, and beside each median the
bytes the call must write.  One timed window is short (milliseconds): the first repetitions after an idle spell run at idle clocks,
which is what the warm-up launches are for, and the minimum-to-maximum spread says how steady the rest was.  A number, not a
tuning target; the split inside a2p_render_rasterize needs a kernel trace (rocprofv3 --kernel-trace --stats, a run of its own)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "reps": reps}


def ellipsoid(rows=61, cols=120):
    """(rest [V, 3], vi [F, 3], vt [V, 2]): a closed latitude / longitude mesh; the pole rows are small rings, not points."""
    lat = np.linspace(0.02, np.pi - 0.02, rows)[:, None]
    lon = (np.arange(cols) * 2 * np.pi / cols)[None, :]
    rest = np.stack([0.25 * np.sin(lat) * np.cos(lon), 0.85 * np.cos(lat) * np.ones_like(lon), 0.15 * np.sin(lat) * np.sin(lon)], -1)
    vid = lambda r, c: r * cols + c % cols
    vi = np.array([t for r in range(rows - 1) for c in range(cols) for t in ([vid(r, c), vid(r + 1, c), vid(r + 1, c + 1)],
                                                                             [vid(r, c), vid(r + 1, c + 1), vid(r, c + 1)])])
    vt = np.stack(np.broadcast_arrays(lon / (2 * np.pi), lat / np.pi), -1).reshape(-1, 2)
    return rest.reshape(-1, 3).astype(np.float32), vi, vt.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    from audio2photoreal_amd import _lib, render as RD

    dev = torch.device("cuda:0")
    N = args.frames
    rest, vi, vt = ellipsoid()
    V, F = len(rest), len(vi)
    sway = 0.05 * np.sin(np.arange(N) * 0.1)[:, None, None] * rest[None, :, 1:2] * np.array([1.0, 0.0, 0.3])
    verts = torch.from_numpy((rest[None] + sway).astype(np.float32)).to(dev)
    tex = torch.randn(1, 3, 1024, 1024, device=dev)
    lib, p, stream = _lib.load(), _lib.ptr, _lib.current_stream(dev)
    res = {"workload": {"V": V, "F": F, "N": N, "mesh": "stand-in: a closed ellipsoid of body proportions, 61 x 120 vertices (no measured asset on hand)",
                        "camera": "look_at from 3.0 in front, 35 degrees vertical, the whole mesh in view"},
           "device": torch.cuda.get_device_name(0), "tuned": False,
           "method": f"device events around one export, median of {args.reps} after {args.warmup} warm-up calls; short windows: see min / max"}
    for H, W in ((1024, 667), (256, 256)):
        rz = RD.BodyRasterizer.from_arrays(vi, vt, vi, H, W)
        K, Rt = RD.look_at([0.0, 0.0, 3.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0], H, W, 35.0, device=dev)
        t = rz._tables(dev)
        proj = torch.empty(N, V, 3, device=dev)
        key = torch.empty(N, H, W, dtype=torch.int64, device=dev)
        face = torch.empty(N, H, W, dtype=torch.int32, device=dev)
        bary, depth = torch.empty(N, H, W, 3, device=dev), torch.empty(N, H, W, device=dev)
        values = {C: torch.randn(N, V, C, device=dev) for C in (3, 7)}
        out = {C: torch.empty(N, C, H, W, device=dev) for C in (3, 7)}

        def rasterize():
            _lib.check(lib.a2p_render_rasterize(p(verts), N, V, p(t["vi"]), F, p(K), 0, p(Rt), 0, H, W, 1e-3, p(proj), p(key), p(face), p(bary),
                                                p(depth), stream), "a2p_render_rasterize")

        def interpolate(C):
            _lib.check(lib.a2p_render_interpolate(p(values[C]), N, V, C, p(t["vi"]), F, p(face), p(bary), H, W, p(out[C]), stream),
                       "a2p_render_interpolate")

        def texture():
            _lib.check(lib.a2p_render_texture(p(face), p(bary), N, H, W, p(t["vt"]), len(vt), p(t["vti"]), F, p(tex), 0, 3, 1024, 1024, 0,
                                              p(out[3]), stream), "a2p_render_texture")

        r = {"a2p_render_rasterize": {**timed(rasterize, args.reps, args.warmup), "bytes_written": N * (V * 12 + H * W * 28)}}
        covered = float((face >= 0).float().mean())
        again = rz.rasterize(verts, K, Rt)                                    # the public call runs the same launches
        assert torch.equal(again["face"], face) and torch.equal(again["bary"], bary) and torch.equal(again["depth"], depth)
        del again
        for C in (3, 7):
            r[f"a2p_render_interpolate_C{C}"] = {**timed(lambda: interpolate(C), args.reps, args.warmup), "bytes_written": N * C * H * W * 4}
        r["a2p_render_texture_C3"] = {**timed(texture, args.reps, args.warmup), "bytes_written": N * 3 * H * W * 4}
        for v in r.values():
            v["frames_per_second"] = N / (v["median_ms"] * 1e-3)
            v["written_bytes_per_s"] = v["bytes_written"] / (v["median_ms"] * 1e-3)
        r["covered_fraction"] = covered
        r["pixels_per_face"] = covered * H * W * 2 / F                        # closed mesh: front and back
        res[f"{H}x{W}"] = r
        del proj, key, face, bary, depth, values, out
        torch.cuda.empty_cache()
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
