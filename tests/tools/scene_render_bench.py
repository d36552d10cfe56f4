"""Time the multi-body scene render (SceneRasterizer.render, csrc/kernels_scene.h) against two single-body anti-aliased renders.

    python tests/tools/scene_render_bench.py --out profiles/scene_render.json                     # device events
    rocprofv3 --kernel-trace --output-format csv -d DIR -o p -- python tests/tools/scene_render_bench.py --trace-pass
    python tests/tools/scene_render_bench.py --merge-trace DIR/.../p_kernel_trace.csv --out profiles/scene_render.json

Workload: two bodies of the size of scratch/render_time.py's stand-in (a closed ellipsoid of body proportions, V = 7320, F = 14400
each), the second turned by 25 degrees and moved half a body width to the side and a little forward so that it overlaps the first,
64 frames at 1024 x 667, 2 x 2 samples per pixel, a 3 x 1024 x 1024 texture per body, over a background.

Device events (the first form): the whole SceneRasterizer.render call and, interleaved with it repetition by repetition, the two
BodyRasterizer.render_antialiased calls that existed before it (the second body's vertices moved beforehand; their two images
cannot be merged into the scene's, they only give the cost of rendering each body once).  3 warm-up calls, median of 20, minimum
and maximum kept.  The events cannot see inside one export, so the time of the resolve kernel alone comes from a kernel trace in a
run of its own (the second and third form): one warm-up call and --trace-calls measured ones; the merge drops every kernel's
warm-up dispatch and adds the mean device time per call of each kernel to the record."""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scratch"))
from render_time import ellipsoid  # noqa: E402

H, W, S, FRAMES = 1024, 667, 2, 64
KERNELS = (("scene_resolve_kernel", "resolve"), ("render_cover_kernel", "cover"), ("scene_project_kernel", "project"))


def timed_interleaved(fns: dict, reps: int, warmup: int) -> dict:
    """{name: {"median_ms", "min_ms", "max_ms", "reps"}}: the alternatives run in turn inside every repetition."""
    for _ in range(warmup):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(reps):
        for k, fn in fns.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            ms[k].append(a.elapsed_time(b))
    return {k: {"median_ms": sorted(v)[len(v) // 2], "min_ms": min(v), "max_ms": max(v), "reps": reps} for k, v in ms.items()}


def merge_trace(args):
    rows = sorted(csv.DictReader(open(args.merge_trace)), key=lambda r: int(r["Start_Timestamp"]))
    res = json.load(open(args.out)) if os.path.exists(args.out) else {}
    split = {}
    for pattern, kind in KERNELS:
        ms = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6 for r in rows if pattern in r["Kernel_Name"]]
        assert len(ms) >= 2, (pattern, len(ms))
        split[kind + "_ms"] = sum(ms[1:]) / (len(ms) - 1)                      # the first dispatch is the warm-up call's
        split["calls"] = len(ms) - 1
    split["source"] = "kernel trace in a run of its own, mean device time per call after one warm-up call (one chunk per call)"
    res["kernels"] = split
    if "scene" in res:
        res["kernels"]["resolve_share_of_scene_call"] = split["resolve_ms"] / res["scene"]["median_ms"]
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps(res["kernels"], indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=FRAMES)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-bytes", type=int, default=8 << 30, help="scratch of one chunk of frames: all frames in one chunk by default")
    ap.add_argument("--trace-pass", action="store_true", help="run under rocprofv3 --kernel-trace: one warm-up call and --trace-calls more")
    ap.add_argument("--trace-calls", type=int, default=5)
    ap.add_argument("--merge-trace", default=None, metavar="CSV", help="add the per-kernel times of a trace pass to --out")
    args = ap.parse_args()
    if args.merge_trace:
        return merge_trace(args)
    assert torch.cuda.is_available(), "timing needs the MI355X"
    from audio2photoreal_amd import render as RD
    from audio2photoreal_amd import scene as SN

    dev = torch.device("cuda:0")
    N = args.frames
    rest, vi, vt = ellipsoid()
    sway = 0.05 * np.sin(np.arange(N) * 0.1)[:, None, None] * rest[None, :, 1:2] * np.array([1.0, 0.0, 0.3])
    verts = torch.from_numpy((rest[None] + sway).astype(np.float32)).to(dev)
    width = float(rest[:, 0].max() - rest[:, 0].min())
    M = SN.placement(25.0, (0.5 * width, 0.0, 0.15 * width), (0.0, 1.0, 0.0), device=dev)
    moved = (verts @ M[:, :3].T + M[:, 3]).contiguous()                        # what the single-body call gets for the second body
    tex = [torch.randn(1, 3, 1024, 1024, device=dev) for _ in range(2)]
    bg = torch.randn(1, 3, H, W, device=dev)
    K, Rt = RD.look_at([0.25 * width, 0.0, 3.0], [0.25 * width, 0.0, 0.0], [0.0, 1.0, 0.0], H, W, 35.0, device=dev)
    sc = SN.SceneRasterizer([(vi, vt, vi), (vi, vt, vi)], H, W)
    rz = RD.BodyRasterizer.from_arrays(vi, vt, vi, H, W)

    def scene():
        return sc.render([verts, verts], tex, K, Rt, [None, M], supersample=S, background=bg, max_bytes=args.max_bytes)

    def two_calls():
        return (rz.render_antialiased(verts, tex[0], K, Rt, supersample=S, background=bg, max_bytes=args.max_bytes),
                rz.render_antialiased(moved, tex[1], K, Rt, supersample=S, background=bg, max_bytes=args.max_bytes))

    if args.trace_pass:
        for _ in range(1 + args.trace_calls):
            scene()
        torch.cuda.synchronize()
        return
    got, (one, two) = scene(), two_calls()
    share = got["body_alpha"].mean(dim=(0, 2, 3)).tolist()
    both = float(((got["body_alpha"][:, 0] > 0) & (got["body_alpha"][:, 1] > 0)).float().mean())
    hidden = float(one["alpha"].mean() + two["alpha"].mean() - got["alpha"].mean())     # coverage one body hides of the other
    del got, one, two
    res = {"workload": {"bodies": 2, "V": int(verts.shape[1]), "F": int(len(vi)), "N": N, "H": H, "W": W, "S": S,
                        "mesh": "the stand-in of scratch/render_time.py, twice: a closed ellipsoid of body proportions",
                        "texture": "3 x 1024 x 1024 per body, shared by the frames", "background": "one 3 x H x W image", "max_bytes": args.max_bytes,
                        "mean_body_alpha": share, "pixels_with_both_bodies": both, "coverage_hidden_by_the_other_body": hidden},
           "device": torch.cuda.get_device_name(0), "tuned": False,
           "method": f"device events around a whole call over all frames, the two alternatives interleaved; median of {args.reps} after "
                     f"{args.warmup} warm-up calls"}
    r = timed_interleaved({"scene": scene, "two_single_body_calls": two_calls}, args.reps, args.warmup)
    for v in r.values():
        v["frames_per_second"] = N / (v["median_ms"] * 1e-3)
    res.update(r)
    res["scene_over_two_calls"] = r["scene"]["median_ms"] / r["two_single_body_calls"]["median_ms"]
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
