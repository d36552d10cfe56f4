"""Time the anti-aliased renderer (BodyRasterizer.render_antialiased, csrc/kernels_render_aa.h) against the composition it replaces.

    python scratch/render_aa_time.py --out profiles/render_aa_time.json                      # device events
    rocprofv3 --kernel-trace --output-format csv -d DIR -o p -- python scratch/render_aa_time.py --trace-pass DIR/manifest.json
    python scratch/render_aa_time.py --merge-trace DIR/.../p_kernel_trace.csv --manifest DIR/manifest.json --out profiles/render_aa_time.json

Workload: that of scratch/render_time.py (profiles/render_time.json): 600 frames of the body-sized ellipsoid, V = 7320, F = 14400,
at 1024 x 667 and 256 x 256, a shared 3 x 1024 x 1024 texture, for s = 1 to 4 samples per axis.

Device events (the first form): per size and s, the whole render_antialiased call and, interleaved with it repetition by
repetition, the composition of existing launches -- rasterize and sample_texture at (s H, s W) through K', then F.avg_pool2d --
each over all 600 frames in chunks under the same --max-bytes budget of scratch and intermediates.  3 warm-up calls, median of 20,
minimum and maximum kept.  The events cannot see inside one export, so the split of a call into project + key fill + cover and the
fused resolve comes from a kernel trace in a run of its own (the second and third form): the trace pass makes one warm-up call and
--trace-calls measured ones per configuration and writes how many dispatches of the fused kernel belong to each; the merge walks
the dispatches in time order, cuts them at those counts, and adds the mean device time per call of each kernel to the record."""
import argparse
import csv
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scratch"))
from render_time import ellipsoid  # noqa: E402

SIZES = ((1024, 667), (256, 256))
SAMPLES = (1, 2, 3, 4)


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


def scene(N, dev):
    rest, vi, vt = ellipsoid()
    sway = 0.05 * np.sin(np.arange(N) * 0.1)[:, None, None] * rest[None, :, 1:2] * np.array([1.0, 0.0, 0.3])
    return torch.from_numpy((rest[None] + sway).astype(np.float32)).to(dev), vi, vt, torch.randn(1, 3, 1024, 1024, device=dev)


def merge_trace(args):
    rows = list(csv.DictReader(open(args.merge_trace)))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    manifest = json.load(open(args.manifest))
    res = json.load(open(args.out)) if os.path.exists(args.out) else {}
    kinds = (("render_aa_kernel", "fused_resolve"), ("render_cover_kernel", "cover"), ("render_project_scaled_kernel", "project"))
    at = 0
    for cfg in manifest["configs"]:
        seen, calls, sums = 0, 0, {"fused_resolve": 0.0, "cover": 0.0, "project": 0.0, "key_fill": 0.0}
        first = at
        while seen < cfg["fused_dispatches"]:                                 # this configuration's dispatches end with its last fused kernel
            seen += "render_aa_kernel" in rows[at]["Kernel_Name"]
            at += 1
        skip = 0
        for r in rows[first:at]:                                              # the warm-up call's dispatches come first and are left out
            name = r["Kernel_Name"]
            if skip < cfg["warmup_fused_dispatches"]:
                skip += "render_aa_kernel" in name
                continue
            kind = next((k for pat, k in kinds if pat in name), "key_fill")
            sums[kind] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-6
        calls = cfg["calls"]
        split = {k + "_ms": v / calls for k, v in sums.items()}
        split["project_fill_cover_ms"] = split["project_ms"] + split["key_fill_ms"] + split["cover_ms"]
        split["source"] = f"kernel trace, mean device time per call over {calls} calls after one warm-up call"
        res.setdefault(cfg["size"], {}).setdefault(f"s{cfg['s']}", {})["kernels"] = split
    assert at <= len(rows)
    with open(args.out, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(json.dumps({k: v for k, v in res.items() if "x" in k}, indent=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max-bytes", type=int, default=8 << 30, help="scratch and intermediates of one chunk of frames, for both alternatives")
    ap.add_argument("--trace-pass", default=None, metavar="MANIFEST", help="run under rocprofv3 --kernel-trace: a few calls per configuration")
    ap.add_argument("--trace-calls", type=int, default=3)
    ap.add_argument("--merge-trace", default=None, metavar="CSV", help="add the per-kernel split of a trace pass to --out")
    ap.add_argument("--manifest", default=None)
    args = ap.parse_args()
    if args.merge_trace:
        return merge_trace(args)
    assert torch.cuda.is_available(), "timing needs the MI355X"
    import torch.nn.functional as F
    from audio2photoreal_amd import render as RD

    dev = torch.device("cuda:0")
    N = args.frames
    verts, vi, vt, tex = scene(N, dev)
    V, nF = verts.shape[1], len(vi)
    res = {"workload": {"V": V, "F": nF, "N": N, "mesh": "the stand-in of scratch/render_time.py: a closed ellipsoid of body proportions",
                        "texture": "shared 3 x 1024 x 1024", "max_bytes": args.max_bytes},
           "device": torch.cuda.get_device_name(0), "tuned": False,
           "method": f"device events around a whole call over all frames, the two alternatives interleaved; median of {args.reps} after "
                     f"{args.warmup} warm-up calls"}
    manifest = {"configs": []}
    for H, W in SIZES:
        rz = RD.BodyRasterizer.from_arrays(vi, vt, vi, H, W)
        K, Rt = RD.look_at([0.0, 0.0, 3.0], [0.0, 0.0, 0.0], [0.0, 1.0, 0.0], H, W, 35.0, device=dev)
        out = torch.empty(N, 3, H, W, device=dev)
        for s in SAMPLES:
            big = RD.BodyRasterizer.from_arrays(vi, vt, vi, s * H, s * W)
            Ks = K.clone()
            Ks[:2] *= s
            fused_step = min(N, max(1, args.max_bytes // (12 * V + 8 * s * s * H * W)))       # render_antialiased's own chunking
            step = max(1, args.max_bytes // (12 * V + (8 + 20 + 12) * s * s * H * W))         # proj; key, fragments and colour per sample

            def fused():
                return rz.render_antialiased(verts, tex, K, Rt, supersample=s, max_bytes=args.max_bytes)

            def composition():
                for a in range(0, N, step):
                    frag = big.rasterize(verts[a:a + step], Ks, Rt)
                    out[a:a + step] = F.avg_pool2d(big.sample_texture(frag, tex), s)
                return out

            if args.trace_pass:
                for _ in range(1 + args.trace_calls):
                    fused()
                torch.cuda.synchronize()
                chunks = -(-N // fused_step)
                manifest["configs"].append({"size": f"{H}x{W}", "s": s, "calls": args.trace_calls, "warmup_fused_dispatches": chunks,
                                            "fused_dispatches": chunks * (1 + args.trace_calls)})
                continue
            got, ref = fused(), composition()
            covered = got["alpha"].mean().item()
            # the same image up to float32 rounding: on this 1024-texel noise texture one ulp of u moves the sample by 6e-5 texels
            # between unrelated values, and the two kernels contract the uv sums differently (measured 1.5e-4 at s = 1)
            diff = (got["render"] - ref).abs().max().item() / ref.abs().max().item()
            assert diff < 1e-3, diff
            del got, ref
            r = timed_interleaved({"render_antialiased": fused, "composition": composition}, args.reps, args.warmup)
            for v in r.values():
                v["frames_per_second"] = N / (v["median_ms"] * 1e-3)
            r["render_antialiased"]["frames_per_chunk"], r["composition"]["frames_per_chunk"] = fused_step, min(N, step)
            r["fused_over_composition"] = r["render_antialiased"]["median_ms"] / r["composition"]["median_ms"]
            r["mean_alpha"], r["max_normalised_difference"] = covered, diff
            r["composition_extra_bytes_per_pixel"] = s * s * (20 + 4 * 3)
            res.setdefault(f"{H}x{W}", {})[f"s{s}"] = r
            torch.cuda.empty_cache()
    if args.trace_pass:
        with open(args.trace_pass, "w") as f:
            json.dump(manifest, f)
        return
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
