"""Time the four kernels of the surface maps (audio2photoreal_amd/surface.py) with device events.

    python scratch/surface_time.py [--out profiles/surface_timing.json] [--assets static_assets.pt] [--uv-size 1024] [--frames 30] [--channels 7]

Workload: V and F of a real static_assets.pt when given, otherwise a synthetic grid mesh of about 10^4 vertices in one UV chart;
uv_size 1024, 30 frames per call, C = 7 (position 3, normal 3, view cosine 1).  After warm-up each call is timed alone, `--reps`
times, between two events on the current stream; the median and the spread are reported.  A plain device-to-device copy of
to_uv's output size is timed in the same process: the figure of interest is to_uv's written bytes per second as a fraction of
that copy's written bytes per second (the copy also reads as much as it writes).  A number, not a tuning target."""
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


def grid_mesh(nx, ny):
    vid = lambda i, j: j * nx + i
    vi = np.array([t for j in range(ny - 1) for i in range(nx - 1)
                   for t in ([vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)], [vid(i, j), vid(i + 1, j + 1), vid(i, j + 1)])])
    ii, jj = np.meshgrid(np.arange(nx), np.arange(ny))
    rs = np.random.RandomState(1)
    vt = np.stack([0.02 + 0.96 * ii / (nx - 1), 0.02 + 0.96 * jj / (ny - 1)], -1).reshape(-1, 2) + rs.uniform(-1e-3, 1e-3, (nx * ny, 2))
    rest = np.stack([ii * 0.01, jj * 0.01, 0.1 * np.sin(ii * 0.1) * np.cos(jj * 0.1)], -1).reshape(-1, 3)
    return vi, vt.astype(np.float32), rest.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--assets", default=None)
    ap.add_argument("--uv-size", type=int, default=1024)
    ap.add_argument("--frames", type=int, default=30)
    ap.add_argument("--channels", type=int, default=7)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    from audio2photoreal_amd import surface as S

    dev = torch.device("cuda:0")
    H, N, C = args.uv_size, args.frames, args.channels
    if args.assets:
        sf = S.BodySurface.from_static_assets(torch.load(args.assets, map_location="cpu", weights_only=False), uv_size=H)
        rest, mesh = np.random.RandomState(2).randn(sf.V, 3).astype(np.float32), f"topology of {os.path.basename(args.assets)}"
    else:
        vi, vt, rest = grid_mesh(100, 100)
        sf, mesh = S.BodySurface.from_arrays(vi, vt, vi, uv_size=H), "synthetic 100 x 100 grid, one chart"
    rs = np.random.RandomState(3)
    verts = torch.from_numpy(rest[None] + rs.randn(N, sf.V, 3).astype(np.float32) * 1e-3).to(dev)
    cam = torch.tensor([[0.5, 0.5, 3.0]], device=dev)
    values = torch.from_numpy(rs.randn(N, sf.V, C).astype(np.float32)).to(dev)
    uv_in = torch.from_numpy(rs.randn(N, C, H, H).astype(np.float32)).to(dev)
    sf.index_image                                                            # rasterise before anything is timed

    def raster():
        sf._img.clear()
        sf.index_image

    res = {"normals_and_view_cos": timed(lambda: sf.normals_and_view_cos(verts, cam), args.reps, args.warmup),
           "to_uv": timed(lambda: sf.to_uv(values), args.reps, args.warmup),
           "from_uv": timed(lambda: sf.from_uv(uv_in), args.reps, args.warmup),
           "uv_index": timed(raster, args.reps, args.warmup)}
    out = sf.to_uv(values)
    dst = torch.empty_like(out)
    res["copy_of_to_uv_output"] = timed(lambda: dst.copy_(out), args.reps, args.warmup)
    out_bytes = N * C * H * H * 4
    rate = lambda k: out_bytes / (res[k]["median_ms"] * 1e-3)
    res["to_uv"].update(output_bytes=out_bytes, table_bytes=24 * H * H, written_bytes_per_s=rate("to_uv"))
    res["copy_of_to_uv_output"].update(bytes=out_bytes, written_bytes_per_s=rate("copy_of_to_uv_output"))
    res["to_uv_written_rate_over_copy"] = rate("to_uv") / rate("copy_of_to_uv_output")
    res = {"workload": {"mesh": mesh, "V": sf.V, "F": sf.F, "uv_size": H, "frames": N, "channels": C,
                        "covered_texels": float((sf.face_index_image >= 0).float().mean())},
           "device": torch.cuda.get_device_name(0),
           "method": f"device events around one call (allocation of the output included), median of {args.reps} after {args.warmup} warm-up calls",
           **res, "tuned": False}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
