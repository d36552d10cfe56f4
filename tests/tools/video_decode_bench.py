"""Time the GPU JPEG reader (audio2photoreal_amd/video.py decode_jpeg_frames, csrc/kernels_video_decode.h).

    python tests/tools/video_decode_bench.py [--out profiles/video_decode.json] [--frames 128]

Workload: a 4:2:0 clip at the renderer's frame size, 667 x 2048 (two 1024-wide panels: a shaded, textured figure on black that moves
from frame to frame, mild sensor-like noise), quality 90, encoded by this package.  Method: device events on the current stream around
windows of `--inner` back-to-back calls after warm-up, `--reps` windows, the median per call with the min and max beside it.  Timed:
the integer stage (a2p_jpeg_restarts and a2p_jpeg_decode_entropy, with the upload of the compressed bytes), the arithmetic stage
(a2p_jpeg_pixels), decode_jpeg_frames from host bytes to GPU frames, and for scale the encoder on the same frames in the same run;
where Pillow imports, Image.open(...).convert("RGB") of the same files on the host, per frame, on one core.  Numbers, not tuning
targets."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def make_frames(n, h, w, dev, step=32):
    """uint8 [n, h, w, 3]: per 1024-wide panel an ellipse with a smooth shading and a fine texture on black, drifting over the frames."""
    out = torch.empty(n, h, w, 3, dtype=torch.uint8, device=dev)
    y = torch.arange(h, device=dev, dtype=torch.float32)[None, :, None]
    x = torch.arange(w, device=dev, dtype=torch.float32)[None, None, :]
    gen = torch.Generator(device=dev).manual_seed(1)
    for a in range(0, n, step):
        t = torch.arange(a, min(n, a + step), device=dev, dtype=torch.float32)[:, None, None]
        xp = x % 1024
        cx, cy = 512 + 60 * torch.sin(t / 17), h / 2 + 25 * torch.cos(t / 23)
        inside = (((xp - cx) / 230) ** 2 + ((y - cy) / 300) ** 2) < 1
        shade = 0.55 + 0.35 * torch.cos((xp - cx) / 160) * torch.cos((y - cy) / 210)
        tex = 0.08 * torch.sin(xp / 3.1 + t / 5) * torch.sin(y / 2.7)
        rgb = torch.stack([(shade + tex) * 230, (shade * 0.8 + tex) * 210, (shade * 0.7 - tex) * 200], -1)
        rgb = rgb * inside[..., None] + 2.0 * torch.randn(rgb.shape, device=dev, generator=gen)
        out[a:a + step] = rgb.clip(0, 255).to(torch.uint8)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--height", type=int, default=667)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=4, help="calls per timed window")
    ap.add_argument("--pil-frames", type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    from audio2photoreal_amd import video as V

    dev = torch.device("cuda:0")
    N, H, W, q = args.frames, args.height, args.width, args.quality
    rows = []

    def window(fn, inner):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / inner

    def timed(fn, inner=None, reps=None):
        inner, reps = inner or args.inner, reps or args.reps
        for _ in range(args.warmup):
            fn()
        torch.cuda.synchronize()
        v = sorted(window(fn, inner) for _ in range(reps))
        return {"median_ms": v[len(v) // 2], "min_ms": v[0], "max_ms": v[-1]}

    def row(name, stat, **extra):
        e = {"step": name, "frames": N, **stat, "ms_per_frame": stat["median_ms"] / N, "frames_per_s": N / (stat["median_ms"] * 1e-3), **extra}
        rows.append(e)
        print(json.dumps(e), flush=True)
        return e

    with torch.cuda.device(dev):
        frames = make_frames(N, H, W, dev)
        data, off = V.encode_jpeg_frames(frames, q, "420")
        files = [data[off[n]:off[n + 1]].tobytes() for n in range(N)]
        headers = V._parse_all(*V._jpeg_files(files, None))
        segments = [memoryview(f)[h["segment"][0]:h["segment"][1]] for f, h in zip(files, headers)]
        compressed = int(off[-1])

        row("a2p_jpeg_restarts + a2p_jpeg_decode_entropy (with the upload of the compressed bytes)",
            timed(lambda: V._entropy_stage(segments, headers[0], dev)), compressed_bytes=compressed)
        coef, status = V._entropy_stage(segments, headers[0], dev)
        assert not bool(status.any())
        qt = V.header_qtabs(headers[0])
        out = torch.empty(N, H, W, 3, dtype=torch.uint8, device=dev)
        st = timed(lambda: V.pixels(coef, H, W, qt, "420", out))
        row("a2p_jpeg_pixels", st, written_GBps=N * H * W * 3 / (st["median_ms"] * 1e-3) / 1e9)
        del coef
        whole = row("decode_jpeg_frames (host bytes in, GPU frames out, the status read back)",
                    timed(lambda: V.decode_jpeg_frames(files, out=out), inner=1, reps=5))
        psnr = float(10 * torch.log10(255.0 ** 2 / ((out.float() - frames.float()) ** 2).mean()))
        row("encode_jpeg_frames on the same frames (device-to-host copy included), for scale",
            timed(lambda: V.encode_jpeg_frames(frames, q, "420"), inner=1, reps=5))

        pil = None
        try:
            from PIL import Image
            k = min(N, args.pil_frames)
            t0 = time.perf_counter()
            for f in files[:k]:
                np.asarray(Image.open(io.BytesIO(f)).convert("RGB"))
            dt = time.perf_counter() - t0
            pil = {"frames": k, "ms_per_frame": 1e3 * dt / k, "speedup_per_frame": (1e3 * dt / k) / whole["ms_per_frame"]}
            print(json.dumps({"pillow": pil}), flush=True)
        except ImportError:
            pass

    res = {"workload": {"frames": N, "height": H, "width": W, "quality": q, "subsampling": "420", "compressed_bytes": compressed,
                        "restart_intervals_per_frame": V.decode_grid(headers[0])[0], "round_trip_psnr_db": psnr,
                        "content": "two 1024-wide panels, a shaded textured ellipse on black, N(0, 2) noise"},
           "device": torch.cuda.get_device_name(0),
           "method": f"device events around windows of {args.inner} back-to-back calls (1 for the whole-clip rows), per-call median of {args.reps} (5) "
                     f"windows after {args.warmup} warm-up calls; min and max beside it",
           "steps": rows, "pillow_host": pil, "tuned": False}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    print("decode_jpeg_frames:", whole)


if __name__ == "__main__":
    main()
