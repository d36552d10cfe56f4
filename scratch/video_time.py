"""Time the GPU Motion-JPEG encoder (audio2photoreal_amd/video.py, csrc/kernels_video.h).

    python scratch/video_time.py [--out profiles/video_timing.json] [--frames 600]

Workload: 600 frames of 667 x 2048 (two 1024-wide panels: a shaded, textured figure on black that moves from frame to frame, mild
sensor-like noise), quality 90, 4:2:0.  Method of scratch/encoder_time.py: device events on the current stream around windows of
`--inner` back-to-back calls after warm-up, `--reps` windows, the median per call with the min and max in the record.  The two
launches (coefficients; entropy coding = its sizing and its writing pass) are timed on one chunk of frames, the chunk
encode_jpeg_frames itself works in; encode_jpeg_frames on all frames, device-to-host copy included.  `read_GBps` is the uint8 bytes
read over the time, `copy_fraction` that rate over the rate of a device-to-device copy of the same bytes in this process (the copy
also writes them).  Beside it, where Pillow imports, Image.save(format="JPEG") of the same frames on the host, per frame, on one
core.  Numbers, not tuning targets."""
import argparse
import io
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_frames(n, h, w, dev, step=50):
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
    ap.add_argument("--frames", type=int, default=600)
    ap.add_argument("--height", type=int, default=667)
    ap.add_argument("--width", type=int, default=2048)
    ap.add_argument("--quality", type=int, default=90)
    ap.add_argument("--subsampling", default="420")
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--inner", type=int, default=4, help="calls per timed window")
    ap.add_argument("--pil-frames", type=int, default=16)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    from audio2photoreal_amd import _lib
    from audio2photoreal_amd import video as V

    dev = torch.device("cuda:0")
    N, H, W, q, sub = args.frames, args.height, args.width, args.quality, args.subsampling
    rows_, cols_, bpm = V.mcu_grid(H, W, sub)
    chunk = min(N, max(1, (1 << 28) // (rows_ * cols_ * bpm * 128)))
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

    def row(name, frames, stat, **extra):
        n_bytes = frames * H * W * 3
        e = {"step": name, "frames": frames, **stat, "ms_per_frame": stat["median_ms"] / frames, "frames_per_s": frames / (stat["median_ms"] * 1e-3),
             "read_bytes": n_bytes, "read_GBps": n_bytes / (stat["median_ms"] * 1e-3) / 1e9, **extra}
        rows.append(e)
        print(json.dumps(e), flush=True)
        return e

    with torch.cuda.device(dev):
        frames = make_frames(N, H, W, dev)
        part = frames[:chunk]
        src = part.reshape(-1)
        dst = torch.empty_like(src)
        copy = timed(lambda: dst.copy_(src))
        copy_GBps = src.numel() / (copy["median_ms"] * 1e-3) / 1e9
        del dst

        frac = lambda stat: {"copy_fraction": copy["median_ms"] / stat["median_ms"]}
        st = timed(lambda: V.coefficients(part, q, sub))
        row("a2p_jpeg_coefficients", chunk, st, **frac(st))
        coef = V.coefficients(part, q, sub)
        _, huff = V._tables(dev)
        lib, stream = _lib.load(), _lib.current_stream(dev)
        head = V.frame_header(H, W, q, sub)
        head_t = torch.frombuffer(bytearray(head), dtype=torch.uint8).to(dev)
        tail_t = torch.frombuffer(bytearray(V.EOI), dtype=torch.uint8).to(dev)
        interval = torch.empty(chunk * rows_, dtype=torch.int64, device=dev)
        offsets = torch.empty(chunk + 1, dtype=torch.int64, device=dev)

        def entropy(out, n):
            _lib.check(lib.a2p_jpeg_entropy(_lib.ptr(coef), chunk, rows_, cols_, bpm, _lib.ptr(huff), _lib.ptr(head_t), len(head), _lib.ptr(tail_t), 2,
                                            _lib.ptr(interval), _lib.ptr(offsets), _lib.ptr(out), n, stream), "a2p_jpeg_entropy")
        st = timed(lambda: entropy(None, 0))
        row("a2p_jpeg_entropy, sizing pass (with the prefix sums)", chunk, st, **frac(st))
        entropy(None, 0)
        total = int(offsets[-1])
        out = torch.empty(total, dtype=torch.uint8, device=dev)
        st = timed(lambda: entropy(out, total))
        row("a2p_jpeg_entropy, writing pass", chunk, st, **frac(st), compressed_bytes=total, compression=chunk * H * W * 3 / total)
        st = timed(lambda: V.entropy_segments(coef, head=head, tail=V.EOI))
        row("entropy_segments (both passes, the offsets read back, the stream allocated)", chunk, st, **frac(st))
        del out, coef

        st = timed(lambda: V.encode_jpeg_frames(frames, q, sub), inner=1, reps=5)
        data, off = V.encode_jpeg_frames(frames, q, sub)
        whole = row("encode_jpeg_frames (all frames, device-to-host copy included)", N, st, copy_fraction=(copy["median_ms"] / chunk) / (st["median_ms"] / N),
                    compressed_bytes=int(len(data)), chunks=-(-N // chunk))

        pil = None
        try:
            from PIL import Image
            host = frames[:args.pil_frames].cpu().numpy()
            sizes, t0 = [], time.perf_counter()
            for f in host:
                buf = io.BytesIO()
                Image.fromarray(f, "RGB").save(buf, format="JPEG", quality=q, subsampling=2 if sub == "420" else 0)
                sizes.append(buf.tell())
            dt = time.perf_counter() - t0
            pil = {"frames": len(host), "ms_per_frame": 1e3 * dt / len(host), "bytes_per_frame": float(np.mean(sizes)),
                   "gpu_bytes_per_frame": float(np.mean(np.diff(off)[:len(host)])), "speedup_per_frame": (1e3 * dt / len(host)) / whole["ms_per_frame"]}
            print(json.dumps({"pillow": pil}), flush=True)
        except ImportError:
            pass

    res = {"workload": {"frames": N, "height": H, "width": W, "quality": q, "subsampling": sub, "chunk_frames": chunk,
                        "content": "two 1024-wide panels, a shaded textured ellipse on black, N(0, 2) noise"},
           "device": torch.cuda.get_device_name(0),
           "method": f"device events around windows of {args.inner} back-to-back calls (1 for encode_jpeg_frames), per-call median of {args.reps} (5) windows "
                     f"after {args.warmup} warm-up calls; min and max beside it",
           "device_copy": {"bytes": int(src.numel()), **copy, "GBps": copy_GBps}, "steps": rows, "pillow_host": pil, "tuned": False}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    print("encode_jpeg_frames:", rows[-1])


if __name__ == "__main__":
    main()
