"""Timing of the test-split batch assembly (a2p_dataset_batch, csrc/kernels_dataset.h) at B = 8, T = 600, for face and pose:

  kernel    the one launch of CaptureBatches.launch into preallocated outputs, HIP events, median of --runs after warm-up
  torch     the same batch from the same resident takes with torch ops on the GPU (index, subtract, divide, cast, transpose,
            stack): what a user of the package would write without the kernel
  copy      a device-to-device copy moving the same number of bytes (read + written): the bandwidth ceiling

The takes are larger than the 256 MiB last-level cache and every run takes other chunks, so reads come from HBM.  Bytes are
counted from the shapes.  Needs the MI355X; writes one JSON (default profiles/dataset_batch.json).

    python tests/tools/dataset_batch_bench.py [--runs 30] [--out profiles/dataset_batch.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import dataset_restatement as R  # noqa: E402
from audio2photoreal_amd.data.batches import CaptureBatches  # noqa: E402
from audio2photoreal_amd.data.capture import Take  # noqa: E402

B, T, SPF = 8, 600, 1600


def make_takes(n=4, frames=6100, seed=1):
    rs = np.random.RandomState(seed)
    takes = []
    for k in range(n):
        present = np.ones(frames, np.uint8)
        present[rs.choice(frames, 200, replace=False)] = 0
        audio = (rs.randint(-6000, 6000, (frames * SPF, 2)).astype(np.float32) / np.float32(32768.0))
        takes.append(Take(f"take{k}", rs.standard_normal((frames, 104)).astype(np.float32), rs.standard_normal((frames, 256)),
                          present, audio))
    return takes


def torch_batch(d, idx):
    inp, kf, miss, audio = [], [], [], []
    amean = torch.tensor(d.amean, device=d.device)
    astd = float(d.astd[0])
    for i in idx:
        k, s = int(d.plan[i, 0]), int(d.plan[i, 1])
        v = (d._motion[k][s:s + T].double() - d._mean) / d._std
        if d.face:
            m = d._present[k][s:s + T, None].double().expand(T, d.C)
            v = v * m
            miss.append(m.float())
        else:
            miss.append(torch.ones(T, d.C, device=d.device))
        v = v.float() + 0.0
        inp.append(v.t()[:, None, :])
        kf.append(v[::d.step])
        audio.append((d._audio[k][s * SPF:(s + T) * SPF] - amean) / astd + 0.0)
    return torch.stack(inp), torch.stack(kf), torch.stack(miss), torch.stack(audio)


INNER = 10   # calls between one pair of events: a lone ~50 us launch would be timed together with the host's launch latency


def timed(fn, runs, warmup=5):
    """(median, min, max) ms per call over `runs` samples of INNER back-to-back calls each."""
    for i in range(warmup):
        fn(i)
    torch.cuda.synchronize()
    ms = []
    for r in range(runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for j in range(INNER):
            fn(r * INNER + j)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / INNER)
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dataset_batch.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "this measurement needs the MI355X"
    takes = make_takes()
    stats = R.golden_stats()
    out = {"B": B, "T": T, "runs": args.runs, "calls_per_run": INNER, "device": torch.cuda.get_device_name(0), "formats": {}}
    for fmt in ("face", "pose"):
        d = CaptureBatches(takes, stats, fmt, T=T, seed=10, device="cuda")
        n = len(d)
        sets = [[(r * B + j) % n for j in range(B)] for r in range(args.runs * INNER + 5)]
        gt, kw = d.batch(sets[0])
        y = kw["y"]
        ref = torch_batch(d, sets[0])
        same = all(torch.equal(a.view(torch.int32), b.contiguous().view(torch.int32))
                   for a, b in zip((gt, y["keyframes"], y["missing"], y["audio"]), ref))
        outs = (gt, y["keyframes"], y["missing"], y["audio"])
        esz = 8 if fmt == "face" else 4
        read = B * T * (d.C * esz + (1 if d.face else 0) + SPF * 2 * 4)
        written = sum(t.numel() * 4 for t in outs)
        moved = read + written
        k_med, k_min, k_max = timed(lambda i: d.launch(sets[i % len(sets)], *outs), args.runs)
        t_med, t_min, t_max = timed(lambda i: torch_batch(d, sets[i % len(sets)]), args.runs)
        half = moved // 2 // 4
        srcs = [torch.empty(half, dtype=torch.float32, device="cuda").normal_() for _ in range(6)]   # 6 x ~64 MB: past the cache
        dst = torch.empty(half, dtype=torch.float32, device="cuda")
        c_med, c_min, c_max = timed(lambda i: dst.copy_(srcs[i % len(srcs)]), args.runs)
        out["formats"][fmt] = {
            "bytes_read": read, "bytes_written": written, "resident_bytes": d.resident_bytes, "torch_formulation_same_bits": bool(same),
            "kernel_ms": {"median": k_med, "min": k_min, "max": k_max}, "torch_ms": {"median": t_med, "min": t_min, "max": t_max},
            "copy_ms": {"median": c_med, "min": c_min, "max": c_max},
            "kernel_GBps": moved / k_med / 1e6, "torch_GBps": moved / t_med / 1e6, "copy_GBps": moved / c_med / 1e6,
            "torch_over_kernel": t_med / k_med, "kernel_share_of_copy_ceiling": c_med / k_med}
        print(fmt, json.dumps(out["formats"][fmt]))
        del d, srcs, dst
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
