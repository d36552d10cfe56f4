"""Time the two launches of the posed geometry (audio2photoreal_amd/skinning.py) with device events.

    python scratch/skinning_time.py [--out profiles/skinning_timing.json] [--joints 160] [--verts 8192] [--k 8] [--frames 4800]

Workload: a synthetic skeleton (no measured asset is on hand: random parents among the six preceding joints, 1..K influences per
vertex), N frames = 8 samples of 600.  After warm-up each launch is timed alone, `--reps` times, between two events on the
current stream; the median and the spread are reported.  For the vertex kernel the achieved bytes per second are set beside the
floor of a stream that only writes its output (N V 3 floats): the bytes it must also read are the N J 12 matrix floats once per
vertex tile and the [K, V] index and weight tables, which stay in cache across frames.  A number, not a tuning target."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--joints", type=int, default=160)
    ap.add_argument("--verts", type=int, default=8192)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--frames", type=int, default=4800)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    import skinning_restatement as R
    from audio2photoreal_amd import _lib, skinning as S

    J, V, K, N = args.joints, args.verts, args.k, args.frames
    skel = R.make_skeleton(1, J, V, K)
    poses, scales = R.make_inputs(2, N)
    sk = S.BodySkeleton.from_arrays(skel["parents"], skel["pre_rotation"], skel["joint_offset"], skel["transform"], skel["transform_offsets"],
                                    104, 12, skel["rest_vertices"], skel["skin_indices"], skel["skin_weights"], lbs_scale=scales[0])
    dev = torch.device("cuda:0")
    tp = torch.from_numpy(poses).to(dev)
    t = sk._tables(dev)
    states = torch.empty(N, J, 8, device=dev)
    mats = torch.empty(N, J, 3, 4, device=dev)
    out = torch.empty(N, V, 3, device=dev)
    lib, p, stream = _lib.load(), _lib.ptr, _lib.current_stream(dev)

    def run_states():
        _lib.check(lib.a2p_skin_states(p(tp), p(t["lbs_scale"]), 0, N, 104, 12, J, p(t["row_ptr"]), p(t["cols"]), p(t["vals"]), p(t["offsets"]),
                                       p(t["joint_offset"]), p(t["pre_rotation"]), p(t["parents"]), p(t["order"]), p(t["level_start"]),
                                       sk.level_start.size - 1, p(t["inv_bind"]), p(states), p(mats), stream), "a2p_skin_states")

    def run_vertices():
        _lib.check(lib.a2p_skin_vertices(p(mats), N, J, p(t["base"]), None, 0, p(t["idx"]), p(t["w"]), V, K, 1.0, 1.0, 1.0, p(out), stream),
                   "a2p_skin_vertices")

    rs, rv = timed(run_states, args.reps, args.warmup), timed(run_vertices, args.reps, args.warmup)
    assert torch.equal(states, sk.joint_states(tp)) and torch.equal(out, sk.pose_vertices(tp))      # the public calls run the same launches
    assert bool(torch.isfinite(out).all())
    tiles = (V + 1023) // 1024
    out_bytes = N * V * 3 * 4
    moved = out_bytes + N * tiles * J * 12 * 4 + N * V * K * 8 + N * V * 3 * 4      # + matrices per tile, tables and base vertices per frame (cache hits)
    sec = rv["median_ms"] * 1e-3
    res = {"workload": {"J": J, "V": V, "K": K, "N": N, "levels": int(sk.level_start.size - 1), "skeleton": "synthetic (tests/skinning_restatement.make_skeleton seed 1)",
                        "frames": "8 samples x 600 frames" if N == 4800 else f"{N} frames"},
           "device": torch.cuda.get_device_name(0), "method": f"device events around one launch, median of {args.reps} after {args.warmup} warm-up launches",
           "a2p_skin_states": {**rs, "output_bytes": N * J * 20 * 4, "frames_per_second": N / (rs["median_ms"] * 1e-3)},
           "a2p_skin_vertices": {**rv, "output_bytes": out_bytes, "output_floor_bytes_per_s_achieved": out_bytes / sec,
                                 "bytes_requested_incl_cached_reads": moved, "requested_bytes_per_s": moved / sec,
                                 "frames_per_second": N / sec,
                                 "note": "floor = the output stream alone; compare output_floor_bytes_per_s_achieved with the HBM bandwidth of the device"},
           "tuned": False}
    line = json.dumps(res, indent=1)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
