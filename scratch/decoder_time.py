"""Time the decoder layers (audio2photoreal_amd/decoder.py) against the same steps composed from torch operators.

    python scratch/decoder_time.py [--out profiles/decoder_timing.json] [--frames 8] [--uv-size 1024] [--n-init-channels 64] ...

Workload: a full-size BodyDecoder with random weights (the released config.yml is not at hand; the defaults below are the
configuration as remembered, unverified, and the one used is recorded), random 0/1 masks, a synthetic seam table and a 100 x 100
grid mesh; 8 frames per call.  Every launch of every residual block, each block, the seam steps, the two heads and the whole
forward are timed between two device events on the current stream, after warm-up, `--reps` times; the median is reported.  Beside
each, the same step composed from library operators on the same GPU and the same inputs -- F.interpolate(bilinear,
align_corners=True), F.conv2d, the bias add, F.leaky_relu, the sum, F.grid_sample -- is timed the same way: that composition is
the yardstick.  For each launch `floor_bytes` is what reading its sources, weights, bias and mask once and writing its output once
takes, and `floor_GBps` that figure over the measured time; `tile_bytes` is what the kernel's tiling asks of the memory system
before any cache (the source re-read once per chunk of 8 output channels, the halo of the 8 x 32 tile included).  Traffic counters
were not collected.  Numbers, not tuning targets."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CONFIG = (("uv_size", 1024), ("init_uv_size", 64), ("n_init_channels", 64), ("n_min_channels", 4), ("n_pose_dims", 98),
          ("n_pose_enc_channels", 16), ("n_embs", 1024), ("n_embs_enc_channels", 32), ("n_face_embs", 256))


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
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1]}


def grid_mesh(nx, ny):
    vid = lambda i, j: j * nx + i
    vi = np.array([t for j in range(ny - 1) for i in range(nx - 1)
                   for t in ([vid(i, j), vid(i + 1, j), vid(i + 1, j + 1)], [vid(i, j), vid(i + 1, j + 1), vid(i, j + 1)])])
    ii, jj = np.meshgrid(np.arange(nx), np.arange(ny))
    vt = np.stack([0.02 + 0.96 * ii / (nx - 1), 0.02 + 0.96 * jj / (ny - 1)], -1).reshape(-1, 2)
    return vi, vt.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    for name, default in CONFIG:
        ap.add_argument("--" + name.replace("_", "-"), type=int, default=default)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    import decoder_restatement as R
    from audio2photoreal_amd import decoder as D
    from audio2photoreal_amd import surface as S

    dev = torch.device("cuda:0")
    cfg = {name: getattr(args, name) for name, _ in CONFIG}
    N, U, S0 = args.frames, cfg["uv_size"], 64
    rs = np.random.RandomState(1)
    params = R.random_params(cfg, 2)
    assets = {"pose_cond_mask": (rs.rand(cfg["n_pose_dims"], S0, S0) < 0.6).astype(np.float32), "head_cond_mask": (rs.rand(S0, S0) < 0.3).astype(np.float32),
              "face_cond_mask": (rs.rand(S0, S0) < 0.4).astype(np.float32), "body_cond_mask": (rs.rand(S0, S0) < 0.8).astype(np.float32),
              "seam_data_1024": R.random_seams(rs, U, U, pairs=20000, chains=1000)}
    vi, vt = grid_mesh(100, 100)
    dec = D.BodyDecoder.from_state_dict({"decoder." + k: v for k, v in params.items()}, assets, S.BodySurface.from_arrays(vi, vt, vi, uv_size=U), **cfg)
    t = dec._tables(dev)
    motion = torch.from_numpy(rs.randn(N, 6 + cfg["n_pose_dims"]).astype(np.float32)).to(dev)
    embs = torch.from_numpy(rs.randn(N, cfg["n_embs"]).astype(np.float32)).to(dev)
    face = torch.from_numpy(rs.randn(N, cfg["n_face_embs"]).astype(np.float32)).to(dev)
    T = lambda fn: timed(fn, args.reps, args.warmup)
    rows = []

    def row(name, shape, hip, ref, floor=None, tile=None):
        h, r = T(hip), T(ref)
        e = {"step": name, "shape": shape, "hip_ms": h["median_ms"], "hip_min_max_ms": [h["min_ms"], h["max_ms"]], "torch_ms": r["median_ms"],
             "torch_min_max_ms": [r["min_ms"], r["max_ms"]], "faster": "hip" if h["median_ms"] < r["median_ms"] else "torch",
             "torch_over_hip": r["median_ms"] / h["median_ms"]}
        if floor is not None:
            e.update(floor_bytes=int(floor), tile_bytes=int(tile), floor_GBps=floor / (h["median_ms"] * 1e-3) / 1e9)
        rows.append(e)
        print(json.dumps(e), flush=True)

    def t_up(x, size):
        return x if x.shape[-1] == size else F.interpolate(x, size=(size, size), mode="bilinear", align_corners=True)

    def block(spec, x, mask=None):
        """Time the two launches of a block and the block; returns its output."""
        name, cin, cout, size, k, groups = spec
        w1, b1, w2, b2 = (t[f"{name}.{p}"] for p in ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias"))
        wr, br = t[f"{name}.conv_resize.weight"], t[f"{name}.conv_resize.bias"]
        hip1 = lambda: D.conv2d_ub(x, w1, b1, groups=groups, size=(size, size), slope=0.2)
        ref1 = lambda: F.leaky_relu(F.conv2d(t_up(x, size), w1, None, 1, k // 2, 1, groups) + b1[None], 0.2)
        h = hip1()
        hip2 = lambda: D.conv2d_ub(h, w2, b2, groups=groups, slope=0.2, skip_src=x, skip_weight=wr, skip_bias=br, mask=mask)

        def ref2():
            y = F.leaky_relu(F.conv2d(h, w2, None, 1, k // 2, 1, groups) + b2[None], 0.2) + F.conv2d(t_up(x, size), wr, br, 1, 0, 1, groups)
            return y if mask is None else y * mask

        shape = f"{cin}->{cout} g{groups} k{k} {x.shape[-1]}->{size}"
        px, ph, halo = 4 * N * x[0].numel(), 4 * N * cin * size * size, (340 / 256 if k == 3 else 1.0)
        chunks = lambda c: -(-(c // groups) // (4 if c // groups <= 4 else 8))
        up = (size / x.shape[-1]) ** 2                                        # an upsampled source is asked for 4 taps per element
        row(f"{name}.launch1", shape, hip1, ref1, px + 4 * (w1.numel() + b1.numel()) + ph,
            chunks(cin) * halo * (4 * up if up > 1 else 1) * px + 4 * b1.numel() + ph)
        out_b = 4 * N * cout * size * size
        row(f"{name}.launch2", shape, hip2, ref2, ph + px + 4 * (w2.numel() + b2.numel() + wr.numel()) + out_b,
            chunks(cout) * (halo * ph + (4 * up if up > 1 else 1) * px) + 4 * b2.numel() + out_b)
        row(f"{name}", shape, lambda: (hip1(), hip2()), lambda: (ref1(), ref2()))
        return hip2()

    with torch.cuda.device(dev):
        pose_masked = motion[:, 6:, None, None] * t["pose_cond_mask"]
        pose_conv = block(dec.pose_block, pose_masked, mask=t["non_head_mask"])
        e = dec._fc(t, embs, "embs_fc.0", 128)
        for spec in dec.embs_blocks:
            e = block(spec, e)
        f = dec._fc(t, face, "face_embs_fc.0", 32)
        for spec in dec.face_blocks:
            f = block(spec, f)
        merged = e.clone()
        merged[:, :, 32:, :32] = f * t["face_quadrant"] + e[:, :, 32:, :32] * t["non_head_quadrant"]
        joint = block(dec.joint_block, torch.cat([pose_conv, merged], 1))
        x = torch.cat([joint, joint], 1)
        for spec in dec.up_blocks:
            x = block(spec, x)

        seam, st = dec.seam_sampler, dec.seam_sampler._tables(dev)
        dst, src = st["dst"].long(), st["src"].long()
        grid = (2.0 * (st["uvs"] - 0.5))[None].expand(N, -1, -1, -1)

        def ref_impaint():
            flat = x.reshape(N, x.shape[1], -1)
            flat[:, :, dst] = flat[:, :, src]

        def ref_resample(v):
            return (1.0 - st["weights"]) * v + st["weights"] * F.grid_sample(v, grid, align_corners=False, padding_mode="border")

        planes = 4 * N * x[0].numel()
        row("seam.impaint", f"{x.shape[1]} x {U}^2, {seam.P} pairs", lambda: seam.impaint(x), ref_impaint, 16 * N * x.shape[1] * seam.P, 16 * N * x.shape[1] * seam.P)
        row("seam.resample", f"{x.shape[1]} x {U}^2", lambda: seam.resample(x), lambda: ref_resample(x), 2 * planes + 12 * U * U, 6 * planes + 12 * U * U)
        x = seam.resample(seam.resample(x))
        C = dec.n_channels[-1]
        for name, sl in (("verts_conv", slice(0, C)), ("tex_conv", slice(C, 2 * C))):
            w, b = t[f"{name}.weight"], t[f"{name}.bias"]
            xs = x[:, sl]
            row(name, f"{C}->3 k3 {U}^2", lambda: D.conv2d_ub(xs, w, b), lambda: F.conv2d(xs, w, None, 1, 1) + b[None],
                planes // 2 + 4 * (w.numel() + b.numel()) + 12 * N * U * U, (340 / 256) * planes // 2 + 4 * b.numel() + 12 * N * U * U)

        def ref_block(spec, v, mask=None):
            name, _, _, size, k, groups = spec
            p = lambda s: t[f"{name}.{s}"]
            h = F.leaky_relu(F.conv2d(t_up(v, size), p("conv1.weight"), None, 1, k // 2, 1, groups) + p("conv1.bias")[None], 0.2)
            y = F.leaky_relu(F.conv2d(h, p("conv2.weight"), None, 1, k // 2, 1, groups) + p("conv2.bias")[None], 0.2)
            y = y + F.conv2d(t_up(v, size), p("conv_resize.weight"), p("conv_resize.bias"), 1, 0, 1, groups)
            return y if mask is None else y * mask

        def ref_forward():
            pc = ref_block(dec.pose_block, motion[:, 6:, None, None] * t["pose_cond_mask"], t["non_head_mask"])
            a = F.leaky_relu(F.linear(embs, t["embs_fc.0.weight"][:, :, 0, 0], t["embs_fc.0.bias"]), 0.2).reshape(N, 128, 4, 4)
            for spec in dec.embs_blocks:
                a = ref_block(spec, a)
            b = F.leaky_relu(F.linear(face, t["face_embs_fc.0.weight"][:, :, 0, 0], t["face_embs_fc.0.bias"]), 0.2).reshape(N, 32, 4, 4)
            for spec in dec.face_blocks:
                b = ref_block(spec, b)
            a[:, :, 32:, :32] = b * t["face_quadrant"] + a[:, :, 32:, :32] * t["non_head_quadrant"]
            j = ref_block(dec.joint_block, torch.cat([pc, a], 1))
            v = torch.cat([j, j], 1)
            for spec in dec.up_blocks:
                v = ref_block(spec, v)
            flat = v.reshape(N, v.shape[1], -1)
            flat[:, :, dst] = flat[:, :, src]
            v = ref_resample(ref_resample(v))
            uv = F.conv2d(v[:, :C], t["verts_conv.weight"], None, 1, 1) + t["verts_conv.bias"][None]
            tex = F.conv2d(v[:, C:], t["tex_conv.weight"], None, 1, 1) + t["tex_conv.bias"][None]
            return dec.surface.from_uv(uv), tex

        row("forward", f"{N} frames", lambda: dec.forward(motion, embs, face), ref_forward)
        got, (want_v, want_tex) = dec.forward(motion, embs, face), ref_forward()
        agree = {"tex_mean_rec": float((got["tex_mean_rec"] - want_tex).abs().max() / want_tex.abs().max()),
                 "geom_delta_rec": float((got["geom_delta_rec"] - want_v).abs().max() / want_v.abs().max())}

    res = {"workload": {**cfg, "frames": N, "configuration_source": "remembered, unverified; random weights"},
           "device": torch.cuda.get_device_name(0),
           "method": f"device events around one call (allocation of the outputs included), median of {args.reps} after {args.warmup} warm-up calls; "
                     "torch = the same step from F.interpolate / F.conv2d / adds / F.leaky_relu / F.grid_sample on the same inputs",
           "hip_vs_torch_normalised_difference": agree, "activation_bytes_per_frame": dec.activation_bytes_per_frame(), "steps": rows,
           "tuned": False}
    line = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(line + "\n")
    print("forward:", rows[-1], agree)


if __name__ == "__main__":
    main()
