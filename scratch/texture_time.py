"""Time the texture layers (audio2photoreal_amd/texture.py) against the same steps composed from torch operators.

    python scratch/texture_time.py [--out profiles/texture_timing.json] [--frames 8] [--uv-size 1024] [--n-init-ftrs 8] ...

Workload: a release-size BodyTexture (1024 -> 2048) with random weights (the released config.yml is not at hand; upscale_n_ftrs and
the pose width are assumptions and are recorded), synthetic seam tables and a 100 x 100 grid mesh; 8 frames per call.  Every launch
of ViewUNet, PoseShadow and UpscaleNet, compose_texture, forward_tex and the whole BodyTexture.forward are timed between two device
events on the current stream around a window of `--inner` back-to-back calls, after warm-up, `--reps` windows; the median window
over `--inner` is reported per call.  Beside each, the same step composed from library operators on the same GPU and the same
inputs -- F.conv2d(stride=2), F.conv_transpose2d, F.interpolate, F.pixel_shuffle, F.grid_sample and elementwise ops -- is timed
in windows that ALTERNATE with the HIP ones: that composition is the yardstick.  A window of a step that takes under 0.1 ms is
still only a few milliseconds: such ratios are indicative.  For compose_texture `floor_bytes`
is what reading its inputs once and writing its output once takes, and `copy_fraction` its bytes per second over those of a
device-to-device copy moving the same number of bytes (read plus written), measured in this process.  Numbers, not tuning targets."""
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
sys.path.insert(0, os.path.join(ROOT, "scratch"))

CONFIG = (("uv_size", 1024), ("n_init_ftrs", 8), ("upscale_n_ftrs", 8), ("pose_to_shadow_dims", 104))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed window")
    for name, default in CONFIG:
        ap.add_argument("--" + name.replace("_", "-"), type=int, default=default)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    import texture_restatement as R
    from audio2photoreal_amd import decoder as D
    from audio2photoreal_amd import surface as S
    from audio2photoreal_amd import texture as T
    from decoder_time import grid_mesh

    dev = torch.device("cuda:0")
    cfg = {name: getattr(args, name) for name, _ in CONFIG}
    N, U, Fh = args.frames, cfg["uv_size"], cfg["n_init_ftrs"]
    rs = np.random.RandomState(1)
    sd = {"decoder_view.unet." + k: v for k, v in R.unet_params(dict(in_channels=4, out_channels=3, size=U, n_init_ftrs=Fh), 2).items()}
    up_p = {}
    R.random_layer(rs, up_p, "conv_block.0", (cfg["upscale_n_ftrs"], 6, 3, 3), (cfg["upscale_n_ftrs"], U, U))
    R.random_layer(rs, up_p, "out_block", (12, cfg["upscale_n_ftrs"], 1, 1), (12, U, U))
    sd.update({"upscale_net." + k: v for k, v in up_p.items()})
    sd.update({"pose_to_shadow." + k: v for k, v in R.shadow_params(dict(n_pose_dims=cfg["pose_to_shadow_dims"]), 3).items()})
    assets = {"seam_data_1024": R.random_seams(rs, U, U, pairs=20000, chains=1000), "seam_data_2048": R.random_seams(rs, 2 * U, 2 * U, pairs=40000, chains=2000),
              "tex_mean": (100 + 40 * rs.rand(3, 256, 256)).astype(np.float32), "tex_var": np.float32(64.0)}
    vi, vt = grid_mesh(100, 100)
    surface = S.BodySurface.from_arrays(vi, vt, vi, uv_size=U)
    tex = T.BodyTexture.from_state_dict(sd, assets, surface, **cfg)
    rows = []

    def window(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.inner):
            fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / args.inner

    def timed_pair(hip, ref):
        """Per-call ms of hip and ref: `reps` windows of `inner` calls each, the two alternating."""
        for _ in range(args.warmup):
            hip(), ref()
        torch.cuda.synchronize()
        ms = ([], [])
        for _ in range(args.reps):
            ms[0].append(window(hip))
            ms[1].append(window(ref))
        stat = lambda v: {"median_ms": sorted(v)[len(v) // 2], "min_ms": min(v), "max_ms": max(v)}
        return stat(ms[0]), stat(ms[1])

    def row(name, shape, hip, ref, **extra):
        h, r = timed_pair(hip, ref)
        e = {"step": name, "shape": shape, "hip_ms": h["median_ms"], "hip_min_max_ms": [h["min_ms"], h["max_ms"]], "torch_ms": r["median_ms"],
             "torch_min_max_ms": [r["min_ms"], r["max_ms"]], "faster": "hip" if h["median_ms"] < r["median_ms"] else "torch",
             "torch_over_hip": r["median_ms"] / h["median_ms"], **{k: v(h["median_ms"]) if callable(v) else v for k, v in extra.items()}}
        rows.append(e)
        print(json.dumps(e), flush=True)
        return e

    lrelu = lambda v: F.leaky_relu(v, 0.2)
    with torch.cuda.device(dev):
        geom = torch.from_numpy(np.concatenate([vt * 2 - 1, 0.1 * rs.randn(len(vt), 1).astype(np.float32)], 1)[None].repeat(N, 0)).to(dev).contiguous()
        geom = geom + 0.01 * torch.randn_like(geom)
        cam = torch.tensor([[0.0, 0.0, 3.0]], device=dev)
        mean_rec = torch.randn(N, 3, U, U, device=dev)
        motion = torch.randn(N, cfg["pose_to_shadow_dims"], device=dev)

        # ---- ViewUNet, launch by launch
        net, t = tex.view_net, tex.view_net._tables(dev)
        cond = torch.cat([surface.to_uv(surface.view_cos(geom, cam)[..., None]), mean_rec], 1)
        xs = [cond]
        for i in range(1, 6):
            x, w, b = xs[-1], t[f"down{i}.0.weight"], t[f"down{i}.0.bias"]
            row(f"unet.down{i}", f"{w.shape[1]}->{w.shape[0]} {x.shape[-1]}->{x.shape[-1] // 2}", lambda: T.conv2d_down_ub(x, w, b, slope=0.2),
                lambda: lrelu(F.conv2d(x, w, None, 2, 1) + b[None]))
            xs.append(T.conv2d_down_ub(x, w, b, slope=0.2))
        h = xs[5]
        for i in range(1, 6):
            x, w, b, skip = h, t[f"up{i}.0.weight"], t[f"up{i}.0.bias"], xs[5 - i] if i < 5 else None
            row(f"unet.up{i}", f"{w.shape[0]}->{w.shape[1]} {x.shape[-1]}->{2 * x.shape[-1]}" + (" +skip" if i < 5 else ""),
                lambda: T.conv_transpose2d_ub(x, w, b, slope=0.2, skip=skip),
                lambda: (lrelu(F.conv_transpose2d(x, w, None, 2, 1) + b[None]) + skip) if skip is not None else lrelu(F.conv_transpose2d(x, w, None, 2, 1) + b[None]))
            h = T.conv_transpose2d_ub(x, w, b, slope=0.2, skip=skip)
        w_cat = torch.cat([t["out.weight_x"], t["out.weight_x1"][:, :, None, None]], 1)
        row("unet.out", f"{Fh}+4->3 k1 {U}^2", lambda: D.conv2d_ub(h, t["out.weight_x"], t["out.bias"], skip_src=cond, skip_weight=t["out.weight_x1"]),
            lambda: F.conv2d(torch.cat([h, cond], 1), w_cat) + t["out.bias"][None])

        def ref_unet(x1):
            v, keep = x1, [x1]
            for i in range(1, 6):
                v = lrelu(F.conv2d(v, t[f"down{i}.0.weight"], None, 2, 1) + t[f"down{i}.0.bias"][None])
                keep.append(v)
            for i in range(1, 6):
                v = lrelu(F.conv_transpose2d(v, t[f"up{i}.0.weight"], None, 2, 1) + t[f"up{i}.0.bias"][None])
                v = v + keep[5 - i] if i < 5 else v
            return F.conv2d(torch.cat([v, x1], 1), w_cat) + t["out.bias"][None]

        row("unet", f"{N} frames", lambda: net(cond), lambda: ref_unet(cond))
        view_rec = net(cond)
        agree = {"unet": float((view_rec - ref_unet(cond)).abs().max() / view_rec.abs().max())}

        # ---- PoseShadow
        ps, p = tex.pose_shadow, tex.pose_shadow._tables(dev)
        x = lrelu(F.linear(motion, p["fc_block.0.weight"][:, :, 0, 0], p["fc_block.0.bias"])).reshape(N, 256, 4, 4)
        for i, cin, cout, s in ps.LAYERS:
            xi, w, b, last = x, p[f"conv_block.{i}.weight"], p[f"conv_block.{i}.bias"], i == 8
            hip = lambda: T.conv_transpose2d_ub(xi, w, b, slope=None if last else 0.2, sigmoid_beta=1.0 if last else None)
            row(f"shadow.conv_block.{i}", f"{cin}->{cout} {s // 2}->{s}", hip,
                lambda: torch.sigmoid(F.conv_transpose2d(xi, w, None, 2, 1) + b[None] + 1.0) if last else lrelu(F.conv_transpose2d(xi, w, None, 2, 1) + b[None]))
            x = hip()
        low = x
        row("shadow.resize", f"128->{2 * U}", lambda: T.resize_bilinear(low, (2 * U, 2 * U)),
            lambda: F.interpolate(low, (2 * U, 2 * U), mode="bilinear", align_corners=False))

        def ref_shadow(m):
            v = lrelu(F.linear(m, p["fc_block.0.weight"][:, :, 0, 0], p["fc_block.0.bias"])).reshape(-1, 256, 4, 4)
            for i, _, _, _ in ps.LAYERS:
                v = F.conv_transpose2d(v, p[f"conv_block.{i}.weight"], None, 2, 1) + p[f"conv_block.{i}.bias"][None]
                v = torch.sigmoid(v + 1.0) if i == 8 else lrelu(v)
            return F.interpolate(v, (2 * U, 2 * U), mode="bilinear", align_corners=False)

        row("shadow", f"{N} frames", lambda: ps(motion), lambda: ref_shadow(motion))
        shadow = ps(motion)
        agree["shadow"] = float((shadow - ref_shadow(motion)).abs().max() / shadow.abs().max())

        # ---- UpscaleNet and compose
        un, q = tex.upscale_net, tex.upscale_net._tables(dev)
        x6 = torch.cat([mean_rec, view_rec], 1)
        row("upscale.conv_block", f"6->{un.n_ftrs} k3 {U}^2", lambda: D.conv2d_ub(x6, q["conv_block.0.weight"], q["conv_block.0.bias"], slope=0.2),
            lambda: lrelu(F.conv2d(x6, q["conv_block.0.weight"], None, 1, 1) + q["conv_block.0.bias"][None]))
        h6 = D.conv2d_ub(x6, q["conv_block.0.weight"], q["conv_block.0.bias"], slope=0.2)
        row("upscale.out_block", f"{un.n_ftrs}->12 k1 {U}^2", lambda: D.conv2d_ub(h6, q["out_block.weight"], q["out_block.bias"]),
            lambda: F.conv2d(h6, q["out_block.weight"]) + q["out_block.bias"][None])
        u = un(x6)
        tsum = tex.seam_sampler.resample(tex.seam_sampler.impaint(mean_rec + view_rec))
        tm = tex._tex_mean(dev)
        ref_compose = lambda: ((F.interpolate(tsum, (2 * U, 2 * U), mode="bilinear", align_corners=False) + F.pixel_shuffle(u, 2)) * tex.tex_std + tm[None]) * shadow
        floor = 4 * (tsum.numel() + u.numel() + tm.numel() + shadow.numel() + N * 3 * 4 * U * U)
        src = torch.empty(floor // 8, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        copy, _ = timed_pair(lambda: dst.copy_(src), lambda: None)
        copy_gbps = floor / (copy["median_ms"] * 1e-3) / 1e9
        row("compose_texture", f"{N} x 3 x {2 * U}^2", lambda: T.compose_texture(tsum, u, tm, tex.tex_std, shadow), ref_compose, floor_bytes=floor,
            floor_GBps=lambda ms: floor / (ms * 1e-3) / 1e9, copy_GBps=copy_gbps, copy_ms=copy["median_ms"], copy_fraction=lambda ms: copy["median_ms"] / ms)
        agree["compose"] = float((T.compose_texture(tsum, u, tm, tex.tex_std, shadow) - ref_compose()).abs().max() / ref_compose().abs().max())
        del src, dst

        # ---- forward_tex and the whole forward
        def ref_seam(seam, v, resamples):
            st = seam._tables(dev)
            flat = v.reshape(v.shape[0], v.shape[1], -1)
            flat[:, :, st["dst"].long()] = flat[:, :, st["src"].long()]
            grid = (2.0 * (st["uvs"] - 0.5))[None].expand(v.shape[0], -1, -1, -1)
            for _ in range(resamples):
                v = (1.0 - st["weights"]) * v + st["weights"] * F.grid_sample(v, grid, align_corners=False, padding_mode="border")
            return v

        def ref_forward_tex(a, b, sh):
            x = torch.cat([a, b], 1)
            tr = F.interpolate(ref_seam(tex.seam_sampler, a + b, 1), (2 * U, 2 * U), mode="bilinear", align_corners=False)
            uu = F.conv2d(lrelu(F.conv2d(x, q["conv_block.0.weight"], None, 1, 1) + q["conv_block.0.bias"][None]), q["out_block.weight"]) + q["out_block.bias"][None]
            tr = (tr + F.pixel_shuffle(uu, 2)) * tex.tex_std + tm[None]
            return ref_seam(tex.seam_sampler_2k, tr * ref_seam(tex.seam_sampler_2k, sh.clone(), 2), 2)

        row("forward_tex", f"{N} frames", lambda: tex.forward_tex(mean_rec, view_rec, shadow), lambda: ref_forward_tex(mean_rec, view_rec, shadow))

        def ref_forward():
            c = torch.cat([surface.to_uv(surface.view_cos(geom, cam)[..., None]), mean_rec], 1)
            return ref_forward_tex(mean_rec, ref_unet(c), ref_shadow(motion))

        row("forward", f"{N} frames", lambda: tex.forward(geom, mean_rec, cam, motion=motion), ref_forward)
        got, want = tex.forward(geom, mean_rec, cam, motion=motion)["tex_rec"], ref_forward()
        agree["tex_rec"] = float((got - want).abs().max() / want.abs().max())

    res = {"workload": {**cfg, "frames": N, "configuration_source": "upscale_n_ftrs and pose_to_shadow_dims assumed; random weights"},
           "device": torch.cuda.get_device_name(0),
           "method": f"device events around windows of {args.inner} back-to-back calls (allocation of the outputs included), per-call median of {args.reps} windows after "
                     f"{args.warmup} warm-up calls, HIP and torch windows alternating; "
                     "torch = the same step from F.conv2d(stride=2) / F.conv_transpose2d / F.interpolate / F.pixel_shuffle / F.grid_sample / elementwise ops",
           "hip_vs_torch_normalised_difference": agree, "activation_bytes_per_frame": tex.activation_bytes_per_frame(), "steps": rows, "tuned": False}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    print("forward:", rows[-1], agree)


if __name__ == "__main__":
    main()
