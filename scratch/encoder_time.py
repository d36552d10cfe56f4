"""Time the encode path (audio2photoreal_amd/encoder.py, BodySkeleton.unpose_vertices) against the same steps composed from torch
operators.

    python scratch/encoder_time.py [--out profiles/encoder_timing.json] [--frames 8]

Workload: release-size FaceDecoder (256 codes -> 7306 vertices and a 1024 x 1024 texture), FaceEncoder and BodyEncoder (512 x 512,
seven blocks) with random weights, a 100 x 100 grid mesh at uv 1024 and a random 160-joint skeleton over its vertices; 8 frames
per call.  Method of scratch/texture_time.py: every launch and every whole network is timed between two device events on the
current stream around a window of `--inner` back-to-back calls (allocation of the outputs included), after warm-up, `--reps`
windows, the median reported per call; the same step composed from F.linear / F.conv2d / F.conv_transpose2d / F.interpolate on
the same inputs is timed in windows that ALTERNATE with the HIP ones.  For the two 22 MB linear layers `weight_GBps` is the
weight bytes over the call's time and `copy_fraction` that rate over the rate of a device-to-device copy of the same byte count
(bytes read; the copy also writes them), measured in this process.  Numbers, not tuning targets."""
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

FACE_DEC = dict(n_latent=256, n_hidden=256, V=7306, n_view=8, s0=4,
                ladder=((256, 256), (256, 128), (128, 128), (128, 64), (64, 64), (64, 32), (32, 8), (8, 3)))
FACE_ENC = dict(uv_size=512, ladder=((3, 4), (4, 8), (8, 16), (16, 32), (32, 64), (64, 128), (128, 128)), n_geom=256, n_joint=512, n_embs=256)
BODY_ENC = dict(uv_size=512, ladder=((3, 8), (8, 16), (16, 32), (32, 32), (32, 64), (64, 128), (128, 128)), n_embs=1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed window")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "timing needs the MI355X"
    import encoder_restatement as R
    import skinning_restatement as SR
    from audio2photoreal_amd import decoder as D
    from audio2photoreal_amd import encoder as E
    from audio2photoreal_amd import skinning as SK
    from audio2photoreal_amd import surface as S
    from audio2photoreal_amd import texture as T
    from decoder_time import grid_mesh

    dev = torch.device("cuda:0")
    N = args.frames
    rs = np.random.RandomState(1)
    yy, xx = np.mgrid[0:1024, 0:1024]
    assets = {"face_frontal_view": rs.randn(3).astype(np.float32),
              "mugsy_face_mask": np.repeat(np.clip(1.5 - np.hypot(yy - 511.5, xx - 511.5) / 300.0, 0, 1)[:, :, None], 3, 2).astype(np.float32),
              "face_mask": (np.hypot(yy - 200, xx - 800) < 150).astype(np.float32)}
    vi, vt = grid_mesh(100, 100)
    surface = S.BodySurface.from_arrays(vi, vt, vi, uv_size=1024)
    prefixed = lambda p, prefix: {prefix + k: v for k, v in p.items()}
    fdec = E.FaceDecoder.from_state_dict(prefixed(R.face_decoder_params(FACE_DEC, 2), "decoder_face."), assets)
    fenc = E.FaceEncoder.from_state_dict(prefixed(R.face_encoder_params(FACE_ENC, 3 * FACE_DEC["V"], 3), "encoder_face."), assets)
    benc = E.BodyEncoder.from_state_dict(prefixed(R.body_encoder_params(BODY_ENC, 4), "encoder."), assets, surface)
    skel = SR.make_skeleton(5, 160, surface.V, 8, P_pos=104, P_scale=29)
    template = np.concatenate([vt * 2 - 1, 0.1 * rs.randn(len(vt), 1).astype(np.float32)], 1).astype(np.float32)
    sk = SK.BodySkeleton.from_arrays(skel["parents"], skel["pre_rotation"], skel["joint_offset"], skel["transform"], skel["transform_offsets"], 104, 29,
                                     skel["rest_vertices"], skel["skin_indices"], skel["skin_weights"], template_verts=template,
                                     lbs_scale=np.zeros(29, np.float32), global_scaling=np.float32(10.0))
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

    def copy_rate(n_bytes):
        src = torch.empty(n_bytes // 4, dtype=torch.float32, device=dev).normal_()
        dst = torch.empty_like(src)
        c, _ = timed_pair(lambda: dst.copy_(src), lambda: None)
        return c["median_ms"]

    lrelu = lambda v: F.leaky_relu(v, 0.2)
    nerr = lambda a, b: float((a - b).abs().max() / b.abs().max())
    agree = {}
    with torch.cuda.device(dev):
        codes = torch.randn(N, 256, device=dev)
        t = fdec._tables(dev)

        def lin_row(name, x, w, b, slope, big=False):
            extra = {}
            if big:
                n_bytes = 4 * w.numel()
                copy_ms = copy_rate(n_bytes)
                extra = dict(weight_bytes=n_bytes, weight_GBps=lambda ms: n_bytes / (ms * 1e-3) / 1e9, copy_ms=copy_ms,
                             copy_GBps=n_bytes / (copy_ms * 1e-3) / 1e9, copy_fraction=lambda ms: copy_ms / ms)
            act = lrelu if slope is not None else (lambda v: v)
            row(name, f"{w.shape[1]}->{w.shape[0]}, {x.shape[0]} rows", lambda: E.linear(x, w, b, slope=slope), lambda: act(F.linear(x, w, b)), **extra)
            return E.linear(x, w, b, slope=slope)

        # ---- FaceDecoder, launch by launch
        enc = lin_row("face_decoder.encmod", codes, t["encmod.0.weight"], t["encmod.0.bias"], 0.2)
        lin_row("face_decoder.geommod", enc, t["geommod.0.weight"], t["geommod.0.bias"], None, big=True)
        encview = torch.cat([enc, t["viewout"].expand(N, -1)], 1)
        y = lin_row("face_decoder.texmod2", encview, t["texmod2.0.weight"], t["texmod2.0.bias"], 0.2).reshape(N, 256, 4, 4)
        for i, (name, cin, cout, s) in enumerate(fdec.layers):
            xi, w, b, last = y, t[f"{name}.weight"], t[f"{name}.bias"], i + 1 == len(fdec.layers)
            hip = lambda: T.conv_transpose2d_ub(xi, w, b, slope=None if last else 0.2)
            row(f"face_decoder.{name}", f"{cin}->{cout} {s}->{2 * s}", hip,
                lambda: (F.conv_transpose2d(xi, w, None, 2, 1) + b[None]) if last else lrelu(F.conv_transpose2d(xi, w, None, 2, 1) + b[None]))
            y = hip()

        def ref_face_decoder(c):
            e = lrelu(F.linear(c, t["encmod.0.weight"], t["encmod.0.bias"]))
            g = F.linear(e, t["geommod.0.weight"], t["geommod.0.bias"])
            view = lrelu(F.linear(t["frontal_view"].expand(c.shape[0], -1), t["viewmod.0.weight"], t["viewmod.0.bias"]))
            v = lrelu(F.linear(torch.cat([e, view], 1), t["texmod2.0.weight"], t["texmod2.0.bias"])).reshape(-1, 256, 4, 4)
            for i, (name, _, _, _) in enumerate(fdec.layers):
                v = F.conv_transpose2d(v, t[f"{name}.weight"], None, 2, 1) + t[f"{name}.bias"][None]
                v = v if i + 1 == len(fdec.layers) else lrelu(v)
            return g.reshape(c.shape[0], -1, 3), v

        row("face_decoder", f"{N} frames", lambda: fdec(codes), lambda: ref_face_decoder(codes))
        face = fdec(codes)
        g_ref, raw_ref = ref_face_decoder(codes)
        agree["face_geom"], agree["face_tex_raw"] = nerr(face["face_geom"], g_ref), nerr(face["face_tex_raw"], raw_ref)

        # ---- FaceEncoder
        q, bias = fenc._tables(dev), fdec.bias(dev)
        raw, geom = face["face_tex_raw"], face["face_geom"].reshape(N, -1)
        ref_cond = lambda: (F.interpolate(255 * (raw + bias[None] + 0.5), (512, 512), mode="bilinear", align_corners=False) / 255.0 - 0.5) * q["tex_cond_mask"]
        row("face_encoder.tex_cond", f"{N} x 3 x 1024^2 -> 512^2", lambda: E.face_tex_cond(raw, bias, q["tex_cond_mask"]), ref_cond)

        def ref_block(p, name, x):
            c_out, c_in = p[f"{name}.conv_resize.weight"].shape
            skip = F.conv2d(x, p[f"{name}.conv_resize.weight"].reshape(c_out, c_in, 1, 1), p[f"{name}.conv_resize.bias"], stride=2)
            h = lrelu(F.conv2d(x, p[f"{name}.conv1.weight"], None, 1, 1) + p[f"{name}.conv1.bias"][None])
            return lrelu(F.conv2d(h, p[f"{name}.conv2.weight"], None, 2, 1) + p[f"{name}.conv2.bias"][None]) + skip

        def block_rows(prefix, p, blocks, x):
            for name, cin, cout, s in blocks:
                xi = x
                h = D.conv2d_ub(xi, p[f"{name}.conv1.weight"], p[f"{name}.conv1.bias"], slope=0.2)
                row(f"{prefix}.{name}.down3", f"{cin}->{cout} {s}->{s // 2}",
                    lambda: E.conv2d_down3_ub(h, xi, p[f"{name}.conv2.weight"], p[f"{name}.conv2.bias"], p[f"{name}.conv_resize.weight"], p[f"{name}.conv_resize.bias"]),
                    lambda: lrelu(F.conv2d(h, p[f"{name}.conv2.weight"], None, 2, 1) + p[f"{name}.conv2.bias"][None])
                    + F.conv2d(xi, p[f"{name}.conv_resize.weight"].reshape(cout, cin, 1, 1), p[f"{name}.conv_resize.bias"], stride=2))
                row(f"{prefix}.{name}", f"{cin}->{cout} {s}->{s // 2} (both launches)", lambda: E.conv_down_block(xi, p, name), lambda: ref_block(p, name, xi))
                x = E.conv_down_block(xi, p, name)
            return x

        x = block_rows("face_encoder", q, fenc.blocks, E.face_tex_cond(raw, bias, q["tex_cond_mask"]))
        genc = lin_row("face_encoder.geommod", geom, q["geommod.0.weight"], q["geommod.0.bias"], 0.2, big=True)
        joint = torch.cat([x.reshape(N, -1), genc], 1)
        j = lin_row("face_encoder.jointmod", joint, q["jointmod.0.weight"], q["jointmod.0.bias"], 0.2)
        lin_row("face_encoder.mu", j, q["mu.weight"], q["mu.bias"], None)

        def ref_face_encoder():
            v = ref_cond()
            for name, _, _, _ in fenc.blocks:
                v = ref_block(q, name, v)
            ge = lrelu(F.linear(geom, q["geommod.0.weight"], q["geommod.0.bias"]))
            jj = lrelu(F.linear(torch.cat([v.reshape(N, -1), ge], 1), q["jointmod.0.weight"], q["jointmod.0.bias"]))
            return F.linear(jj, q["mu.weight"], q["mu.bias"]), 0.1 * F.linear(jj, q["logvar.weight"], q["logvar.bias"])

        row("face_encoder", f"{N} frames", lambda: fenc(face["face_geom"], raw, bias), ref_face_encoder)
        agree["face_embs"] = nerr(fenc(face["face_geom"], raw, bias)["face_embs"], ref_face_encoder()[0])

        # ---- unpose and BodyEncoder
        poses = 0.3 * torch.randn(N, 104, device=dev)
        posed = sk.pose_vertices(poses, verts_unposed=0.02 * torch.randn(N, sk.V, 3, device=dev))
        mats, tb = sk.transforms(poses), sk._tables(dev)
        idx, w = tb["idx"].long().T, tb["w"].T                                # [V, K]

        def ref_unpose():
            m = (mats[:, idx] * w[None, :, :, None, None]).sum(2)               # [N, V, 3, 4]
            m4 = torch.cat([m, torch.tensor([0.0, 0, 0, 1], device=dev).expand(N, sk.V, 1, 4)], 2)
            v4 = torch.cat([posed / 10.0, torch.ones(N, sk.V, 1, device=dev)], 2)[..., None]
            return torch.linalg.inv(m4).matmul(v4)[..., :3, 0] - tb["base"]

        row("unpose_vertices", f"{N} x {sk.V} vertices, {sk.J} joints, K = {sk.K} (state solve included; torch: blend and inverse only)",
            lambda: sk.unpose_vertices(poses, posed), ref_unpose)
        unposed = sk.unpose_vertices(poses, posed)
        agree["unpose"] = nerr(unposed, ref_unpose())
        b = benc._tables(dev)
        uv = surface.to_uv(unposed)
        cond = T.resize_bilinear(uv, (512, 512)) * b["mask"]
        block_rows("body_encoder", b, benc.blocks, cond)

        def ref_body_encoder():
            v = F.interpolate(uv, (512, 512), mode="bilinear", align_corners=False) * b["mask"]
            for name, _, _, _ in benc.blocks:
                v = ref_block(b, name, v)
            v = v.reshape(N, -1)
            return F.linear(v, b["mu.weight"], b["mu.bias"]), 0.1 * F.linear(v, b["logvar.weight"], b["logvar.bias"])

        row("body_encoder", f"{N} frames (to_uv included; torch: from the UV map)", lambda: benc(unposed), ref_body_encoder)
        agree["embs"] = nerr(benc(unposed)["embs"], ref_body_encoder()[0])
        face_codes = torch.randn(N, 256, device=dev)
        row("encode_motion", f"{N} frames", lambda: E.encode_motion(fdec, fenc, benc, sk, poses, face_codes),
            lambda: (ref_face_decoder(face_codes), ref_face_encoder(), ref_unpose(), ref_body_encoder()))

    res = {"workload": {"frames": N, "face_decoder": FACE_DEC, "face_encoder": FACE_ENC, "body_encoder": BODY_ENC, "mesh": "100 x 100 grid at uv 1024",
                        "skeleton": "160 random joints, K = 8", "configuration_source": "the reference's constructors; random weights"},
           "device": torch.cuda.get_device_name(0),
           "method": f"device events around windows of {args.inner} back-to-back calls (allocation of the outputs included), per-call median of {args.reps} windows after "
                     f"{args.warmup} warm-up calls, HIP and torch windows alternating; torch = the same step from F.linear / F.conv2d / F.conv_transpose2d / "
                     "F.interpolate / torch.linalg.inv / elementwise ops",
           "hip_vs_torch_normalised_difference": agree,
           "activation_bytes_per_frame": E.activation_bytes_per_frame(fdec, fenc, benc, sk), "steps": rows, "tuned": False}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(res, indent=1) + "\n")
    print("encode_motion:", rows[-1], agree)


if __name__ == "__main__":
    main()
