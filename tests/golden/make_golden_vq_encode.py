"""Golden vectors for the residual-VQ encode (TemporalVertexCodec.encode), produced by the REFERENCE itself (model/vqvae.py from
/root/reference, CPU fp32) on the synthetic decode-side weights plus the synthetic encoder weights of audio2photoreal_amd.synthetic.
Build container only:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_vq_encode.py

Two input sets of B sequences x T keyframes: random normal poses, and the reference's decode of random tokens (poses whose latents
lie nearer the codebooks, where near-ties between codes are realistic).  Stored per set: the poses, the encoder's latents, the
tokens, and the float64 top-2 distance margin of every (sequence, frame, level), taken along the reference's own residual path:
how far the chosen code's float64 distance is from the nearest other code's (0 or negative means fp32 rounding decided the pick).
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import ref_import as ri  # noqa: E402
from audio2photoreal_amd.spec import TokenizerSpec  # noqa: E402
from audio2photoreal_amd.synthetic import synthetic_tokenizer_encoder_state_dict, synthetic_tokenizer_state_dict  # noqa: E402

SEED = 10
B, T = 3, 20                     # 20 keyframes: a 600-frame window


def _margins(codec, latents):
    """float64 (second-best distance - best distance) per (b, t, level) along the residual path of the fp32 tokens."""
    res = latents.double().reshape(-1, latents.shape[-1])
    out = []
    for layer in codec.quantizer.layers:
        embed = layer._codebook.embed.double()
        d = (res.pow(2).sum(1, keepdim=True) - 2 * res @ embed.t() + embed.pow(2).sum(1)[None])
        idx = layer.encode(res.float())          # the reference's own pick on this residual, in fp32
        best = d.gather(1, idx[:, None])[:, 0]
        d2 = d.clone()
        d2.scatter_(1, idx[:, None], float("inf"))
        out.append(d2.min(1).values - best)
        res = res - embed[idx]
    return torch.stack(out, -1).reshape(*latents.shape[:-1], -1)


def main():
    torch.manual_seed(SEED)
    torch.set_num_threads(8)
    ri.import_reference()
    import model.vqvae as vq
    ts = TokenizerSpec()
    sd = {**synthetic_tokenizer_state_dict(ts, SEED), **synthetic_tokenizer_encoder_state_dict(ts, SEED)}
    out = {}
    with ri.cpu_cuda(), torch.no_grad():
        t = vq.TemporalVertexCodec(n_vertices=ts.n_vertices, latent_dim=ts.latent_dim, categories=ts.categories,
                                   residual_depth=ts.residual_depth).eval()
        missing, unexpected = t.load_state_dict(sd, strict=False)
        assert not unexpected, unexpected
        assert all(k.startswith("decoder.project_mean_shape") or k.endswith(("inited", "cluster_size", "embed_avg"))
                   for k in missing), missing
        rng = np.random.default_rng(SEED + 3)
        q = torch.from_numpy(rng.integers(0, ts.categories, size=(B, T, ts.residual_depth)))
        inputs = {"randn": torch.from_numpy(rng.standard_normal((B, T, ts.n_vertices)).astype(np.float32)),
                  "decoded": t.decode(q).float().contiguous()}
        for name, poses in inputs.items():
            lat = t.encoder(poses)
            tok = t.encode(poses)
            out[f"{name}/poses"], out[f"{name}/latents"], out[f"{name}/tokens"] = poses.numpy(), lat.numpy(), tok.numpy()
            out[f"{name}/margin"] = _margins(t, lat).numpy()
            assert torch.equal(tok, t.predict(poses))
    np.savez(os.path.join(HERE, "golden_vq_encode_v1.npz"), **out)
    print({k: (v.dtype, v.shape) for k, v in out.items()}, sum(v.nbytes for v in out.values()) / 1e6, "MB")
    for name in inputs:
        m = out[f"{name}/margin"]
        print(name, "min margin", m.min(), "entries below 1e-3", int((m < 1e-3).sum()))


if __name__ == "__main__":
    main()
