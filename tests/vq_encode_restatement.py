"""float64 restatement of TemporalVertexCodec.encode (reference model/vqvae.py:499-506, 395-430, 364-379, 169-195) for the tests:
the causal dilated Conv1d encoder and the residual nearest-code search.  torch CPU only."""
import torch
import torch.nn.functional as F

DILATIONS = (1, 2, 3, 1)


def encoder(sd, poses):
    """poses [B, T, nv] -> latents float64 [B, T, e]: 7 zero rows of left padding, enc.0 (k=1), LeakyReLU(0.2), enc.{2,4,6,8}
    (k=2, dilations 1,2,3,1) with LeakyReLU between them and none after the last."""
    w = {k: v.double() for k, v in sd.items() if k.startswith("encoder.enc.")}
    x = F.pad(poses.double().permute(0, 2, 1), (7, 0))
    x = F.leaky_relu(F.conv1d(x, w["encoder.enc.0.weight"], w["encoder.enc.0.bias"]), 0.2)
    for j, (i, dl) in enumerate(zip((2, 4, 6, 8), DILATIONS)):
        x = F.conv1d(x, w[f"encoder.enc.{i}.weight"], w[f"encoder.enc.{i}.bias"], dilation=dl)
        if j < 3:
            x = F.leaky_relu(x, 0.2)
    return x.permute(0, 2, 1).contiguous()


def distances(sd, level, residual):
    """|x - embed|^2 in the reference's form |x|^2 - 2 x.embed + |embed|^2, float64: [N, categories]."""
    embed = sd[f"quantizer.layers.{level}._codebook.embed"].double()
    r = residual.double()
    return r.pow(2).sum(1, keepdim=True) - 2 * r @ embed.t() + embed.pow(2).sum(1)[None]


def quantize(sd, latents, depth):
    """latents [B, T, e] -> tokens int64 [B, T, depth] (argmin of the float64 distance, lowest index on a tie)."""
    res = latents.double().reshape(-1, latents.shape[-1])
    out = []
    for k in range(depth):
        idx = distances(sd, k, res).argmin(1)
        out.append(idx)
        res = res - sd[f"quantizer.layers.{k}._codebook.embed"].double()[idx]
    return torch.stack(out, -1).reshape(*latents.shape[:-1], depth)


def encode(sd, poses, depth):
    return quantize(sd, encoder(sd, poses), depth)
