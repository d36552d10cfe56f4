"""Float64 restatement of the body denoiser with audio and keyframes dropped SEPARATELY, and of the guidance modes built on it.

The reference's `FiLMTransformer.forward` draws one dropout mask for the keyframe tokens (`encode_keyframes`, model/diffusion.py:325-328)
and another for the audio tokens and the pooled hidden (:366-369), so a trained pose checkpoint has seen all four combinations; its
`ClassifierFreeSampleModel` only ever evaluates two of them.  Nothing in the reference computes the other two, so the oracle here is a
composition of pieces `oracle/a2p_oracle.py` has already pinned to the reference: `OracleDenoiser.encode_keyframes(kf, mask, drop_k)`
and `cond_tokens(ce, drop_a)` take their drops separately as they are; `forward2` below restates the twenty lines of
`OracleDenoiser.forward` around them with two drop arguments instead of one.

Write e(K, A) for the output with the keyframes kept (K) or replaced by `null_pose_embed`, and the audio kept (A) or replaced by
`null_cond_embed` / `null_cond_hidden`:

    joint   e(0,0) + s (e(K,A) - e(0,0))                                 ClassifierFreeSampleModel
    audio   e(K,0) + s (e(K,A) - e(K,0))
    dual    e(0,0) + s_k (e(K,0) - e(0,0)) + s (e(K,A) - e(K,0))
"""
import torch

from oracle.a2p_oracle import OracleDenoiser, decoder_layer, layer_norm, mish, pose_conv_tail, sinusoidal_pos_emb


def forward2(den: OracleDenoiser, x, times, cond_embed, keyframes, mask, drop_audio: float, drop_keyframes: float):
    """`OracleDenoiser.forward` of the pose model with `cond_drop_prob` split in two.  Output [B, T, C] in den.dtype."""
    assert den.data_format == "pose" and drop_audio in (0.0, 1.0) and drop_keyframes in (0.0, 1.0)
    sd, d = den.sd, den.d
    if x.dim() == 4:
        x = x.permute(0, 3, 1, 2).squeeze(-1)
    x = x.to(den.dtype)
    pose_tokens = den.encode_keyframes(keyframes, mask, drop_keyframes)
    x = x @ sd["input_projection.weight"].T + sd["input_projection.bias"]
    ct, cond_hidden = den.cond_tokens(cond_embed, drop_audio)
    emb = sinusoidal_pos_emb(times, d, den.dtype)
    t_hidden = mish(emb @ sd["time_mlp.1.weight"].T + sd["time_mlp.1.bias"])
    t = t_hidden @ sd["to_time_cond.0.weight"].T + sd["to_time_cond.0.bias"]
    t_tokens = (t_hidden @ sd["to_time_tokens.0.weight"].T + sd["to_time_tokens.0.bias"]).view(-1, 2, d)
    t = t + cond_hidden
    mem = layer_norm(torch.cat((ct, t_tokens), dim=-2), sd["norm_cond.weight"], sd["norm_cond.bias"])
    for l in range(den.L):
        x = decoder_layer(sd, f"seqTransDecoder.stack.{l}.", x, mem, t, den.H, den.freqs, pose_tokens)
    out = x @ sd["final_layer.weight"].T + sd["final_layer.bias"]
    return pose_conv_tail(sd, out.permute(0, 2, 1)).permute(0, 2, 1)


def branches(den, x, times, cond_embed, keyframes, mask, need=("ka", "k", "0")):
    """The branches a guidance mode needs: {"ka": e(K,A), "k": e(K,0), "0": e(0,0)}."""
    drops = {"ka": (0.0, 0.0), "k": (1.0, 0.0), "0": (1.0, 1.0)}
    return {n: forward2(den, x, times, cond_embed, keyframes, mask, *drops[n]) for n in need}


def guided(den, mode: str, x, times, cond_embed, keyframes, mask, s, s_k=None):
    """The guided output [B, T, C] of `mode` ("joint", "audio", "dual"); s, s_k: [B] tensors (or numbers)."""
    B = x.shape[0]
    col = lambda v: torch.as_tensor(v, dtype=den.dtype).expand(B).view(B, 1, 1) if torch.as_tensor(v).dim() == 0 \
        else torch.as_tensor(v).to(den.dtype).view(B, 1, 1)
    if mode == "joint":
        e = branches(den, x, times, cond_embed, keyframes, mask, ("ka", "0"))
        return e["0"] + col(s) * (e["ka"] - e["0"])
    if mode == "audio":
        e = branches(den, x, times, cond_embed, keyframes, mask, ("ka", "k"))
        return e["k"] + col(s) * (e["ka"] - e["k"])
    assert mode == "dual" and s_k is not None
    e = branches(den, x, times, cond_embed, keyframes, mask)
    return e["0"] + col(s_k) * (e["k"] - e["0"]) + col(s) * (e["ka"] - e["k"])


def model_fn(den, mode: str, cond_embed, keyframes, mask, s, s_k=None):
    """`model_fn(x, t)` for OracleSampler's loops."""
    return lambda x, ts: guided(den, mode, x, ts, cond_embed, keyframes, mask, s, s_k)
