"""float64 restatement of one training step of the residual-VQ tokenizer, for the tests: TemporalVertexCodec in training mode,
SmoothL1 losses, AdamW and the EMA codebook update, in two forms that share only the forward: torch autograd, and the hand-written
backward the HIP kernels implement (only level 0 of the straight-through residual VQ carries commitment gradient).  torch CPU only.

State: {"params": {name: tensor}, "exp_avg": {...}, "exp_avg_sq": {...}, "step": int, "embed": [depth x [C, e]],
"embed_avg": [...], "cluster_size": [depth x [C]]}, everything float64.  `decoder.project_mean_shape.*` is carried and never
touched (no gradient reaches it)."""
import math

import torch
import torch.nn.functional as F

DILATIONS = (1, 2, 3, 1)
BETAS, ADAM_EPS = (0.9, 0.99), 1e-8


def param_shapes(nv, e):
    """Names and shapes in the order of the codec's parameters(): the layout of the flat buffers."""
    s = [("encoder.enc.0.weight", (e, nv, 1)), ("encoder.enc.0.bias", (e,))]
    for i in (2, 4, 6, 8):
        s += [(f"encoder.enc.{i}.weight", (e, e, 2)), (f"encoder.enc.{i}.bias", (e,))]
    s += [("decoder.project_mean_shape.weight", (e, nv)), ("decoder.project_mean_shape.bias", (e,))]
    for i in (0, 2, 4, 6):
        s += [(f"decoder.dec.{i}.weight", (e, e, 2)), (f"decoder.dec.{i}.bias", (e,))]
    s += [("decoder.dec.8.weight", (nv, e, 1)), ("decoder.dec.8.bias", (nv,))]
    return s


def trainable(name):
    return "project_mean_shape" not in name


def flatten(tensors, nv, e):
    """{name: tensor} -> one flat float64 vector in parameter order; a missing entry (project_mean_shape's gradient) is zeros."""
    return torch.cat([tensors[n].double().reshape(-1) if n in tensors else torch.zeros(math.prod(sh), dtype=torch.float64)
                      for n, sh in param_shapes(nv, e)])


def unflatten(flat, nv, e):
    out, o = {}, 0
    for n, sh in param_shapes(nv, e):
        k = math.prod(sh)
        out[n] = flat[o:o + k].reshape(sh)
        o += k
    assert o == flat.numel()
    return out


def make_state(sd, depth, ema_scale=5.0, dtype=torch.float64):
    """An inited training state from a state dict: embed_avg = ema_scale * embed, cluster_size = ema_scale, zero moments.
    `dtype=torch.float32` runs the same restatement in the precision of the code under test (the yardstick of its rounding)."""
    names = [k for k in sd if k.startswith(("encoder.", "decoder."))]
    params = {k: sd[k].to(dtype).clone() for k in names}
    embed = [sd[f"quantizer.layers.{k}._codebook.embed"].to(dtype).clone() for k in range(depth)]
    return {"params": params, "exp_avg": {k: torch.zeros_like(v) for k, v in params.items() if trainable(k)},
            "exp_avg_sq": {k: torch.zeros_like(v) for k, v in params.items() if trainable(k)}, "step": 0, "embed": embed,
            "embed_avg": [ema_scale * b for b in embed],
            "cluster_size": [torch.full((b.shape[0],), ema_scale, dtype=dtype) for b in embed]}


def _dtype(state):
    return state["embed"][0].dtype


def smooth_l1(d):
    a = d.abs()
    return torch.where(a < 1, 0.5 * d * d, a - 0.5)


def smooth_l1_grad(d):
    return torch.where(d.abs() < 1, d, torch.sign(d))


def pick(embed, res):
    """Nearest code per row in the reference's form |x|^2 - 2 x.e + |e|^2; lowest index on a tie.  Also the top-2 relative margin."""
    d = res.pow(2).sum(1, keepdim=True) - 2 * res @ embed.t() + embed.pow(2).sum(1)[None]
    idx = d.argmin(1)
    if d.shape[1] > 1:
        two = d.topk(2, dim=1, largest=False).values
        margin = (two[:, 1] - two[:, 0]) / two[:, 1].abs().clamp_min(1e-300)
    else:
        margin = torch.full((d.shape[0],), float("inf"), dtype=d.dtype)
    return idx, margin


def encoder_acts(P, x):
    """x [B, T, nv] -> the inputs of the five encoder convs (channels first, padded) and the latents z [B, e, T]."""
    h = F.pad(x.permute(0, 2, 1), (7, 0))
    ins, pre = [], []
    for j, i in enumerate((0, 2, 4, 6, 8)):
        ins.append(h)
        h = F.conv1d(h, P[f"encoder.enc.{i}.weight"], P[f"encoder.enc.{i}.bias"], dilation=1 if j == 0 else DILATIONS[j - 1])
        pre.append(h)
        if j < 4:
            h = F.leaky_relu(h, 0.2)
    return ins, pre, h


def decoder_acts(P, q):
    """q [B, e, T] (quantised latents) -> inputs and pre-activations of the five decoder convs, and pred [B, T, nv]."""
    h = F.pad(q, (7, 0))
    ins, pre = [], []
    for j, i in enumerate((0, 2, 4, 6, 8)):
        ins.append(h)
        h = F.conv1d(h, P[f"decoder.dec.{i}.weight"], P[f"decoder.dec.{i}.bias"], dilation=DILATIONS[j] if j < 4 else 1)
        pre.append(h)
        if j < 4:
            h = F.leaky_relu(h, 0.2)
    return ins, pre, h.permute(0, 2, 1)


def quantise(embeds, z_rows):
    """Residual quantisation of rows [N, e] with fixed books: tokens [N, depth], per-level residuals, codes and margins."""
    res, toks, residuals, codes, margins = z_rows, [], [], [], []
    for embed in embeds:
        idx, m = pick(embed, res)
        q = embed[idx]
        toks.append(idx), residuals.append(res), codes.append(q), margins.append(m)
        res = res - q
    return torch.stack(toks, -1), residuals, codes, torch.stack(margins, -1)


def losses(pred, x, commit_levels, hp):
    motion = smooth_l1(pred - x).mean()
    vel = smooth_l1((pred[..., :-1] - pred[..., 1:]) - (x[..., :-1] - x[..., 1:])).mean() if hp["loss_vel"] > 0 else pred.new_zeros(())
    commit = torch.stack(commit_levels).mean()
    return {"loss": motion + hp["commit"] * commit + hp["loss_vel"] * vel, "loss_motion": motion, "loss_commit": commit, "loss_vel": vel}


def perplexity(tokens_last, categories):
    prob = torch.bincount(tokens_last.reshape(-1), minlength=categories).double() / tokens_last.numel()   # float64 in either mode
    return torch.exp(-(prob * torch.log(prob + 1e-7)).sum())


def _forward_autograd(P, embeds, x, hp):
    B, T, _ = x.shape
    e = embeds[0].shape[1]
    _, enc_pre, z = encoder_acts(P, x)
    rows = z.permute(0, 2, 1).reshape(B * T, e)
    tokens, residuals, codes, margins = quantise(embeds, rows.detach())
    # the straight-through chain as the model builds it: quantized = x + (q - x).detach(); residual = residual - quantized
    res, total, commit_levels = rows, 0.0, []
    for q in codes:
        st = res + (q - res).detach()
        commit_levels.append(((st.detach() - res) ** 2).mean())
        res = res - st
        total = total + st
    _, dec_pre, pred = decoder_acts(P, total.reshape(B, T, e).permute(0, 2, 1))
    out = losses(pred, x, commit_levels, hp)
    out.update(tokens=tokens.reshape(B, T, -1), residuals=residuals, margins=margins, pred=pred,
               preacts=[t for t in enc_pre[:4] + dec_pre[:4]])
    return out


def gradients_autograd(state, x, hp):
    P = {k: v.clone().requires_grad_(trainable(k)) for k, v in state["params"].items()}
    out = _forward_autograd(P, state["embed"], x.to(_dtype(state)), hp)
    names = [k for k in P if trainable(k)]
    grads = dict(zip(names, torch.autograd.grad(out["loss"], [P[k] for k in names])))
    return grads, {k: (v.detach() if torch.is_tensor(v) else v) for k, v in out.items()}


def _conv_backward(dy, xin, W, dilation):
    """Gradients of y = conv1d(xin, W, b, dilation) written out: (dx, dW, db)."""
    k, L = W.shape[2], dy.shape[2]
    dW = torch.stack([torch.einsum("bot,bit->oi", dy, xin[:, :, j * dilation:j * dilation + L]) for j in range(k)], -1)
    dx = torch.zeros_like(xin)
    for j in range(k):
        dx[:, :, j * dilation:j * dilation + L] += torch.einsum("oi,bot->bit", W[:, :, j], dy)
    return dx, dW, dy.sum((0, 2))


def _slope(pre):
    """LeakyReLU(0.2)'s derivative in the tensor's own precision (at 0 the slope of the negative side, as torch takes it)."""
    return torch.where(pre > 0, torch.ones_like(pre), torch.full_like(pre, 0.2))


def gradients_manual(state, x, hp):
    """The backward as the kernels do it, every formula written out; no autograd."""
    with torch.no_grad():
        P, embeds, x = state["params"], state["embed"], x.to(_dtype(state))
        B, T, nv = x.shape
        e, depth = embeds[0].shape[1], len(embeds)
        enc_in, enc_pre, z = encoder_acts(P, x)
        rows = z.permute(0, 2, 1).reshape(B * T, e)
        tokens, residuals, codes, margins = quantise(embeds, rows)
        commit_levels = [((q - r) ** 2).mean() for q, r in zip(codes, residuals)]
        total = sum(codes[1:], codes[0])
        dec_in, dec_pre, pred = decoder_acts(P, total.reshape(B, T, e).permute(0, 2, 1))
        out = losses(pred, x, commit_levels, hp)
        N = B * T
        dpred = smooth_l1_grad(pred - x) / (N * nv)
        if hp["loss_vel"] > 0:
            gv = hp["loss_vel"] * smooth_l1_grad((pred[..., :-1] - pred[..., 1:]) - (x[..., :-1] - x[..., 1:])) / (N * (nv - 1))
            dpred[..., :-1] += gv
            dpred[..., 1:] -= gv
        grads = {}
        g = dpred.permute(0, 2, 1)
        for j, i in reversed(list(enumerate((0, 2, 4, 6, 8)))):
            if j < 4:
                g = g * _slope(dec_pre[j])
            g, grads[f"decoder.dec.{i}.weight"], grads[f"decoder.dec.{i}.bias"] = _conv_backward(
                g, dec_in[j], P[f"decoder.dec.{i}.weight"], DILATIONS[j] if j < 4 else 1)
        # straight-through: the decoder's gradient reaches z through level 0 alone, and so does the commitment term
        dz = g[:, :, 7:] + hp["commit"] / depth * 2 * (rows - codes[0]).reshape(B, T, e).permute(0, 2, 1) / (N * e)
        g = dz
        for j, i in reversed(list(enumerate((0, 2, 4, 6, 8)))):
            if j < 4:
                g = g * _slope(enc_pre[j])
            g, grads[f"encoder.enc.{i}.weight"], grads[f"encoder.enc.{i}.bias"] = _conv_backward(
                g, enc_in[j], P[f"encoder.enc.{i}.weight"], 1 if j == 0 else DILATIONS[j - 1])
        out.update(tokens=tokens.reshape(B, T, -1), residuals=residuals, margins=margins, pred=pred, preacts=enc_pre[:4] + dec_pre[:4])
        return grads, out


def adamw(state, grads, hp):
    """torch.optim.AdamW's single-tensor path: decoupled decay, then the bias-corrected update."""
    b1, b2 = BETAS
    step = state["step"] + 1
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    new = {"params": dict(state["params"]), "exp_avg": {}, "exp_avg_sq": {}, "step": step}
    for k, g in grads.items():
        p = state["params"][k] * (1 - hp["lr"] * hp["weight_decay"])
        m = state["exp_avg"][k] + (g - state["exp_avg"][k]) * (1 - b1)
        v = state["exp_avg_sq"][k] * b2 + (1 - b2) * g * g
        new["params"][k] = p - hp["lr"] / bc1 * m / (v.sqrt() / math.sqrt(bc2) + ADAM_EPS)
        new["exp_avg"][k], new["exp_avg_sq"][k] = m, v
    return new


def ema(state, tokens, residuals, hp):
    """EuclideanCodebook.forward's training branch per level: one-hot sums, EMA, Laplace-smoothed normalisation."""
    decay, eps = hp.get("decay", 0.99), hp.get("eps", 1e-5)
    tok = tokens.reshape(-1, tokens.shape[-1])
    embed, embed_avg, cluster = [], [], []
    for k, res in enumerate(residuals):
        C = state["embed"][k].shape[0]
        count = torch.bincount(tok[:, k], minlength=C).to(res.dtype)
        sums = torch.zeros_like(state["embed"][k]).index_add_(0, tok[:, k], res)
        cs = state["cluster_size"][k] * decay + count * (1 - decay)
        avg = state["embed_avg"][k] * decay + sums * (1 - decay)
        smoothed = (cs + eps) / (cs.sum() + C * eps) * cs.sum()
        embed.append(avg / smoothed[:, None]), embed_avg.append(avg), cluster.append(cs)
    return {"embed": embed, "embed_avg": embed_avg, "cluster_size": cluster}


def step(state, x, hp, manual=False):
    """One training step: (new state, {losses, perplexity, tokens, grads, margins, preacts})."""
    grads, out = (gradients_manual if manual else gradients_autograd)(state, x, hp)
    new = adamw(state, grads, hp)
    new.update(ema(state, out["tokens"], out["residuals"], hp))
    out["perplexity"] = perplexity(out["tokens"][..., -1], state["embed"][-1].shape[0])
    out["grads"] = grads
    return new, out


def kmeans(samples, means, iters=10):
    """k-means from given starting rows: nearest mean by squared distance (lowest index on a tie), empty clusters keep their mean.
    Returns (means, bins of the last assignment)."""
    samples, means = samples.double(), means.double().clone()
    C = means.shape[0]
    bins = None
    for _ in range(iters):
        d = ((samples[:, None, :] - means[None]) ** 2).sum(-1)
        buckets = d.argmin(1)
        bins = torch.bincount(buckets, minlength=C)
        sums = torch.zeros_like(means).index_add_(0, buckets, samples)
        means = torch.where((bins == 0)[:, None], means, sums / bins.clamp_min(1)[:, None].double())
    return means, bins
