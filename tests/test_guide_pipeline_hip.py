"""The keyframe guide (csrc/kernels_guide.h) at the geometry every public entry point runs it at, against a float64 oracle.

`generate_from_recording`, `generate_from_long_recording`, `continue_recording`, `regenerate_segment` and `bench.py --pipeline`
all drive the guide with 1998 audio tokens (1950 memory rows after the conv stack), 20 keyframes x depth 4 = 80 autoregressive
positions, several sequences per launch and top_p = 0.97.  tests/test_guide_hip.py pins the kernels to the reference's own
vectors at 798 tokens / 8 positions / 2 sequences; this file covers what only that larger geometry reaches: the second pass of
the self-attention score loop (positions >= 64), K/V cache and rotary rows up to 79, cross attention over 1950 rows, the last
`pre_audio` rows, sequence boundaries of the hoisted conv GEMMs, realistic (small) nuclei, a vocabulary that is not a power of
two, edge uniforms of the categorical draw, and the residual-VQ decode at its LDS limit.

The oracle (oracle/guide_oracle.py) runs with every weight and input in float64 except `rotary.freqs`: the reference forms the
rotary angle position x freq in fp32 (its cached table), and a float64 angle at memory rows up to 1949 would not be what it
computes.  Draws are not compared token for token: the oracle is teacher-forced on the GPU's own tokens and every draw must fall
inside the float64 inverse-CDF bracket of its uniform (up to DELTA)."""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from audio2photoreal_amd import _lib
from audio2photoreal_amd.model.guide import GuideTransformer
from audio2photoreal_amd.model.vqvae import TemporalVertexCodec
from audio2photoreal_amd.spec import GuideSpec, TokenizerSpec
from audio2photoreal_amd.synthetic import synthetic_guide_state_dict, synthetic_tensor, synthetic_tokenizer_state_dict
from conftest import record, rel_l2, rel_max
from oracle import guide_oracle as G
from oracle.a2p_oracle import rotary

pytestmark = pytest.mark.gpu
SEED = 10
B, S, KEYS = 4, 1998, 20
PEAK = 8.0                # final_layer x 8: a trained guide's peaked logits (nucleus median 2 / 6 tokens at 0.94 / 0.97 here)
U_MAX = float(np.nextafter(np.float32(1), np.float32(0)))    # 1 - 2^-24, the largest value torch.rand returns
# fp32 gates, ~10x the errors measured on the MI355X (relative; the largest of any sequence / position / T):
#   pre_audio 4.6e-6 (mem / memr 3.4e-6, hidden 8.8e-7), logits 1.0e-6 (x8 scales the absolute logit error by 8),
#   return_probs 2.7e-6 (synthetic) and 1.3e-5 (x8: softmax turns the 8x larger absolute logit error into relative
#   probability error), VQ decode 4.2e-7
PRE_TOL, LOGIT_TOL, VQ_TOL = 5e-5, 1e-5, 5e-6
PROB_TOL = {"broad": 3e-5, "peaked": 1.5e-4}
DELTA = 1e-4              # CDF slack of the nucleus-size and bracket checks: ~10x the largest probability error above
TIE = 1e-5                # relative probability difference under which two tokens may sort either way


def _f64(sd):
    return {k: (v if k == "rotary.freqs" else v.double()) for k, v in sd.items()}


def _peaked(sd):
    return dict(sd, **{k: sd[k] * PEAK for k in ("final_layer.weight", "final_layer.bias")})


def _guide(gs, sd, dev, max_batch=B):
    g = GuideTransformer(tokens=gs.tokens, num_heads=gs.num_heads, num_layers=gs.num_layers, dim=gs.dim, ff_size=gs.ff_size,
                         emb_len=gs.emb_len, num_audio_layers=gs.num_audio_layers, max_batch=max_batch, max_positions=96)
    g.load_state_dict(sd, strict=False)
    return g.to(dev).eval()


def _debug(g, name, shape):
    host = np.empty(shape, np.float32)
    _lib.check(_lib.load().a2p_guide_debug_read(g._ctx, name.encode(), host.ctypes.data_as(C.c_void_p), host.nbytes), "debug_read")
    return torch.from_numpy(host)


def _setup(gs, batch, n_tokens, dev, tag):
    """GPU modules (synthetic and peaked logits) and their float64 oracles, with the conditioning computed once."""
    sd = synthetic_guide_state_dict(gs, SEED)
    sd64 = _f64(sd)
    cond = synthetic_tensor(SEED, tag, (batch, n_tokens, gs.cond_feature_dim))
    o = G.OracleGuide(sd64, gs.tokens, gs.num_layers, gs.num_heads, gs.audio_conv_dilations)
    with torch.no_grad():
        feats = o.pre_audio(cond.double())
        conds = {p: o.condition(None, p, features=feats) for p in (0.0, 1.0)}
    return SimpleNamespace(
        gs=gs, cond=cond.to(dev), feats=feats, conds=conds, sd64=sd64,
        gpu={"broad": _guide(gs, sd, dev, batch), "peaked": _guide(gs, _peaked(sd), dev, batch)},
        oracle={"broad": o, "peaked": G.OracleGuide(_peaked(sd64), gs.tokens, gs.num_layers, gs.num_heads, gs.audio_conv_dilations)})


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def full(dev):
    """Pipeline geometry: 4 sequences x 1998 audio tokens (a distinct condition per sequence)."""
    return _setup(GuideSpec(), B, S, dev, "guide_pipeline_cond")


@pytest.fixture(scope="module")
def mini(dev):
    """A 1000-token, 2-layer guide: the sort runs over 1024 entries, 24 of them padding."""
    return _setup(GuideSpec(tokens=1000, num_layers=2), 3, 200, dev, "guide_pipeline_cond_mini")


def _tf_tokens(gs, batch, n):
    """Start token, then fixed random ids that include the first and the last id."""
    t = torch.from_numpy(np.random.default_rng(SEED + 7).integers(0, gs.tokens, size=(batch, n)))
    t[:, 0] = gs.tokens
    t[:, 5], t[:, n - 3] = 0, gs.tokens - 1
    t[0, n - 1], t[batch - 1, n - 2] = 0, gs.tokens - 1
    return t


def _audit(oracle, cond, toks, u, probs, top_p, start):
    """Teacher-force the oracle on the GPU's own draws (start token prepended) and check every (step, sequence):
    * the nucleus size is the reference rule's on the float64 cumulative mass C (entry k kept while C[k-1] < top_p), up to DELTA;
    * `return_probs` on that support equals the float64 sorted probabilities renormalised over it;
    * the drawn token's bracket [F_lo, F_hi) of the float64 nucleus CDF contains u, up to DELTA (tokens whose probabilities
      differ by less than TIE relative may sort either way: the bracket spans such ties).
    Returns the statistics, violations in `bad`."""
    Bn, n = toks.shape
    prefix = torch.cat([torch.full((Bn, 1), start, dtype=torch.int64), toks[:, :-1]], dim=1)
    with torch.no_grad():
        P, I = torch.sort(torch.softmax(oracle.forward(prefix, None, cond=cond), dim=-1), dim=-1, descending=True)
    Cm = torch.cumsum(P, dim=-1)
    V = P.shape[-1]
    st = SimpleNamespace(sizes=[], size_diff=0, prob_err=0.0, margin=float("inf"), ties=0, bad=[], ranks=[])
    for i in range(n):
        for b in range(Bn):
            p, c, idx, pg = P[b, i], Cm[b, i], I[b, i], probs[i, b].double()
            ng = int((pg > 0).sum())
            n_or = 1 + int((c[:-1] < top_p).sum())
            st.sizes.append(ng)
            st.size_diff += ng != n_or
            if not ((ng == 1 or float(c[ng - 2]) < top_p + DELTA) and (ng == V or float(c[ng - 1]) >= top_p - DELTA)):
                st.bad.append(f"step {i} seq {b}: nucleus of {ng} (float64 rule: {n_or}, mass {float(c[ng - 1]):.7f})")
                continue
            q = p[:ng] / p[:ng].sum()
            st.prob_err = max(st.prob_err, float((pg[:ng] - q).abs().max() / q.max()))
            if bool((pg[ng:] != 0).any()):
                st.bad.append(f"step {i} seq {b}: nonzero probabilities past the nucleus")
            r = int((idx == toks[b, i]).nonzero()[0, 0])
            if r >= ng:
                st.bad.append(f"step {i} seq {b}: token {int(toks[b, i])} has float64 rank {r}, outside the nucleus of {ng}")
                continue
            qa = p / p[:ng].sum()
            qt = float(qa[r])
            lo = float(qa[:ng][qa[:ng] > qt * (1 + TIE)].sum())
            hi = float(qa[:ng][qa[:ng] >= qt * (1 - TIE)].sum())
            F = torch.cumsum(q, 0)
            st.ties += abs(lo - (float(F[r - 1]) if r else 0.0)) > 1e-12 or abs(hi - float(F[r])) > 1e-12
            st.ranks.append((i, b, r, ng, lo, hi))
            uu = float(u[i, b])
            m = min(uu - lo, hi - uu)
            st.margin = min(st.margin, m)
            if m < -DELTA:
                st.bad.append(f"step {i} seq {b}: u = {uu:.8f} outside the bracket [{lo:.8f}, {hi:.8f}) of rank {r} / {ng}")
    return st


def _sizes(st):
    s = np.array(st.sizes)
    return dict(nucleus_median=float(np.median(s)), nucleus_min=int(s.min()), nucleus_max=int(s.max()))


# ------------------------------------------------------------------------------------------------------- a. conditioning
def test_hoisted_conditioning_every_row_every_sequence(full):
    gs, g = full.gs, full.gpu["broad"]
    Sv = gs.cond_tokens_after_conv(S)
    g(torch.full((B, 1), gs.tokens, device=full.cond.device), full.cond)             # prepares the hoisted state
    pre = g.pre_audio_features(B * S).view(B, S, -1)[:, :Sv]
    mem = _debug(g, "mem", (B, S, gs.dim))[:, :Sv]
    memr = _debug(g, "memr", (B, S, gs.dim))[:, :Sv]
    hidden = _debug(g, "hidden", (B, gs.dim))
    mem64, h64 = full.conds[0.0]
    errs = {}
    for b in range(B):
        errs[f"pre_audio_seq{b}"] = rel_l2(pre[b], full.feats[b])
        errs[f"pre_audio_last48_seq{b}"] = rel_l2(pre[b, -48:], full.feats[b, -48:])
        errs[f"pre_audio_last48_max_seq{b}"] = rel_max(pre[b, -48:], full.feats[b, -48:])
    errs["mem"] = rel_l2(mem, mem64)
    errs["memr"] = rel_l2(memr, rotary(mem64, full.sd64["rotary.freqs"]))
    errs["memr_last48"] = rel_l2(memr[:, -48:], rotary(mem64, full.sd64["rotary.freqs"])[:, -48:])
    errs["hidden"] = rel_l2(hidden, h64)
    record("guide_pipeline/conditioning", **errs)
    assert pre.shape == full.feats.shape == (B, 1950, gs.cond_feature_dim)
    assert all(v < PRE_TOL for v in errs.values()), errs


# ------------------------------------------------------------------------------------------------------- b. logits
def _logits_check(ns, drop, n, name, regime="broad"):
    gs, g = ns.gs, ns.gpu[regime]
    toks = _tf_tokens(gs, ns.cond.shape[0], n)
    got = g(toks.to(ns.cond.device), ns.cond, cond_drop_prob=drop).cpu()
    with torch.no_grad():
        want = ns.oracle[regime].forward(toks, None, cond=ns.conds[drop])
    per = [rel_l2(got[:, i], want[:, i]) for i in range(n)]
    per_max = [rel_max(got[:, i], want[:, i]) for i in range(n)]
    tail = max(per[64:]) if n > 64 else max(per)
    record(name, rel_l2=rel_l2(got, want), worst_position_rel_l2=max(per), worst_position=int(np.argmax(per)),
           positions_64_79_rel_l2=tail, worst_position_rel_max=max(per_max), abs_max=float((got - want).abs().max()))
    assert max(per) < LOGIT_TOL and max(per_max) < LOGIT_TOL, (per, per_max)
    assert tail < LOGIT_TOL, per[64:]


@pytest.mark.parametrize("regime,drop", [("broad", 0.0), ("broad", 1.0), ("peaked", 0.0)])
def test_teacher_forced_logits_at_80_positions(full, regime, drop):
    _logits_check(full, drop, KEYS * 4, f"guide_pipeline/logits_{regime}_drop{int(drop)}", regime)


# ------------------------------------------------------------------------------------------------------- c. draws
def _generate(ns, regime, u, top_p, keys):
    g = ns.gpu[regime]
    n_seq = ns.cond.shape[0]
    toks, probs = g.generate(ns.cond, keys, 4, n_sequences=n_seq, max_key_len=keys, max_seq_len=30 * keys, top_p=top_p,
                             uniforms=u.to(ns.cond.device), return_probs=True)
    return toks.cpu(), probs.cpu()


@pytest.mark.parametrize("regime", ["broad", "peaked"])
@pytest.mark.parametrize("top_p", [0.0, 0.94, 0.97, 1.0])
def test_generate_draws_inside_the_float64_bracket(full, regime, top_p):
    u = torch.rand(KEYS * 4, B, generator=torch.Generator().manual_seed(int(100 * top_p) + (regime == "peaked")))
    toks, probs = _generate(full, regime, u, top_p, KEYS)
    st = _audit(full.oracle[regime], full.conds[0.0], toks, u, probs, top_p, full.gs.tokens)
    record(f"guide_pipeline/generate_{regime}_p{top_p}", return_probs_err=st.prob_err, min_bracket_margin=st.margin,
           size_differs_near_cut=st.size_diff, tie_brackets=st.ties, violations=len(st.bad), **_sizes(st))
    assert not st.bad, st.bad[:10]
    assert st.prob_err < PROB_TOL[regime]
    if top_p == 0.0:
        assert set(st.sizes) == {1}
    if top_p in (0.94, 0.97):
        med = np.median(st.sizes)
        assert (med >= 500) if regime == "broad" else (med <= 16), med


def _edge_checks(ns, regime, keys, top_p):
    """Whole rows of u = 0 (the head of the nucleus) and u = 1 - 2^-24 (its tail: never the head unless it holds one token)."""
    n_seq, n = ns.cond.shape[0], keys * 4
    bad, head_draws = [], 0
    for uval in (0.0, U_MAX):
        u = torch.full((n, n_seq), uval)
        toks, probs = _generate(ns, regime, u, top_p, keys)
        st = _audit(ns.oracle[regime], ns.conds[0.0], toks, u, probs, top_p, ns.gs.tokens)
        bad += [f"u={uval}: " + s for s in st.bad]
        for i, b, r, ng, lo, hi in st.ranks:              # lo / hi: the float64 bracket of the drawn token (ties spanned)
            if uval == 0.0 and lo > DELTA:
                bad.append(f"u=0 step {i} seq {b}: float64 rank {r}, not the head")
            if uval == U_MAX:
                head_draws += r == 0 and ng > 1
                if hi <= 1 - DELTA or (r == 0 and ng > 1):
                    bad.append(f"u=1-2^-24 step {i} seq {b}: float64 rank {r} of a nucleus of {ng}")
    return bad, head_draws


@pytest.mark.parametrize("regime", ["broad", "peaked"])
def test_generate_edge_uniforms(full, regime):
    bad, head = _edge_checks(full, regime, KEYS, 0.97)
    record(f"guide_pipeline/edge_uniforms_{regime}", violations=len(bad), head_draws_at_u_max=head)
    assert not bad, f"{len(bad)} bad draws: {bad[:10]}"


# ------------------------------------------------------------------------------------------------------- d. V = 1000
def test_non_power_of_two_vocabulary_logits(mini):
    _logits_check(mini, 0.0, 24, "guide_pipeline/mini_v1000_logits")


@pytest.mark.parametrize("regime", ["broad", "peaked"])
def test_non_power_of_two_vocabulary_draws(mini, regime):
    n_seq = mini.cond.shape[0]
    u = torch.rand(24, n_seq, generator=torch.Generator().manual_seed(11))
    toks, probs = _generate(mini, regime, u, 0.97, 6)
    st = _audit(mini.oracle[regime], mini.conds[0.0], toks, u, probs, 0.97, mini.gs.tokens)
    bad, head = _edge_checks(mini, regime, 6, 0.97)
    record(f"guide_pipeline/mini_v1000_generate_{regime}", return_probs_err=st.prob_err, min_bracket_margin=st.margin,
           violations=len(st.bad) + len(bad), head_draws_at_u_max=head, **_sizes(st))
    assert int(toks.max()) < 1000 and not st.bad and not bad, (st.bad + bad)[:10]
    assert st.prob_err < PROB_TOL[regime]


# ------------------------------------------------------------------------------------------------------- e. VQ decode
@pytest.fixture(scope="module")
def vq(dev):
    ts = TokenizerSpec()
    sd = synthetic_tokenizer_state_dict(ts, SEED)
    t = TemporalVertexCodec(ts.n_vertices, ts.latent_dim, ts.categories, ts.residual_depth)
    t.load_state_dict(sd, strict=False)
    return SimpleNamespace(ts=ts, tok=t.to(dev), sd64={k: v.double() for k, v in sd.items()})


def _vq_err(vq, q, dev):
    got = vq.tok.decode(q.to(dev)).cpu()
    want = G.vq_decode(vq.sd64, q, vq.ts.residual_depth)
    assert got.shape == want.shape == (q.shape[0], q.shape[1], vq.ts.n_vertices)
    return max(rel_l2(got, want), rel_max(got, want))


def test_vq_decode_of_drawn_tokens_and_edge_ids(full, vq, dev):
    u = torch.rand(KEYS * 4, B, generator=torch.Generator().manual_seed(97))
    toks, _ = _generate(full, "peaked", u, 0.97, KEYS)
    q = toks.reshape(B, KEYS, 4).clone()
    q[:, 3], q[:, 11] = 0, vq.ts.categories - 1
    errs = {"drawn_T20": _vq_err(vq, q, dev)}
    gen = torch.Generator().manual_seed(5)
    for T in range(1, 8):                            # shorter than the receptive field: left padding only
        errs[f"T{T}"] = _vq_err(vq, torch.randint(0, vq.ts.categories, (2, T, 4), generator=gen), dev)
    errs["T121"] = _vq_err(vq, torch.randint(0, vq.ts.categories, (2, 121, 4), generator=gen), dev)   # 2 (T + 7) 64 4 = 64 KB
    record("guide_pipeline/vq_decode", **errs)
    assert all(v < VQ_TOL for v in errs.values()), errs
    with pytest.raises(_lib.A2PError):
        vq.tok.decode(torch.zeros(2, 122, 4, dtype=torch.int64, device=dev))


def test_replace_keyframes_at_600_frames(full, vq, dev):
    from audio2photoreal_amd.sample.generate import _replace_keyframes
    g = full.gpu["broad"]
    u = torch.rand(KEYS * 4, B, generator=torch.Generator().manual_seed(98)).to(dev)
    y = {"cond_embed": full.cond, "keyframes": torch.zeros(B, KEYS, vq.ts.n_vertices, device=dev)}
    pred = _replace_keyframes({"y": y}, SimpleNamespace(transformer=g, tokenizer=vq.tok), uniforms=u, top_p=0.97)
    toks = g.generate(full.cond, KEYS, 4, n_sequences=B, max_key_len=KEYS, max_seq_len=30 * KEYS, top_p=0.97, uniforms=u)
    want = G.vq_decode(vq.sd64, toks.cpu().reshape(B, KEYS, 4), vq.ts.residual_depth)
    e = max(rel_l2(pred, want), rel_max(pred, want))
    record("guide_pipeline/replace_keyframes_600", rel=e)
    assert pred.shape == (B, KEYS, vq.ts.n_vertices) and e < VQ_TOL
