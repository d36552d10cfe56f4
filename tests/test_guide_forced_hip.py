"""Keyframes from known poses on the MI355X: the residual-VQ encode (csrc/kernels_vq.h vq_encode_kernel) against the reference's
vectors, forced positions of the guide's autoregressive kernel (csrc/kernels_guide.h guide_ar_kernel, a2p_guide_generate_forced)
bit for bit against its own free draws and against the float64 oracle, and the four public options end to end.

Guide geometry: the pipeline's (4 x 1998 audio tokens, 20 keyframes x depth 4 = 80 positions, top_p 0.97)."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import vq_encode_restatement as VE
from audio2photoreal_amd import _lib
from audio2photoreal_amd.model.guide import check_forced_result
from audio2photoreal_amd.model.vqvae import TemporalVertexCodec
from audio2photoreal_amd.spec import GuideSpec, TokenizerSpec
from audio2photoreal_amd.synthetic import synthetic_tokenizer_encoder_state_dict, synthetic_tokenizer_state_dict
from conftest import record, rel_l2, rel_max
from test_guide_pipeline_hip import _setup
from test_inpaint_hip import _recording, _stats

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 10
B, S, KEYS, DEPTH = 4, 1998, 20, 4
N = KEYS * DEPTH
TOP_P = 0.97
# fp32 gate of the encoder latents (relative, L2 and max): ~10x the largest error measured on the MI355X, 6.9e-7 (records
# "guide_forced/vq_encode_*")
LAT_TOL = 1e-5
TIE = 1e-3                # float64 distance gap under which two codes may be picked either way in fp32
DELTA = 1e-4              # CDF slack of the bracket check (tests/test_guide_pipeline_hip.py)
TIE_P = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "golden_vq_encode_v1.npz"))


@pytest.fixture(scope="module")
def vq(dev):
    ts = TokenizerSpec()
    sd = {**synthetic_tokenizer_state_dict(ts, SEED), **synthetic_tokenizer_encoder_state_dict(ts, SEED)}
    t = TemporalVertexCodec(ts.n_vertices, ts.latent_dim, ts.categories, ts.residual_depth, with_encoder=True)
    t.load_state_dict(sd)
    return SimpleNamespace(ts=ts, sd=sd, tok=t.to(dev))


def _encode_abi(vq, poses, half, want_tokens=True, want_latents=True):
    """a2p_vq_encode of the fp32 or the IEEE-half library, straight through the C ABI."""
    books, norms, ws, bs = vq.tok._stage_encoder(poses.device)
    Bq, T, _ = poses.shape
    x = poses.float().contiguous()
    q = torch.full((Bq, T, DEPTH), -7, dtype=torch.int64, device=x.device) if want_tokens else None
    lat = torch.empty(Bq, T, vq.ts.latent_dim, device=x.device) if want_latents else None
    arr = lambda ts: (C.c_void_p * len(ts))(*[t.data_ptr() for t in ts])               # noqa: E731
    lib = _lib.load(half)
    rc = lib.a2p_vq_encode(_lib.ptr(x), Bq, T, DEPTH, vq.ts.categories, vq.ts.latent_dim, vq.ts.n_vertices, arr(books), arr(norms),
                           arr(ws), arr(bs), _lib.ptr(q), _lib.ptr(lat), _lib.current_stream(x.device))
    _lib.check(rc, "a2p_vq_encode")
    torch.cuda.synchronize()
    return (None if q is None else q.cpu()), (None if lat is None else lat.cpu())


def _pick_gaps(sd, lat64, tokens):
    """float64 distance of each fp32 pick minus the float64 minimum, along the residual path of the picks: [B, T, depth]."""
    res = lat64.reshape(-1, lat64.shape[-1])
    q = tokens.reshape(-1, tokens.shape[-1])
    gaps = []
    for k in range(q.shape[1]):
        d = VE.distances(sd, k, res)
        gaps.append(d.gather(1, q[:, k:k + 1])[:, 0] - d.min(1).values)
        res = res - sd[f"quantizer.layers.{k}._codebook.embed"].double()[q[:, k]]
    return torch.stack(gaps, -1).reshape(tokens.shape)


# ------------------------------------------------------------------------------------------------------- 1. encode
@pytest.mark.parametrize("half", [False, True], ids=["fp32_lib", "fp16_lib"])
def test_encode_against_the_reference(vq, golden, dev, half):
    errs, ties = {}, 0
    for name in ("randn", "decoded"):
        poses = torch.from_numpy(golden[f"{name}/poses"])
        q, lat = _encode_abi(vq, poses.to(dev), half)
        want_lat = torch.from_numpy(golden[f"{name}/latents"])
        lat64 = VE.encoder(vq.sd, poses)
        errs[f"{name}_latents_vs_reference"] = max(rel_l2(lat, want_lat), rel_max(lat, want_lat))
        errs[f"{name}_latents_vs_float64"] = max(rel_l2(lat, lat64), rel_max(lat, lat64))
        margin = torch.from_numpy(golden[f"{name}/margin"])
        want_q = torch.from_numpy(golden[f"{name}/tokens"])
        sure = margin > TIE
        ties += int((~sure).sum())
        assert torch.equal(q[sure], want_q[sure]), f"{name}: {int((q != want_q)[sure].sum())} tokens differ outside the tie zone"
        gaps = _pick_gaps(vq.sd, lat64, q)
        errs[f"{name}_max_pick_gap"] = float(gaps.max())
        assert float(gaps.max()) <= TIE, float(gaps.max())
        q2 = vq.tok.encode(poses.to(dev)).cpu()
        assert torch.equal(q2, q) and torch.equal(vq.tok.predict(poses.to(dev)).cpu(), q)
        assert torch.equal(vq.tok.encoder(poses.to(dev)).cpu(), lat)
    record(f"guide_forced/vq_encode_golden_{'fp16' if half else 'fp32'}_lib", tie_zone_entries=ties, **errs)
    assert all(v < LAT_TOL for k, v in errs.items() if "latents" in k), errs


def test_encode_lengths_up_to_the_lds_limit(vq, dev):
    gen = torch.Generator().manual_seed(31)
    errs, ties = {}, 0
    for T in list(range(1, 9)) + [20, 64, 120, 121]:           # 2 (T + 7) 64 4 bytes: 64 KB at T = 121
        poses = torch.randn(2, T, vq.ts.n_vertices, generator=gen)
        q, lat = _encode_abi(vq, poses.to(dev), False)
        lat64 = VE.encoder(vq.sd, poses)
        errs[f"T{T}"] = max(rel_l2(lat, lat64), rel_max(lat, lat64))
        gaps = _pick_gaps(vq.sd, lat64, q)
        assert float(gaps.max()) <= TIE, (T, float(gaps.max()))
        want = VE.quantize(vq.sd, lat64, DEPTH)
        ties += int((q != want).sum())
        assert bool(((q >= 0) & (q < vq.ts.categories)).all())
        q_only, _ = _encode_abi(vq, poses.to(dev), False, want_latents=False)
        _, lat_only = _encode_abi(vq, poses.to(dev), False, want_tokens=False)
        assert torch.equal(q_only, q) and torch.equal(lat_only, lat)
    record("guide_forced/vq_encode_lengths", tokens_off_float64=ties, **errs)
    assert all(v < LAT_TOL for v in errs.values()), errs
    with pytest.raises(_lib.A2PError, match="LDS"):
        vq.tok.encode(torch.zeros(2, 122, vq.ts.n_vertices, device=dev))


@pytest.mark.parametrize("latent,categories", [(128, 256), (32, 128)])
def test_encode_both_outputs_at_other_latent_widths(dev, latent, categories):
    """Tokens and latents from one launch at widths where a wave's rows are not the rows it copied to latents_out, from T = 1 up
    to the LDS limit; one frame past it is refused."""
    ts = TokenizerSpec(latent_dim=latent, categories=categories)
    sd = {**synthetic_tokenizer_state_dict(ts, SEED), **synthetic_tokenizer_encoder_state_dict(ts, SEED)}
    t = TemporalVertexCodec(ts.n_vertices, ts.latent_dim, ts.categories, ts.residual_depth, with_encoder=True)
    t.load_state_dict(sd)
    ns = SimpleNamespace(ts=ts, sd=sd, tok=t.to(dev))
    t_max = 65536 // (2 * latent * 4) - 7                    # 2 (T + 7) latent 4 bytes <= 64 KB
    gen = torch.Generator().manual_seed(latent)
    errs = {}
    for T in (1, 20, t_max):
        poses = torch.randn(3, T, ts.n_vertices, generator=gen)
        q, lat = _encode_abi(ns, poses.to(dev), False)
        lat64 = VE.encoder(sd, poses)
        errs[f"T{T}"] = max(rel_l2(lat, lat64), rel_max(lat, lat64))
        gaps = _pick_gaps(sd, lat64, q)
        assert float(gaps.max()) <= TIE, (T, float(gaps.max()))
        q_only, _ = _encode_abi(ns, poses.to(dev), False, want_latents=False)
        _, lat_only = _encode_abi(ns, poses.to(dev), False, want_tokens=False)
        assert torch.equal(q_only, q) and torch.equal(lat_only, lat), T
    record(f"guide_forced/vq_encode_latent{latent}", **errs)
    assert all(v < LAT_TOL for v in errs.values()), errs
    with pytest.raises(_lib.A2PError, match="LDS"):
        ns.tok.encode(torch.zeros(1, t_max + 1, ts.n_vertices, device=dev))


def test_encode_refuses_an_encoder_that_was_never_loaded(dev):
    ts = TokenizerSpec()
    t = TemporalVertexCodec(ts.n_vertices, ts.latent_dim, ts.categories, ts.residual_depth, with_encoder=True)
    t.load_state_dict(synthetic_tokenizer_state_dict(ts, SEED), strict=False)            # decode side only
    t = t.to(dev)
    with pytest.raises(_lib.A2PError, match="all zero"):
        t.encode(torch.zeros(1, 4, ts.n_vertices, device=dev))


# ------------------------------------------------------------------------------------------------------- 2. guide identities
@pytest.fixture(scope="module")
def full(dev):
    return _setup(GuideSpec(), B, S, dev, "guide_pipeline_cond")


def _gen(ns, u, forced=None, regime="broad"):
    g = ns.gpu[regime]
    kw = {} if forced is None else {"forced_tokens": forced}
    toks, probs = g.generate(ns.cond, KEYS, DEPTH, n_sequences=B, max_key_len=KEYS, max_seq_len=30 * KEYS, top_p=TOP_P,
                             uniforms=u.to(ns.cond.device), return_probs=True, **kw)
    return toks.cpu(), probs.cpu()


def _bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


@pytest.mark.parametrize("regime", ["broad", "peaked"])
def test_forced_all_free_is_the_plain_draw(full, regime):
    u = torch.rand(N, B, generator=torch.Generator().manual_seed(41))
    t0, p0 = _gen(full, u, regime=regime)
    t1, p1 = _gen(full, u, torch.full((B, N), -1, dtype=torch.int64), regime)
    assert torch.equal(t0, t1) and _bits(p0, p1)


def _subsets():
    idx = torch.arange(N)
    return {"prefix": idx < 40, "holes": (idx % 3) == 1, "suffix": idx >= N - 20, "alternate_keyframes": (idx // DEPTH) % 2 == 0}


@pytest.mark.parametrize("regime", ["broad", "peaked"])
def test_forcing_a_runs_own_tokens_returns_that_run(full, regime):
    u = torch.rand(N, B, generator=torch.Generator().manual_seed(42))
    t0, p0 = _gen(full, u, regime=regime)
    for name, pos in _subsets().items():
        m = pos[None].expand(B, N).clone()
        m[1] = m[1].roll(7)                                  # a different subset per sequence
        forced = torch.where(m, t0, torch.full_like(t0, -1))
        t1, p1 = _gen(full, u, forced, regime)
        assert torch.equal(t1, t0), f"{name}: {int((t1 != t0).sum())} tokens differ"
        free = ~m.t()                                        # [N, B] like probs
        assert _bits(p1[free], p0[free]), name
        assert bool((p1[~free] == 0).all()), name            # forced rows: zero-filled
        assert torch.equal(t1[m], forced[m])                 # forced positions echo their values


def test_forced_positions_echo_arbitrary_values(full):
    """Forcing ids the draw would not pick: they come back as given, every free position stays a valid draw."""
    u = torch.rand(N, B, generator=torch.Generator().manual_seed(43))
    forced = torch.full((B, N), -1, dtype=torch.int64)
    forced[:, 0], forced[:, 17], forced[:, N - 1] = 0, full.gs.tokens - 1, 5
    forced[2, 30:50] = torch.arange(20) * 51
    t, p = _gen(full, u, forced)
    m = forced != -1
    assert torch.equal(t[m], forced[m]) and bool((p.transpose(0, 1)[m] == 0).all())
    assert bool(((t >= 0) & (t < full.gs.tokens)).all())


def test_out_of_range_forced_value_stops_the_sequence_through_the_abi(full, dev):
    g = full.gpu["broad"]
    u = torch.rand(N, B, generator=torch.Generator().manual_seed(44))
    t0, _ = _gen(full, u)
    forced = torch.full((B, N), -1, dtype=torch.int64)
    forced[1, 5], forced[3, 0], forced[2, N - 1] = full.gs.tokens, -9, 1 << 40
    fd, ud = forced.to(dev), u.to(dev).contiguous()
    out = torch.full((B, N), -7, dtype=torch.int64, device=dev)
    rc = _lib.load().a2p_guide_generate_forced(g._ctx, B, N, TOP_P, _lib.ptr(ud), _lib.ptr(fd), _lib.ptr(out), None, _lib.current_stream(dev))
    assert rc == 0
    torch.cuda.synchronize()
    got = out.cpu()
    assert got[1, 5] == -2 and got[3, 0] == -2 and got[2, N - 1] == -2
    assert torch.equal(got[0], t0[0]) and torch.equal(got[1, :5], t0[1, :5]) and torch.equal(got[2, :N - 1], t0[2, :N - 1])
    with pytest.raises(_lib.A2PError, match="sequence 1 stopped at position 5"):
        check_forced_result(out)
    t1, _ = _gen(full, u)                                     # the context is unharmed
    assert torch.equal(t1, t0)


# ------------------------------------------------------------------------------------------------------- 3. against the oracle
def test_free_draws_after_an_encoded_prefix_lie_in_the_float64_bracket(full, vq, dev):
    """A prefix of 8 keyframes forced to the tokens of encoded random poses; every later draw must fall inside the float64
    inverse-CDF bracket of the oracle, teacher-forced on the GPU's tokens (tests/test_guide_pipeline_hip.py _audit's rule)."""
    nk = 8
    poses = torch.randn(B, KEYS, vq.ts.n_vertices, generator=torch.Generator().manual_seed(45))
    kt = vq.tok.encode(poses.to(dev)).cpu()
    forced = torch.full((B, KEYS, DEPTH), -1, dtype=torch.int64)
    forced[:, :nk] = kt[:, :nk]
    forced = forced.reshape(B, N)
    u = torch.rand(N, B, generator=torch.Generator().manual_seed(46))
    toks, probs = _gen(full, u, forced)
    assert torch.equal(toks[:, :nk * DEPTH], forced[:, :nk * DEPTH])
    prefix = torch.cat([torch.full((B, 1), full.gs.tokens, dtype=torch.int64), toks[:, :-1]], dim=1)
    with torch.no_grad():
        P, I = torch.sort(torch.softmax(full.oracle["broad"].forward(prefix, None, cond=full.conds[0.0]), dim=-1), dim=-1, descending=True)
    Cm = torch.cumsum(P, dim=-1)
    bad, margin, n_checked = [], float("inf"), 0
    for i in range(nk * DEPTH, N):
        for b in range(B):
            p, c, idx = P[b, i], Cm[b, i], I[b, i]
            ng = int((probs[i, b] > 0).sum())
            if not ((ng == 1 or float(c[ng - 2]) < TOP_P + DELTA) and float(c[ng - 1]) >= TOP_P - DELTA):
                bad.append(f"step {i} seq {b}: nucleus of {ng}")
                continue
            r = int((idx == toks[b, i]).nonzero()[0, 0])
            if r >= ng:
                bad.append(f"step {i} seq {b}: rank {r} outside the nucleus of {ng}")
                continue
            qa = p / p[:ng].sum()
            qt = float(qa[r])
            lo = float(qa[:ng][qa[:ng] > qt * (1 + TIE_P)].sum())
            hi = float(qa[:ng][qa[:ng] >= qt * (1 - TIE_P)].sum())
            m = min(float(u[i, b]) - lo, hi - float(u[i, b]))
            margin = min(margin, m)
            n_checked += 1
            if m < -DELTA:
                bad.append(f"step {i} seq {b}: u = {float(u[i, b]):.8f} outside [{lo:.8f}, {hi:.8f})")
    record("guide_forced/bracket_after_encoded_prefix", draws=n_checked, min_bracket_margin=margin, violations=len(bad))
    assert not bad, bad[:10]
    assert bool((probs[:nk * DEPTH] == 0).all())


# ------------------------------------------------------------------------------------------------------- 4. end to end
MAX_BATCH = 8
_MODELS = {}


def _models(dev, precision):
    """inpaint tests' 2-layer face / body models (ddim10), the body's tokenizer built with its encoder."""
    if precision in _MODELS:
        return _MODELS[precision]
    from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from audio2photoreal_amd.model.guide import GuideTransformer
    from audio2photoreal_amd.model_util import create_model_and_diffusion, default_args, load_model
    from audio2photoreal_amd.spec import face_spec, pose_spec
    from audio2photoreal_amd.synthetic import synthetic_frontend_state_dict, synthetic_guide_state_dict, synthetic_state_dict
    gs, ts = GuideSpec(), TokenizerSpec()
    guide = GuideTransformer(tokens=gs.tokens, num_layers=gs.num_layers, dim=gs.dim, emb_len=gs.emb_len,
                             num_audio_layers=gs.num_audio_layers, max_batch=MAX_BATCH, max_positions=96)
    guide.load_state_dict(synthetic_guide_state_dict(gs, SEED), strict=False)
    tok = TemporalVertexCodec(ts.n_vertices, ts.latent_dim, ts.categories, ts.residual_depth, with_encoder=True)
    tok.load_state_dict({**synthetic_tokenizer_state_dict(ts, SEED), **synthetic_tokenizer_encoder_state_dict(ts, SEED)})
    out = {}
    for fmt, spec in (("face", face_spec(num_layers=2)), ("pose", pose_spec(num_layers=2))):
        m, d = create_model_and_diffusion(default_args(fmt, layers=2, timestep_respacing="ddim10"), "test", precision=precision,
                                          max_batch=MAX_BATCH, audio_frontend="native")
        load_model(m, {**synthetic_state_dict(spec, SEED), **synthetic_frontend_state_dict(SEED, lip=fmt == "face")})
        if fmt == "pose":
            m.setup_guide_predictor(guide.to(dev).eval(), tok.to(dev))
        out[fmt] = (ClassifierFreeSampleModel(m.to(dev).eval()), d)
    _MODELS[precision] = out
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if isinstance(a[k], np.ndarray):
            x, y = np.ascontiguousarray(a[k]), np.ascontiguousarray(b[k])
            assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8)), k
        else:
            assert a[k] == b[k], k


class _Capture:
    """Wraps sample.inpaint._replace_keyframes and keeps the keyframes each call returns."""
    def __init__(self, monkeypatch):
        from audio2photoreal_amd.sample import inpaint
        self.calls = []
        orig = inpaint._replace_keyframes

        def wrapped(*a, **kw):
            out = orig(*a, **kw)
            self.calls.append(out.clone())
            return out
        monkeypatch.setattr(inpaint, "_replace_keyframes", wrapped)


class _GenerateSpy:
    """Wraps the pose model's GuideTransformer.generate and keeps (forced_tokens, tokens) of each call."""
    def __init__(self, model, monkeypatch):
        g = model.model.transformer
        self.calls = []
        orig = g.generate

        def wrapped(*a, **kw):
            out = orig(*a, **kw)
            f = kw.get("forced_tokens")
            self.calls.append((None if f is None else f.detach().cpu().clone(), out.detach().cpu().clone()))
            return out
        monkeypatch.setattr(g, "generate", wrapped)


def _check_forced(call, tok, known, mask, dev):
    """The guide was given encode(known)'s tokens at the known keyframes and -1 elsewhere, and returned them there."""
    forced, toks = call
    R, nk, _ = known.shape
    assert forced is not None, "no forced tokens reached the guide"
    forced, toks = forced.reshape(R, nk, DEPTH), toks.reshape(R, nk, DEPTH)
    want = tok.encode(known.to(dev)).cpu()
    assert torch.equal(forced[mask], want[mask]) and bool((forced[~mask] == -1).all())
    assert torch.equal(toks[mask], want[mask])
    return toks


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_continue_recording_guide_context(dev, precision, monkeypatch):
    from audio2photoreal_amd.sample.inpaint import _normalised
    from audio2photoreal_amd.sample.recording import continue_recording, generate_from_recording
    m = _models(dev, precision)
    stats = _stats()
    prev = generate_from_recording(m["face"], m["pose"], stats, _recording(8.0), 44100, num_repetitions=2, seed=3)
    P = 120
    cap, spy = _Capture(monkeypatch), _GenerateSpy(m["pose"][0], monkeypatch)
    res = continue_recording(m["face"], m["pose"], stats, _recording(4.0, seed=8), 44100, prev, context_frames=P, seed=4,
                             guide_context=True)
    kf = cap.calls[-1]
    want = _normalised(prev["pose"][:, -P:], stats["pose_mean"], stats["pose_std"], "cpu")[:, :, 0, ::30].transpose(1, 2)
    assert _bits(kf[:, :P // 30], want)
    nk = kf.shape[1]
    known = torch.zeros(2, nk, 104)
    known[:, :P // 30] = want
    mask = torch.zeros(2, nk, dtype=torch.bool)
    mask[:, :P // 30] = True
    tok = m["pose"][0].model.tokenizer
    toks = _check_forced(spy.calls[-1], tok, known, mask, dev)
    assert _bits(kf[:, P // 30:], tok.decode(toks.to(dev)).cpu()[:, P // 30:])     # free rows: the decode of the forced draw
    assert np.isfinite(res["pose"]).all() and res["keyframes"].shape == (2, 4, 104)
    if precision == "fp32":
        _same(continue_recording(m["face"], m["pose"], stats, _recording(4.0, seed=8), 44100, prev, context_frames=P, seed=4,
                                 guide_context=False),
              continue_recording(m["face"], m["pose"], stats, _recording(4.0, seed=8), 44100, prev, context_frames=P, seed=4))


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_regenerate_segment_guide_context(dev, precision, monkeypatch):
    from audio2photoreal_amd.sample.inpaint import _normalised
    from audio2photoreal_amd.sample.recording import generate_from_recording, regenerate_segment
    m = _models(dev, precision)
    stats = _stats()
    res = generate_from_recording(m["face"], m["pose"], stats, _recording(8.0), 44100, num_repetitions=2, seed=5)
    s, e = 90, 150
    cap, spy = _Capture(monkeypatch), _GenerateSpy(m["pose"][0], monkeypatch)
    out = regenerate_segment(m["face"], m["pose"], stats, res, s, e, parts=("pose",), seed=6, guide_context=True)
    kf = cap.calls[-1]
    want = _normalised(res["pose"], stats["pose_mean"], stats["pose_std"], "cpu")[:, :, 0, ::30].transpose(1, 2)
    outside = torch.ones(kf.shape[1], dtype=torch.bool)
    outside[s // 30:e // 30] = False
    assert _bits(kf[:, outside], want[:, outside])
    _check_forced(spy.calls[-1], m["pose"][0].model.tokenizer, want, outside[None].expand(2, -1), dev)
    assert np.array_equal(out["pose"][:, :s], res["pose"][:, :s]) and np.array_equal(out["pose"][:, e:], res["pose"][:, e:])
    if precision == "fp32":
        _same(regenerate_segment(m["face"], m["pose"], stats, res, s, e, seed=6, guide_context=False),
              regenerate_segment(m["face"], m["pose"], stats, res, s, e, seed=6))


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_long_recording_chain_keyframes(dev, precision, monkeypatch):
    from audio2photoreal_amd.sample.long_form import generate_from_long_recording
    m = _models(dev, precision)
    stats = _stats()
    wav = _recording(24.0)                                   # 720 frames: 2 windows of 600
    spy = _GenerateSpy(m["pose"][0], monkeypatch)
    out = generate_from_long_recording(m["face"], m["pose"], stats, wav, 44100, num_repetitions=2, seed=7, chain_keyframes=True)
    starts, kf = out["window_starts"], out["keyframes"]
    assert len(starts) == 2 and kf.shape == (2, 2, 20, 104)
    assert len(spy.calls) == 2 and spy.calls[0][0] is None   # one guide launch per window, window 0 unforced
    for w in range(1, len(starts)):
        off = (starts[w] - starts[w - 1]) // 30
        assert np.array_equal(kf[:, w, :20 - off], kf[:, w - 1, off:])
        forced, toks = (t.reshape(2, 20, DEPTH) for t in spy.calls[w])
        prev = spy.calls[w - 1][1].reshape(2, 20, DEPTH)
        assert torch.equal(forced[:, :20 - off], prev[:, off:]) and bool((forced[:, 20 - off:] == -1).all())
        assert torch.equal(toks[:, :20 - off], prev[:, off:])
    plain = generate_from_long_recording(m["face"], m["pose"], stats, wav, 44100, num_repetitions=2, seed=7)
    assert np.array_equal(kf[:, 0], plain["keyframes"][:, 0])       # window 0 draws what it draws unchained
    assert np.isfinite(out["pose"]).all()
    if precision == "fp32":
        _same(generate_from_long_recording(m["face"], m["pose"], stats, wav, 44100, num_repetitions=2, seed=7, chain_keyframes=False),
              plain)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_generate_from_recording_known_keyframes(dev, precision, monkeypatch):
    from audio2photoreal_amd.sample.recording import generate_from_recording
    m = _models(dev, precision)
    stats = _stats()
    rng = np.random.default_rng(12)
    known = {0: stats["pose_mean"] + stats["pose_std"] * rng.standard_normal(104),
             210: stats["pose_mean"] + stats["pose_std"] * rng.standard_normal(104)}
    spy = _GenerateSpy(m["pose"][0], monkeypatch)
    out = generate_from_recording(m["face"], m["pose"], stats, _recording(8.0), 44100, num_repetitions=2, seed=9,
                                  known_keyframes=known)
    nk = out["keyframes"].shape[1]
    kn = torch.zeros(2, nk, 104)
    mask = torch.zeros(2, nk, dtype=torch.bool)
    for f, pose in known.items():
        kn[:, f // 30] = torch.from_numpy(((pose - stats["pose_mean"]) / stats["pose_std"]).astype(np.float32))
        mask[:, f // 30] = True
    _check_forced(spy.calls[-1], m["pose"][0].model.tokenizer, kn, mask, dev)
    err = 0.0
    for f, pose in known.items():
        got = out["keyframes"][:, f // 30]
        err = max(err, float(np.abs(got - pose).max() / np.abs(pose).max()))
    record(f"guide_forced/known_keyframes_roundtrip_{precision}", rel_max=err)
    assert err < 1e-6                                        # fp32 cast of the normalised pose, un-normalised in float64
    assert np.isfinite(out["pose"]).all()
    if precision == "fp32":
        _same(generate_from_recording(m["face"], m["pose"], stats, _recording(8.0), 44100, num_repetitions=2, seed=9, known_keyframes=None),
              generate_from_recording(m["face"], m["pose"], stats, _recording(8.0), 44100, num_repetitions=2, seed=9))
