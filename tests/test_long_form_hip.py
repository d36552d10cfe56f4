"""Windowed joint sampling of long recordings on the MI355X (sample/long_form.py, csrc/kernels_window.h): one window is the
existing path bit for bit, the windowed step tail against a float32 restatement from the per-window guided forwards, the
"every copy of a shared frame holds the same bits" invariant after every step, the window gathers against host slices, and
a 60 s recording end to end."""
import ctypes as C

import numpy as np
import pytest
import torch

from audio2photoreal_amd import _lib
from audio2photoreal_amd.sample.long_form import (generate_from_long_recording, plan_windows, prepare_long_recording,
                                                  window_gather, windowed_sample_loop)
from audio2photoreal_amd.sample.recording import generate_from_recording, prepare_recording

pytestmark = pytest.mark.gpu
SEED = 10
SR = 44100
MAX_BATCH = 8
PRECISIONS = ["fp32", "fp16"]
FORMATS = ["face", "pose"]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _recording(seconds, sr=SR, seed=7):
    """A synthetic stereo int16 recording [L, 2]: tones with a slow amplitude swell + noise."""
    n = int(round(seconds * sr))
    t = np.arange(n) / sr
    rng = np.random.default_rng(seed)
    env = 0.6 + 0.4 * np.sin(2 * np.pi * t / 7.0)
    left = env * (9000 * np.sin(2 * np.pi * 220 * t) + 3000 * np.sin(2 * np.pi * 3100 * t)) + 800 * rng.standard_normal(n)
    right = 7000 * np.sin(2 * np.pi * 330 * t + 0.3) + 800 * rng.standard_normal(n)
    return np.stack([left, right], axis=1).round().clip(-32768, 32767).astype(np.int16)


def _stats(seed=SEED):
    rng = np.random.default_rng(seed)
    return {"audio_mean": np.array([0.003, -0.001]), "audio_std_flat": np.array([0.21]),
            "code_mean": rng.standard_normal(256), "code_std": 0.5 + rng.random(256),
            "pose_mean": rng.standard_normal(104), "pose_std": 0.5 + rng.random(104)}


_MODELS = {}


def _models(dev, precision):
    """2-layer face and body models (ddim10) with native front ends, the body with its guide transformer; batch capacity 8."""
    if precision in _MODELS:
        return _MODELS[precision]
    from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from audio2photoreal_amd.model.guide import GuideTransformer
    from audio2photoreal_amd.model.vqvae import TemporalVertexCodec
    from audio2photoreal_amd.model_util import create_model_and_diffusion, default_args, load_model
    from audio2photoreal_amd.spec import GuideSpec, TokenizerSpec, face_spec, pose_spec
    from audio2photoreal_amd.synthetic import (synthetic_frontend_state_dict, synthetic_guide_state_dict, synthetic_state_dict,
                                               synthetic_tokenizer_state_dict)
    gs, ts = GuideSpec(), TokenizerSpec()
    guide = GuideTransformer(tokens=gs.tokens, num_layers=gs.num_layers, dim=gs.dim, emb_len=gs.emb_len,
                             num_audio_layers=gs.num_audio_layers, max_batch=MAX_BATCH, max_positions=96)
    guide.load_state_dict(synthetic_guide_state_dict(gs, SEED), strict=False)
    tok = TemporalVertexCodec(ts.n_vertices, ts.latent_dim, ts.categories, ts.residual_depth)
    tok.load_state_dict(synthetic_tokenizer_state_dict(ts, SEED), strict=False)
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


def _window_y(fmt, model, plan, R, dev, seed=SEED):
    """Window conditioning from random features: cond_embed [R*W, 1998, cond] (the token count of a 600-frame window)."""
    from audio2photoreal_amd.synthetic import cond_tokens_for_frames
    B = R * plan.W
    g = torch.Generator().manual_seed(seed)
    n_tok = cond_tokens_for_frames(plan.T_w)
    y = {"cond_embed": torch.randn(B, n_tok, model.model.cond_feature_dim, generator=g).to(dev),
         "scale": torch.full((B,), 10.0 if fmt == "face" else 2.0, device=dev)}
    if fmt == "pose":
        y["keyframes"] = torch.randn(B, len(range(plan.T_w)[::30]), 104, generator=g).to(dev)
        y["mask"] = torch.ones(B, 1, 1, plan.T_w, dtype=torch.bool, device=dev)
    return y


def _noise(R, Cf, T, seed=SEED):
    return torch.randn(R, Cf, 1, T, generator=torch.Generator().manual_seed(seed))


# ---------------------------------------------------------------------------------------------- 1. one window is the existing path

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_one_window_is_ddim_sample_loop(dev, fmt, precision):
    model, diff = _models(dev, precision)[fmt]
    plan = plan_windows(600)
    assert plan.W == 1
    R, Cf = 2, model.nfeats
    y = _window_y(fmt, model, plan, R, dev)
    noise = _noise(R, Cf, 600).to(dev)
    got = windowed_sample_loop(diff, model, plan, R, y, noise)
    want = diff.ddim_sample_loop(model, (R, Cf, 1, 600), noise=noise, clip_denoised=False, model_kwargs={"y": y})
    assert got.shape == (R, Cf, 1, 600) and torch.equal(got, want)


@pytest.mark.parametrize("precision", PRECISIONS)
def test_one_window_is_generate_from_recording(dev, precision):
    ms = _models(dev, precision)
    face, pose = ms["face"], ms["pose"]
    wav, stats = _recording(12.5), _stats()
    long = generate_from_long_recording(face, pose, stats, wav, SR, num_repetitions=2, seed=SEED)
    short = generate_from_recording(face, pose, stats, wav, SR, num_repetitions=2, seed=SEED)
    assert long["T"] == short["T"] == 360 and long["window_starts"] == [0]
    assert long["keyframes"].shape == (2, 1, 12, 104)
    for k in ("face", "pose", "audio"):
        assert np.array_equal(long[k], short[k]), k
    assert np.array_equal(long["keyframes"][:, 0], short["keyframes"])


# ---------------------------------------------------------------------------------------------- 2. the tail against a restatement

def _restated_step(mo_cfg, x_win, noise_g, plan, R, tab, t, sampler, eta):
    """float32 torch: blend the per-window guided outputs [R*W, T_w, C] over the covering windows in ascending w, then the update."""
    Cf, T = x_win.shape[1], plan.T_total
    x0 = torch.zeros(R, Cf, T, dtype=torch.float32)
    xg = torch.zeros(R, Cf, T, dtype=torch.float32)
    first = torch.zeros(T, dtype=torch.bool)
    mo = mo_cfg.view(R, plan.W, plan.T_w, Cf).permute(0, 1, 3, 2)            # [R, W, C, T_w]
    xw = x_win.view(R, plan.W, Cf, plan.T_w)
    wts = torch.from_numpy(plan.weights)
    for w, s in enumerate(plan.starts):
        x0[:, :, s:s + plan.T_w] += wts[w] * mo[:, w]
        new = ~first[s:s + plan.T_w]
        xg[:, :, s:s + plan.T_w][:, :, new] = xw[:, w][:, :, new]              # x from the first covering window
        first[s:s + plan.T_w] = True
    T_ = lambda name: float(tab[_lib.TABLE_NAMES.index(name), t])
    nz = 0.0 if t == 0 else 1.0
    if sampler == _lib.SAMPLER_DDIM:
        eps = (T_("sqrt_recip_alphas_cumprod") * xg - x0) / T_("sqrt_recipm1_alphas_cumprod")
        ab, abp = T_("alphas_cumprod"), T_("alphas_cumprod_prev")
        sigma = eta * np.sqrt((1 - abp) / (1 - ab)) * np.sqrt(1 - ab / abp)
        xn = x0 * np.sqrt(abp) + np.sqrt(1 - abp - sigma ** 2) * eps + nz * sigma * noise_g
    else:
        mean = T_("posterior_mean_coef1") * x0 + T_("posterior_mean_coef2") * xg
        xn = mean + nz * np.exp(0.5 * T_("posterior_log_variance_clipped")) * noise_g
    return xn, x0


def _rel(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_windowed_tail_vs_restatement(dev, fmt, precision):
    model, diff = _models(dev, precision)[fmt]
    plan = plan_windows(1200)
    R, Cf = 2, model.nfeats
    B = R * plan.W
    y = _window_y(fmt, model, plan, R, dev)
    x_g = _noise(R, Cf, 1200).to(dev)
    x_win = window_gather(x_g, plan, channels_first=True)
    noise_g = _noise(R, Cf, 1200, seed=SEED + 1)
    tab = diff._tables(dev)
    tmap = diff._timestep_map_tensor(dev)
    starts = (C.c_int32 * plan.W)(*plan.starts)
    weights = torch.from_numpy(plan.weights).to(dev)
    for step in (7, 0):
        t = torch.full((B,), step, dtype=torch.int64, device=dev)
        mo = model(x_win, tmap[t], y).cpu()                                       # guided forward per window [B, T_w, C]
        for sampler, eta in ((_lib.SAMPLER_DDIM, 0.0), (_lib.SAMPLER_DDIM, 0.5), (_lib.SAMPLER_DDPM, 0.0)):
            nz = None if (sampler == _lib.SAMPLER_DDIM and eta == 0.0) else noise_g.to(dev)
            xn_w, x0_w, xn_g, x0_g = model.a2p_sample_step_windowed(sampler, x_win, t, tmap, tab, y, nz, eta, False, starts, weights, 1200)
            want_xn, want_x0 = _restated_step(mo, x_win.cpu(), noise_g.squeeze(2), plan, R, tab.cpu(), step, sampler, eta)
            assert _rel(x0_g.squeeze(2).cpu(), want_x0) <= 1e-6
            assert _rel(xn_g.squeeze(2).cpu(), want_xn) <= 1e-6, (sampler, eta, step)
            assert torch.equal(window_gather(xn_g, plan, channels_first=True), xn_w)
            assert torch.equal(window_gather(x0_g, plan, channels_first=True), x0_w)
    model.model.check_finite()


# ---------------------------------------------------------------------------------------------- 3. the consistency invariant

def _assert_consistent(win, glob, plan):
    """Every window copy of every frame equals the global tensor (hence the copies of a shared frame are bit-identical)."""
    R = glob.shape[0]
    wv = win.view(R, plan.W, win.shape[1], plan.T_w)
    for w, s in enumerate(plan.starts):
        a, b = wv[:, w], glob[:, :, 0, s:s + plan.T_w]
        assert torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32)), f"window {w}"


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("fmt", FORMATS)
@pytest.mark.parametrize("T_total", [1800, 1110])
def test_consistency_after_every_step(dev, fmt, precision, T_total):
    model, diff = _models(dev, precision)[fmt]
    plan = plan_windows(T_total)
    if T_total == 1110:
        cover = np.zeros(T_total, int)
        for s in plan.starts:
            cover[s:s + plan.T_w] += 1
        assert cover.max() == 3
    R = MAX_BATCH // plan.W
    Cf = model.nfeats
    y = _window_y(fmt, model, plan, R, dev)
    noise = _noise(R, Cf, T_total).to(dev)
    n = diff.num_timesteps
    step_noise = [_noise(R, Cf, T_total, seed=100 + i).to(dev) for i in range(n)]
    tab, tmap = diff._tables(dev), diff._timestep_map_tensor(dev)
    starts = (C.c_int32 * plan.W)(*plan.starts)
    weights = torch.from_numpy(plan.weights).to(dev)
    x = window_gather(noise, plan, channels_first=True)
    for k, i in enumerate(reversed(range(n))):
        t = torch.full((R * plan.W,), i, dtype=torch.int64, device=dev)
        x, x0, xg, x0g = model.a2p_sample_step_windowed(_lib.SAMPLER_DDIM, x, t, tmap, tab, y, step_noise[k], 0.5, False, starts,
                                                        weights, T_total)
        _assert_consistent(x, xg, plan)
        _assert_consistent(x0, x0g, plan)
    assert torch.isfinite(x0g).all()
    # the loop drives the same steps
    got = windowed_sample_loop(diff, model, plan, R, y, noise, eta=0.5, step_noise=step_noise)
    assert torch.equal(got, x0g)


# ---------------------------------------------------------------------------------------------- 4. slicing

def test_window_gather_is_slicing(dev):
    wav, stats = _recording(61.0), _stats()
    rec = prepare_long_recording(wav, SR, stats, 2, seed=SEED, device=dev, max_batch=MAX_BATCH)
    plan = rec.plan
    assert rec.T == 1800 and plan.W == 4 and tuple(rec.windows.shape) == (8, 960000, 2)
    for r in range(2):
        for w, s in enumerate(plan.starts):
            assert torch.equal(rec.windows[r * plan.W + w], rec.audio[r, s * 1600:(s + plan.T_w) * 1600])
    # the global audio is prepare_recording's over the whole recording (global peak normalisation, one partner-noise draw)
    assert torch.equal(rec.audio, prepare_recording(wav, SR, stats, 2, seed=SEED, device=dev, max_frames=1800).audio)
    noise = _noise(3, 104, 1110).to(dev)
    p3 = plan_windows(1110)
    win = window_gather(noise, p3, channels_first=True)
    assert tuple(win.shape) == (9, 104, 1, 600)
    for r in range(3):
        for w, s in enumerate(p3.starts):
            assert torch.equal(win[r * p3.W + w], noise[r, :, :, s:s + 600])


# ---------------------------------------------------------------------------------------------- 5. end to end

@pytest.mark.parametrize("precision", PRECISIONS)
def test_sixty_seconds_end_to_end(dev, precision):
    ms = _models(dev, precision)
    face, pose = ms["face"], ms["pose"]
    wav, stats = _recording(61.0), _stats()
    run = lambda **kw: generate_from_long_recording(face, pose, stats, wav, SR, **{"num_repetitions": 2, "seed": SEED, **kw})
    ov = run(overlap=True)
    assert ov["T"] == 1800 and ov["window_starts"] == plan_windows(1800).starts
    assert ov["face"].shape == (2, 1800, 256) and ov["pose"].shape == (2, 1800, 104) and ov["keyframes"].shape == (2, 4, 20, 104)
    assert all(np.isfinite(ov[k]).all() for k in ("face", "pose", "keyframes"))
    seq = run(overlap=False)
    assert all(np.array_equal(ov[k], seq[k]) for k in ("face", "pose", "keyframes")), "the two-stream schedule changed the samples"
    again = run(overlap=True)
    assert all(np.array_equal(ov[k], again[k]) for k in ("face", "pose", "keyframes")), "same seed, different samples"
    other = run(overlap=False, seed=SEED + 1)
    assert not np.array_equal(other["face"], ov["face"]) and not np.array_equal(other["pose"], ov["pose"])
    # the windows' keyframes are predicted independently: window 0 draws what generate_from_recording draws for its first 20 s
    assert not np.array_equal(ov["keyframes"][:, 0], ov["keyframes"][:, 1])
