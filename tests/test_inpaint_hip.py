"""Sampling with held elements on the MI355X (sample/inpaint.py, csrc/kernels_inpaint.h): an all-false mask is the plain fused step
bit for bit, one step against a float32 restatement from the guided forward, held elements through whole DDIM / DDPM loops,
clip continuation and segment re-rolls."""
import numpy as np
import pytest
import torch

from audio2photoreal_amd import _lib
from audio2photoreal_amd.sample import inpaint
from audio2photoreal_amd.sample.inpaint import expand_mask, inpaint_sample_loop
from audio2photoreal_amd.sample.recording import continue_recording, generate_from_recording, regenerate_segment

pytestmark = pytest.mark.gpu
SEED = 10
SR = 44100
MAX_BATCH = 8
PRECISIONS = ["fp32", "fp16"]
FORMATS = ["face", "pose"]
T = 240


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


def _y(fmt, model, B, T, dev, seed=SEED):
    from audio2photoreal_amd.synthetic import cond_tokens_for_frames
    g = torch.Generator().manual_seed(seed)
    y = {"cond_embed": torch.randn(B, cond_tokens_for_frames(T), model.model.cond_feature_dim, generator=g).to(dev),
         "scale": torch.full((B,), 10.0 if fmt == "face" else 2.0, device=dev)}
    if fmt == "pose":
        y["keyframes"] = torch.randn(B, len(range(T)[::30]), 104, generator=g).to(dev)
        y["mask"] = torch.ones(B, 1, 1, T, dtype=torch.bool, device=dev)
    return y


def _randn(*shape, seed=SEED, scale=1.0):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale


def _masks(B, Cf, T):
    """A frame mask (the first 60 frames and frames 150..179 held) and a channel-subset mask (every third channel, frames >= 90)."""
    frames = torch.zeros(B, T, dtype=torch.bool)
    frames[:, :60] = True
    frames[:, 150:180] = True
    chans = torch.zeros(B, Cf, 1, T, dtype=torch.bool)
    chans[:, ::3, :, 90:] = True
    return {"frames": frames, "channels": chans}


STEP_CASES = [(_lib.SAMPLER_DDIM, 0.0, False), (_lib.SAMPLER_DDIM, 0.5, True), (_lib.SAMPLER_DDPM, 0.0, False),
              (_lib.SAMPLER_DDIM, 0.0, True), (_lib.SAMPLER_DDIM, 0.5, False), (_lib.SAMPLER_DDPM, 0.0, True)]


# ---------------------------------------------------------------------------------------------- 1. all-false mask = plain step

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_all_false_mask_is_the_plain_step(dev, fmt, precision):
    model, diff = _models(dev, precision)[fmt]
    B, Cf = 2, model.nfeats
    y = _y(fmt, model, B, T, dev)
    x = _randn(B, Cf, 1, T).to(dev)
    noise = _randn(B, Cf, 1, T, seed=SEED + 1).to(dev)
    known = _randn(B, Cf, 1, T, seed=SEED + 2, scale=3.0).to(dev)
    none = expand_mask(torch.zeros(B, T, dtype=torch.bool, device=dev), B, Cf, T)
    tab, tmap = diff._tables(dev), diff._timestep_map_tensor(dev)
    for step in (7, 0):
        t = torch.full((B,), step, dtype=torch.int64, device=dev)
        for sampler, eta, clip in STEP_CASES:
            nz = None if (sampler == _lib.SAMPLER_DDIM and eta == 0.0) else noise
            want = model.a2p_sample_step(sampler, x, t, tmap, tab, y, nz, eta, clip)
            got = model.a2p_sample_step_inpaint(sampler, x, t, tmap, tab, y, nz, eta, clip, known, none)
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]), (step, sampler, eta, clip)
    model.model.check_finite()


# ---------------------------------------------------------------------------------------------- 2. one step against a restatement

def _fma32(a, b, c):
    """float32 fma(a, b, c) of float32 arrays, correctly rounded: the float64 product is exact, the float64 sum is rounded to odd
    (then the cast to float32 rounds once, 53 >= 24 + 2)."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c = np.broadcast_to(np.asarray(c, np.float32), p.shape).astype(np.float64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    even = (s.view(np.int64) & 1) == 0
    s = np.where((e != 0) & even, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
    return s.astype(np.float32)


def _restated_step(g, x, known, mask, noise, tab, t, sampler, eta, clip):
    """float32 numpy, in the operation order of kernels_misc.h ddim_update / ddpm_update (its fused multiply-adds as fma32).
    g: the guided model output moved to [B, C, T]; DDPM is restated with zero noise (the kernel's noise term is then + 0)."""
    f = np.float32
    x0 = np.clip(g, f(-1), f(1)) if clip else g.copy()
    x0 = np.where(mask, known, x0)
    T_ = lambda name: f(tab[_lib.TABLE_NAMES.index(name), t])
    if sampler == _lib.SAMPLER_DDIM:
        eps = _fma32(np.broadcast_to(T_("sqrt_recip_alphas_cumprod"), x.shape), x, -x0) / T_("sqrt_recipm1_alphas_cumprod")
        ab, abp = T_("alphas_cumprod"), T_("alphas_cumprod_prev")
        sigma = f(f(eta) * np.sqrt(f(f(1) - abp) / f(f(1) - ab))) * np.sqrt(f(f(1) - f(ab / abp)))
        s2 = np.sqrt(_fma32(np.array([-sigma], f), np.array([sigma], f), f(f(1) - abp))[0])
        mean = x0 * np.sqrt(abp) + s2 * eps
        nzs = f(f(1.0 if t != 0 else 0.0) * sigma)
        xn = _fma32(noise, np.broadcast_to(nzs, noise.shape), mean) if noise is not None else mean + f(0) * nzs
    else:
        xn = T_("posterior_mean_coef1") * x0 + T_("posterior_mean_coef2") * x
    return xn.astype(f), x0.astype(f)


def _step_in_place(model, sampler, x, t, tmap, tab, y, noise, eta, clip, known, mask_u8):
    """a2p_sample_step_inpaint with x_next = x (the documented alias); returns pred_xstart."""
    fm = model.model
    fm.prepare(x, y)
    x0 = torch.empty_like(x)
    sc = y["scale"].to(torch.float32).contiguous()
    with _lib.on_device_of(x):
        _lib.check(fm._lib().a2p_sample_step_inpaint(fm._ctx, sampler, _lib.ptr(x), _lib.ptr(t), _lib.ptr(tmap), _lib.ptr(tab),
                                                     tab.shape[1], _lib.ptr(sc), _lib.ptr(noise), float(eta), int(clip),
                                                     _lib.ptr(known), _lib.ptr(mask_u8), _lib.ptr(x), _lib.ptr(x0),
                                                     _lib.current_stream(x.device)), "a2p_sample_step_inpaint")
    return x0


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_step_vs_restatement(dev, fmt, precision):
    model, diff = _models(dev, precision)[fmt]
    B, Cf = 2, model.nfeats
    y = _y(fmt, model, B, T, dev)
    x_in = _randn(B, Cf, 1, T).to(dev)
    noise = _randn(B, Cf, 1, T, seed=SEED + 1).to(dev)
    known = _randn(B, Cf, 1, T, seed=SEED + 2, scale=3.0).to(dev)       # held values beyond [-1, 1]: they are not clamped
    tab, tmap = diff._tables(dev), diff._timestep_map_tensor(dev)
    tab_h = tab.cpu().numpy()
    for kind, m in _masks(B, Cf, T).items():
        mask_u8 = expand_mask(m.to(dev), B, Cf, T)
        mask_h = mask_u8.squeeze(2).cpu().numpy().astype(bool)
        for step in (7, 0):
            t = torch.full((B,), step, dtype=torch.int64, device=dev)
            g = model(x_in, tmap[t], y).cpu().numpy().transpose(0, 2, 1)                 # guided forward [B, T, C] -> [B, C, T]
            for sampler, eta, clip in STEP_CASES:
                if sampler == _lib.SAMPLER_DDPM:
                    nz = torch.zeros_like(noise)
                else:
                    nz = None if eta == 0.0 else noise
                x = x_in.clone()
                x0 = _step_in_place(model, sampler, x, t, tmap, tab, y, nz, eta, clip, known, mask_u8)
                want_xn, want_x0 = _restated_step(g, x_in.squeeze(2).cpu().numpy(), known.squeeze(2).cpu().numpy(), mask_h,
                                                  None if nz is None else nz.squeeze(2).cpu().numpy(), tab_h, step, sampler, eta, clip)
                case = (kind, step, sampler, eta, clip)
                assert torch.equal(x0.squeeze(2).cpu(), torch.from_numpy(want_x0)), case
                assert torch.equal(x.squeeze(2).cpu(), torch.from_numpy(want_xn)), case
                held = torch.from_numpy(mask_h)
                assert torch.equal(x0.squeeze(2).cpu()[held], known.squeeze(2).cpu()[held]), case
    model.model.check_finite()


# ---------------------------------------------------------------------------------------------- 3./4. whole loops

@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_loop_holds_known_elements(dev, fmt, precision):
    model, diff = _models(dev, precision)[fmt]
    B, Cf = 2, model.nfeats
    y = _y(fmt, model, B, T, dev)
    noise = _randn(B, Cf, 1, T).to(dev)
    known = _randn(B, Cf, 1, T, seed=SEED + 2).to(dev)
    n = diff.num_timesteps
    step_noise = [_randn(B, Cf, 1, T, seed=100 + i).to(dev) for i in range(n)]
    tab = diff._tables(dev).cpu()
    assert float(tab[_lib.TABLE_NAMES.index("posterior_mean_coef1"), 0]) == 1.0     # DDPM's last step: mean = x0 exactly
    assert float(tab[_lib.TABLE_NAMES.index("posterior_mean_coef2"), 0]) == 0.0
    for kind, m in _masks(B, Cf, T).items():
        held = expand_mask(m, B, Cf, T).bool()
        m = m.to(dev)
        for sampler in ("ddim", "ddpm"):
            got = inpaint_sample_loop(diff, model, y, known, m, noise, sampler=sampler, step_noise=step_noise)
            if sampler == "ddim":
                plain = diff.ddim_sample_loop(model, (B, Cf, 1, T), noise=noise, clip_denoised=False, model_kwargs={"y": y},
                                              step_noise=step_noise)
            else:
                plain = diff.p_sample_loop(model, (B, Cf, 1, T), noise=noise, clip_denoised=False, model_kwargs={"y": y},
                                           step_noise=step_noise)
            got, plain = got.cpu(), plain.cpu()
            assert torch.isfinite(got).all()
            assert torch.equal(got[held], known.cpu()[held]), (kind, sampler)
            assert not torch.equal(got[~held], plain[~held]), (kind, sampler)      # the held values steer the rest of the clip
            assert torch.equal(got, inpaint_sample_loop(diff, model, y, known, m, noise, sampler=sampler, step_noise=step_noise).cpu())


@pytest.mark.parametrize("precision", PRECISIONS)
@pytest.mark.parametrize("fmt", FORMATS)
def test_all_true_mask_returns_known(dev, fmt, precision):
    model, diff = _models(dev, precision)[fmt]
    B, Cf = 2, model.nfeats
    y = _y(fmt, model, B, T, dev)
    noise = _randn(B, Cf, 1, T).to(dev)
    known = _randn(B, Cf, 1, T, seed=SEED + 2).to(dev)
    for mask in (torch.ones(B, T, dtype=torch.bool, device=dev), torch.ones(B, 1, 1, T, dtype=torch.bool, device=dev)):
        for sampler in ("ddim", "ddpm"):
            got = inpaint_sample_loop(diff, model, y, known, mask, noise, sampler=sampler, eta=0.5)
            assert torch.equal(got, known), sampler


# ---------------------------------------------------------------------------------------------- 5. continue_recording

def _norm(values, mean, std):
    return torch.from_numpy(((np.asarray(values, np.float64) - mean) / std).astype(np.float32).transpose(0, 2, 1).copy())


@pytest.mark.parametrize("precision", PRECISIONS)
def test_continue_recording(dev, precision, monkeypatch):
    ms = _models(dev, precision)
    face, pose = ms["face"], ms["pose"]
    stats = _stats()
    first = generate_from_recording(face, pose, stats, _recording(8.2), SR, num_repetitions=2, seed=SEED)
    assert first["T"] == 240
    calls = []
    loop = inpaint.inpaint_sample_loop

    def spy(diffusion, model, y, known, known_mask, noise, **kw):
        out = loop(diffusion, model, y, known, known_mask, noise, **kw)
        calls.append((model.nfeats, known.cpu(), known_mask.cpu(), out.cpu()))
        return out
    monkeypatch.setattr(inpaint, "inpaint_sample_loop", spy)

    chunks = [_recording(4.2, seed=8), _recording(4.1, sr=22050, seed=9)]
    prev, clip = first, first
    for k, wav in enumerate(chunks):
        calls.clear()
        run = lambda **kw: continue_recording(face, pose, stats, wav, 44100 if k == 0 else 22050, prev,
                                              **{"context_frames": 120, "seed": SEED + k, **kw})
        out = run(overlap=True)
        assert out["T"] == 120 and out["context"] == 120 and out["sr"] == 48000
        assert out["face"].shape == (2, 120, 256) and out["pose"].shape == (2, 120, 104) and out["keyframes"].shape == (2, 4, 104)
        assert out["audio"].shape == (2, 120 * 1600)
        assert all(np.isfinite(out[k_]).all() for k_ in ("face", "pose", "keyframes"))
        # the held frames of the window are the previous clip's last 120 frames, normalised, bit for bit
        assert sorted(c[0] for c in calls) == [104, 256]
        for nf, known, mask, window in calls:
            assert window.shape == (2, nf, 1, 240) and tuple(mask.shape) == (2, 240) and mask[:, :120].all() and not mask[:, 120:].any()
            mean, std, prev_vals = ((stats["code_mean"], stats["code_std"], prev["face"]) if nf == 256 else
                                    (stats["pose_mean"], stats["pose_std"], prev["pose"]))
            want = _norm(prev_vals[:, -120:], mean, std)
            assert torch.equal(window[:, :, 0, :120], want) and torch.equal(known[:, :, 0, :120], want)
        calls.clear()
        seq = run(overlap=False)
        again = run(overlap=True)
        other = run(overlap=True, seed=SEED + 50)
        for key in ("face", "pose", "keyframes"):
            assert np.array_equal(out[key], seq[key]), f"overlap changed {key}"
            assert np.array_equal(out[key], again[key]), f"same seed, different {key}"
        assert not np.array_equal(other["face"], out["face"]) and not np.array_equal(other["pose"], out["pose"])
        clip = {key: np.concatenate([clip[key], out[key]], axis=1) for key in ("face", "pose")}
        prev = out
    assert clip["face"].shape == (2, 480, 256) and clip["pose"].shape == (2, 480, 104)


# ---------------------------------------------------------------------------------------------- 6. regenerate_segment

@pytest.mark.parametrize("precision", PRECISIONS)
def test_regenerate_segment(dev, precision):
    ms = _models(dev, precision)
    face, pose = ms["face"], ms["pose"]
    stats = _stats()
    res = generate_from_recording(face, pose, stats, _recording(8.2), SR, num_repetitions=2, seed=SEED)
    s, e = 90, 180
    for parts in (("face", "pose"), ("face",), ("pose",)):
        out = regenerate_segment(face, pose, stats, res, s, e, parts=parts, seed=SEED + 3)
        assert out["T"] == res["T"] and np.array_equal(out["audio"], res["audio"])
        for key in ("face", "pose"):
            if key in parts:
                assert np.array_equal(out[key][:, :s], res[key][:, :s]) and np.array_equal(out[key][:, e:], res[key][:, e:]), key
                assert not np.array_equal(out[key][:, s:e], res[key][:, s:e]), key
                assert np.isfinite(out[key]).all()
            else:
                assert np.array_equal(out[key], res[key]), key
        if "pose" in parts:
            assert np.array_equal(out["keyframes"][:, :s // 30], res["keyframes"][:, :s // 30])
            assert np.array_equal(out["keyframes"][:, e // 30:], res["keyframes"][:, e // 30:])
        else:
            assert np.array_equal(out["keyframes"], res["keyframes"])
    again = regenerate_segment(face, pose, stats, res, s, e, seed=SEED + 3)
    assert np.array_equal(again["face"], regenerate_segment(face, pose, stats, res, s, e, seed=SEED + 3, overlap=False)["face"])
