"""Recording -> motion on the MI355X: `resample` (csrc/kernels_audio.h) against a float64 restatement of torchaudio's resampler,
`prepare_recording` against the demo's arithmetic (demo/demo.py:159-186), and `generate_from_recording` against itself under
every schedule and against the building blocks driven by hand."""
import math

import numpy as np
import pytest
import torch

import torchaudio_restatement as TA
from audio2photoreal_amd import _lib
from audio2photoreal_amd.audio import _resample_rows, resample
from audio2photoreal_amd.sample.recording import generate_from_recording, prepare_recording

pytestmark = pytest.mark.gpu
SEED = 10
SR = 44100
RATES = [(44100, 48000), (22050, 48000), (16000, 48000), (11025, 48000), (8000, 48000), (96000, 48000), (48000, 16000)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


def _check_close(got, want):
    got = np.asarray(got, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    rel = np.linalg.norm(got - want) / np.linalg.norm(want)
    mx = np.abs(got - want).max() / np.abs(want).max()
    assert rel <= 1e-6 and mx <= 1e-5, (rel, mx)
    return rel, mx


@pytest.mark.parametrize("L", [4097, 30001])
@pytest.mark.parametrize("orig,new", RATES)
def test_resample_vs_restatement(dev, orig, new, L):
    """Batched rows of odd length; the functional form's float32 table (default) and the float64 one of transforms.Resample,
    each against the same table applied in float64."""
    x = torch.from_numpy(np.random.default_rng(orig + L).standard_normal((3, L)).astype(np.float32))
    for kernel_dtype, np_dtype in ((None, np.float32), (torch.float64, np.float64)):
        got = resample(x.to(dev), orig, new, kernel_dtype=kernel_dtype)
        g = math.gcd(orig, new)
        assert got.shape == (3, -(-(new // g) * L // (orig // g)))                 # ceil(n L / o)
        _check_close(got.cpu().numpy(), TA.resample(x.numpy(), orig, new, dtype=np_dtype))


def test_resample_kaiser_identity_and_leading_dims(dev):
    x = torch.from_numpy(np.random.default_rng(1).standard_normal((2, 2, 5001)).astype(np.float32))
    got = resample(x.to(dev), 44100, 48000, resampling_method="sinc_interp_kaiser", kernel_dtype=torch.float64)
    assert got.shape == (2, 2, -(-160 * 5001 // 147))                       # ceil(n L / o), 44.1 -> 48 kHz: o = 147, n = 160
    _check_close(got.cpu().numpy(), TA.resample(x.numpy(), 44100, 48000, kaiser=True))
    xd = x.to(dev)
    assert resample(xd, 48000, 48000) is xd
    # equal rates with the channel average: the averaged input itself
    st = torch.from_numpy(np.random.default_rng(2).standard_normal((777, 2)).astype(np.float32)).to(dev)
    assert torch.equal(_resample_rows(st.contiguous(), 777, 2, 48000, 48000)[0], st.mean(dim=1))


def test_resample_matches_the_frontend_oracle(dev):
    """oracle.frontend_oracle.resample_sinc = transforms.Resample(48000, 16000): its float64-built table is the float64 rule."""
    from oracle.frontend_oracle import resample_sinc
    x = torch.from_numpy(np.random.default_rng(3).standard_normal((2, 48001)).astype(np.float32))
    want = resample_sinc(x).double().numpy()
    _check_close(resample(x.to(dev), 48000, 16000, kernel_dtype=torch.float64).cpu().numpy(), want)


def _recording(seconds=8.3, sr=SR):
    """A synthetic stereo int16 recording [L, 2]: two tones + noise, different per channel."""
    n = int(round(seconds * sr))
    t = np.arange(n) / sr
    rng = np.random.default_rng(7)
    left = 9000 * np.sin(2 * np.pi * 220 * t) + 3000 * np.sin(2 * np.pi * 3100 * t) + 800 * rng.standard_normal(n)
    right = 7000 * np.sin(2 * np.pi * 330 * t + 0.3) + 800 * rng.standard_normal(n)
    return np.stack([left, right], axis=1).round().clip(-32768, 32767).astype(np.int16)


def _stats(seed=SEED):
    rng = np.random.default_rng(seed)
    return {"audio_mean": np.array([0.003, -0.001]), "audio_std_flat": np.array([0.21]),
            "code_mean": rng.standard_normal(256), "code_std": 0.5 + rng.random(256),
            "pose_mean": rng.standard_normal(104), "pose_std": 0.5 + rng.random(104)}


def test_prepare_recording_is_the_demo_arithmetic(dev):
    wav, stats = _recording(), _stats()
    rec = prepare_recording(wav, SR, stats, 2, seed=SEED, device=dev)
    Lc = 384000
    assert rec.T == 240 and tuple(rec.audio.shape) == (2, Lc, 2) and rec.audio.dtype == torch.float32
    # the same resampled mono signal: torch.mean over the channels, then resample -- the in-kernel average has the same bits
    x = torch.from_numpy(wav).float()
    mono = resample(x.mean(dim=1).to(dev), SR, 48000)
    assert torch.equal(mono, _resample_rows(x.to(dev).contiguous(), x.shape[0], 2, SR, 48000)[0])
    noise = np.random.RandomState(SEED).normal(0, 0.001, (1, Lc, 2))
    want, dual = TA.dual_audio(mono[:Lc].cpu().numpy(), noise, stats["audio_mean"], stats["audio_std_flat"], 2)
    got = rec.audio.cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), "y['audio'] differs from the demo's arithmetic"
    un = dual * stats["audio_std_flat"] + stats["audio_mean"]
    assert rec.dual_audio.dtype == np.float64 and np.array_equal(rec.dual_audio, un[0].T)
    # channels-first input is averaged over dim 0 (demo: dim = 0 if shape[0] == 2): same bits
    assert torch.equal(prepare_recording(wav.T.copy(), SR, stats, 2, seed=SEED, device=dev).audio, rec.audio)
    # the whole function against the float64 restatement of the resampler (functional rule: float32 table)
    mono_ref = TA.resample(x.mean(dim=1).numpy(), SR, 48000, dtype=np.float32)[:Lc]
    ref, _ = TA.dual_audio(mono_ref.astype(np.float32), noise, stats["audio_mean"], stats["audio_std_flat"], 2)
    _check_close(got[..., 0], ref[..., 0].astype(np.float64))
    # a silent recording is refused by the library (the demo would divide by zero)
    with pytest.raises(_lib.A2PError, match="peak"):
        prepare_recording(np.zeros((SR * 5, 2), np.int16), SR, stats, 1, device=dev)


# ---------------------------------------------------------------------------------------------- face + body pipeline

def _models(dev, precision, R=2):
    from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from audio2photoreal_amd.model.guide import GuideTransformer
    from audio2photoreal_amd.model.vqvae import TemporalVertexCodec
    from audio2photoreal_amd.model_util import create_model_and_diffusion, default_args, load_model
    from audio2photoreal_amd.spec import GuideSpec, TokenizerSpec, face_spec, pose_spec
    from audio2photoreal_amd.synthetic import (synthetic_frontend_state_dict, synthetic_guide_state_dict, synthetic_state_dict,
                                               synthetic_tokenizer_state_dict)
    gs, ts = GuideSpec(), TokenizerSpec()
    guide = GuideTransformer(tokens=gs.tokens, num_layers=gs.num_layers, dim=gs.dim, emb_len=gs.emb_len,
                             num_audio_layers=gs.num_audio_layers, max_batch=R, max_positions=96)
    guide.load_state_dict(synthetic_guide_state_dict(gs, SEED), strict=False)
    tok = TemporalVertexCodec(ts.n_vertices, ts.latent_dim, ts.categories, ts.residual_depth)
    tok.load_state_dict(synthetic_tokenizer_state_dict(ts, SEED), strict=False)
    out = {}
    for fmt, spec in (("face", face_spec(num_layers=2)), ("pose", pose_spec(num_layers=2))):
        m, d = create_model_and_diffusion(default_args(fmt, layers=2, timestep_respacing="ddim5"), "test", precision=precision,
                                          max_batch=R, audio_frontend="native")
        load_model(m, {**synthetic_state_dict(spec, SEED), **synthetic_frontend_state_dict(SEED, lip=fmt == "face")})
        if fmt == "pose":
            m.setup_guide_predictor(guide.to(dev).eval(), tok.to(dev))
        out[fmt] = (ClassifierFreeSampleModel(m.to(dev).eval()), d)
    return out["face"], out["pose"]


def _by_hand(face, pose, stats, wav, R, seed, dev):
    """The same sample from the existing building blocks: shared front end, _replace_keyframes, two ddim_sample_loop calls."""
    from audio2photoreal_amd.sample.generate import _replace_keyframes
    from audio2photoreal_amd.sample_parallel import derive_seed, per_sample_noise
    (fc, fd), (pc, pd) = face, pose
    rec = prepare_recording(wav, SR, stats, R, seed=seed, device=dev)
    T, audio = rec.T, rec.audio
    with torch.no_grad():
        feats = pc.model.audio_frontend.encode_audio(audio)
        face_ce = fc.model.audio_frontend.encode_lip(audio, feats)
        u = torch.stack([torch.rand(8 * pc.tokenizer.residual_depth, generator=torch.Generator().manual_seed(derive_seed(seed, 1, r)))
                         for r in range(R)], dim=1)
        kf = _replace_keyframes({"y": {"cond_embed": feats, "keyframes": torch.zeros(R, 8, 104, device=dev)}}, pc, u, top_p=0.97).to(dev)
        y = {"cond_embed": feats, "keyframes": kf, "mask": torch.ones(R, 1, 1, T, dtype=torch.bool, device=dev),
             "scale": torch.full((R,), 2.0, device=dev)}
        body = pd.ddim_sample_loop(pc, (R, 104, 1, T), clip_denoised=False, model_kwargs={"y": y},
                                   noise=per_sample_noise((R, 104, 1, T), [derive_seed(seed, 2, r) for r in range(R)]).to(dev))
        yf = {"cond_embed": face_ce, "scale": torch.full((R,), 10.0, device=dev)}
        face_s = fd.ddim_sample_loop(fc, (R, 256, 1, T), clip_denoised=False, model_kwargs={"y": yf},
                                     noise=per_sample_noise((R, 256, 1, T), [derive_seed(seed, 3, r) for r in range(R)]).to(dev))
    return {"face": face_s.squeeze(2).cpu().numpy().transpose(0, 2, 1) * stats["code_std"] + stats["code_mean"],
            "pose": body.squeeze(2).cpu().numpy().transpose(0, 2, 1) * stats["pose_std"] + stats["pose_mean"],
            "keyframes": kf.cpu().numpy() * stats["pose_std"] + stats["pose_mean"]}


def _same(a, b, keys=("face", "pose", "keyframes")):
    return all(np.array_equal(a[k], b[k]) for k in keys)


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_generate_from_recording(dev, precision):
    from audio2photoreal_amd.sample.recording import can_share_features
    wav, stats = _recording(), _stats()
    face, pose = _models(dev, precision)
    assert can_share_features(face[0], pose[0])
    run = lambda **kw: generate_from_recording(face, pose, stats, wav, SR, **{"num_repetitions": 2, "seed": SEED, **kw})
    ov = run(overlap=True)
    assert ov["face"].shape == (2, 240, 256) and ov["pose"].shape == (2, 240, 104) and ov["keyframes"].shape == (2, 8, 104)
    assert ov["T"] == 240 and ov["sr"] == 48000 and ov["audio"].shape == (2, 384000)
    assert ov["face"].dtype == np.float64 and all(np.isfinite(ov[k]).all() for k in ("face", "pose", "keyframes"))
    seq = run(overlap=False)
    assert _same(ov, seq), "the two-stream schedule changed the samples"
    own = run(overlap=False, share_features=False)
    assert _same(own, seq), "sharing the front end's features changed the samples"
    assert _same(run(overlap=True), ov), "same seed, different samples"
    other = run(overlap=False, seed=SEED + 1)
    assert not np.array_equal(other["face"], seq["face"]) and not np.array_equal(other["pose"], seq["pose"])
    assert _same(_by_hand(face, pose, stats, wav, 2, SEED, dev), seq), "the API drifted from its building blocks"
