"""Conversations on the MI355X (sample/conversation.py, csrc/kernels_audio.h): the per-channel resampler against a2p_resample,
prepare_conversation against the float64 restatement, generate_conversation against its building blocks driven by hand, swap
symmetry, the batching and stream rules, and a partner who is heard but not animated."""
import numpy as np
import pytest
import torch

from audio2photoreal_amd import _lib
from audio2photoreal_amd.audio import _resample_rows
from audio2photoreal_amd.sample.conversation import generate_conversation, person_seeds, prepare_conversation
from audio2photoreal_amd.sample.generate import _replace_keyframes
from audio2photoreal_amd.sample.long_form import plan_windows, window_gather, windowed_sample_loop
from audio2photoreal_amd.sample_parallel import derive_seed, per_sample_noise
from tests.conversation_restatement import conversation_audio, person_audio
from tests.test_long_form_hip import MAX_BATCH, SEED, _models, _recording, _stats

pytestmark = pytest.mark.gpu
SR = 44100
KEYS = ("face", "pose", "keyframes")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


_OTHER = {}


def _other_models(dev):
    """A second fp32 model set (other synthetic weights): person B of the asymmetric cases."""
    if "fp32" in _OTHER:
        return _OTHER["fp32"]
    from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel
    from audio2photoreal_amd.model.guide import GuideTransformer
    from audio2photoreal_amd.model.vqvae import TemporalVertexCodec
    from audio2photoreal_amd.model_util import create_model_and_diffusion, default_args, load_model
    from audio2photoreal_amd.spec import GuideSpec, TokenizerSpec, face_spec, pose_spec
    from audio2photoreal_amd.synthetic import (synthetic_frontend_state_dict, synthetic_guide_state_dict, synthetic_state_dict,
                                               synthetic_tokenizer_state_dict)
    s = SEED + 1
    gs, ts = GuideSpec(), TokenizerSpec()
    guide = GuideTransformer(tokens=gs.tokens, num_layers=gs.num_layers, dim=gs.dim, emb_len=gs.emb_len,
                             num_audio_layers=gs.num_audio_layers, max_batch=MAX_BATCH, max_positions=96)
    guide.load_state_dict(synthetic_guide_state_dict(gs, s), strict=False)
    tok = TemporalVertexCodec(ts.n_vertices, ts.latent_dim, ts.categories, ts.residual_depth)
    tok.load_state_dict(synthetic_tokenizer_state_dict(ts, s), strict=False)
    out = {}
    for fmt, spec in (("face", face_spec(num_layers=2)), ("pose", pose_spec(num_layers=2))):
        m, d = create_model_and_diffusion(default_args(fmt, layers=2, timestep_respacing="ddim10"), "test", precision="fp32",
                                          max_batch=MAX_BATCH, audio_frontend="native")
        load_model(m, {**synthetic_state_dict(spec, s), **synthetic_frontend_state_dict(s, lip=fmt == "face")})
        if fmt == "pose":
            m.setup_guide_predictor(guide.to(dev).eval(), tok.to(dev))
        out[fmt] = (ClassifierFreeSampleModel(m.to(dev).eval()), d)
    _OTHER["fp32"] = out
    return out


def _stats_b():
    st = _stats(SEED + 3)
    st["audio_mean"], st["audio_std_flat"] = np.array([-0.002, 0.004]), np.array([0.17])
    return st


def _person(ms, stats):
    return (ms["face"], ms["pose"], stats)


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in KEYS) and np.array_equal(a["audio"], b["audio"])


def _rel(a, b):
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def _channels(wav, sr, dev):
    """Each channel resampled on its own by a2p_resample (the mono path): fp32 [2, Lr]."""
    x = torch.from_numpy(np.ascontiguousarray(np.asarray(wav, np.float32))).to(dev)
    return torch.cat([_resample_rows(x[:, c].contiguous(), x.shape[0], 1, sr, 48000) for c in range(2)])


# ---------------------------------------------------------------------------------------------- kernels

@pytest.mark.parametrize("sr", [44100, 16000, 48000])
def test_resample_channels_is_a2p_resample_per_channel(dev, sr):
    from audio2photoreal_amd.audio import _device_table, resampled_length
    wav = _recording(4.3, sr=sr).astype(np.float32)
    L = wav.shape[0]
    Lr = resampled_length(L, sr, 48000)
    x = torch.from_numpy(wav).to(dev)
    out = torch.full((2, Lr), float("nan"), device=dev)
    table, width, n_phase, n_taps = None, 0, 0, 0
    if sr != 48000:
        table, width = _device_table(sr, 48000, 6, 0.99, "sinc_interp_hann", None, torch.float32, dev)
        n_phase, n_taps = table.shape
    _lib.check(_lib.load().a2p_resample_channels(_lib.ptr(x), L, 2, sr, 48000, _lib.ptr(table), n_phase, n_taps, width, _lib.ptr(out),
                                                 _lib.current_stream(dev)), "a2p_resample_channels")
    want = _channels(wav, sr, dev)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("R", [1, 3])
@pytest.mark.parametrize("normalize", ["peak", "none"])
def test_prepare_conversation_vs_restatement(dev, normalize, R):
    wav = _recording(9.0)
    if normalize == "none":
        wav = wav.astype(np.float32) / 32768.0            # int PCM to [-1, 1]
    stats = (_stats(), _stats_b())
    prep = prepare_conversation(wav, SR, stats, R, normalize=normalize, device=dev)
    assert prep.T == 240 and prep.plan is None and prep.windows == [None, None]
    chans = _channels(wav, SR, dev)[:, :240 * 1600].cpu().numpy()
    want = conversation_audio(chans, stats, R, normalize)
    for p in range(2):
        assert prep.audio[p].shape == (R, 240 * 1600, 2)
        assert np.array_equal(prep.audio[p].cpu().numpy(), want[p]), f"person {p}"
        assert np.array_equal(prep.dual_audio[p], person_audio(chans, p, stats[p], normalize)[1]), f"person {p} dual audio"
    # routing on the device: under equal stats (one mean for both channels) person 1 hears person 0's channels swapped
    eq = {**stats[0], "audio_mean": np.array([0.002, 0.002])}
    same = prepare_conversation(wav.T, SR, (eq, eq), R, normalize=normalize, device=dev)
    assert torch.equal(same.audio[1], same.audio[0].flip(-1))
    assert np.array_equal(same.audio[0].cpu().numpy(), conversation_audio(chans, (eq, eq), R, normalize)[0])
    one = prepare_conversation((wav[:, 0], wav[:, 1]), SR, (None, stats[1]), R, normalize=normalize, device=dev, people=(False, True))
    assert one.audio[0] is None and torch.equal(one.audio[1], prep.audio[1])


def test_silent_channel(dev):
    wav = _recording(5.0).astype(np.float32) / 32768.0
    wav[:, 1] = 0.0
    stats = (_stats(), _stats())
    with pytest.raises(_lib.A2PError, match="peak of channel 1"):
        prepare_conversation(wav, SR, stats, 1, normalize="peak", device=dev)
    prep = prepare_conversation(wav, SR, stats, 1, normalize="none", device=dev)
    z, _ = person_audio(_channels(wav, SR, dev)[:, :prep.T * 1600].cpu().numpy(), 0, stats[0], "none")
    assert np.array_equal(prep.audio[0][0].cpu().numpy(), z.astype(np.float32))


def test_long_prepare_windows(dev):
    wav = _recording(45.0)
    stats = (_stats(), _stats_b())
    prep = prepare_conversation(wav, SR, stats, 2, device=dev)
    assert prep.T == 1320 and prep.plan.W >= 2
    for p in range(2):
        assert torch.equal(prep.windows[p], window_gather(prep.audio[p], prep.plan, k=1600))


# ---------------------------------------------------------------------------------------------- the pipeline by hand

def _by_hand(ms, stats, audio_np, R, seed, sampler, dev, plan=None):
    """Person p's building blocks: y["audio"] of the restatement -> shared features -> guide keyframes (seed's uniforms) -> body
    loop, and the face loop, with generate_from_recording's (plan None) or generate_from_long_recording's draws."""
    face_m, face_d = ms["face"]
    pose_m, pose_d = ms["pose"]
    fm, pm = face_m.model, pose_m.model
    audio = torch.from_numpy(audio_np).to(dev)
    T_total = audio.shape[1] // 1600
    W = 1 if plan is None else plan.W
    T = T_total if plan is None else plan.T_w
    if plan is not None:
        audio = window_gather(audio, plan, k=1600)
    B, nk = R * W, len(range(T)[::30])
    n_u = nk * pm.tokenizer.residual_depth
    uniforms = torch.stack([torch.rand(n_u, generator=torch.Generator().manual_seed(derive_seed(seed, 1, r) if w == 0 else
                                                                                    derive_seed(seed, 1, r, w)))
                            for r in range(R) for w in range(W)], dim=1)
    noise_pose = per_sample_noise((R, pm.nfeats, 1, T_total), [derive_seed(seed, 2, r) for r in range(R)]).to(dev)
    noise_face = per_sample_noise((R, fm.nfeats, 1, T_total), [derive_seed(seed, 3, r) for r in range(R)]).to(dev)
    with torch.no_grad():
        feats = pm.audio_frontend.encode_audio(audio)
        y_face = {"cond_embed": fm.audio_frontend.encode_lip(audio, feats), "scale": torch.full((B,), 10.0, device=dev)}
        guide_y = {"cond_embed": feats, "keyframes": torch.zeros(B, nk, pm.nfeats, device=dev)}
        kf = _replace_keyframes({"y": guide_y}, pose_m, uniforms, top_p=0.97).to(dev)
        y_body = {"cond_embed": feats, "keyframes": kf, "mask": torch.ones(B, 1, 1, T, dtype=torch.bool, device=dev),
                  "scale": torch.full((B,), 2.0, device=dev)}
        if plan is None:
            loop = lambda d: d.ddim_sample_loop if sampler == "ddim" else d.dpm_solver_sample_loop
            face = loop(face_d)(face_m, (R, fm.nfeats, 1, T), noise=noise_face, clip_denoised=False, model_kwargs={"y": y_face})
            body = loop(pose_d)(pose_m, (R, pm.nfeats, 1, T), noise=noise_pose, clip_denoised=False, model_kwargs={"y": y_body})
        else:
            face = windowed_sample_loop(face_d, face_m, plan, R, y_face, noise_face, sampler=sampler)
            body = windowed_sample_loop(pose_d, pose_m, plan, R, y_body, noise_pose, sampler=sampler)
    kf = kf.cpu().numpy()
    if plan is not None:
        kf = kf.reshape(R, W, nk, pm.nfeats)
    return {"face": face.squeeze(2).cpu().numpy().transpose(0, 2, 1) * stats["code_std"] + stats["code_mean"],
            "pose": body.squeeze(2).cpu().numpy().transpose(0, 2, 1) * stats["pose_std"] + stats["pose_mean"],
            "keyframes": kf * stats["pose_std"] + stats["pose_mean"]}


@pytest.mark.parametrize("seconds,sampler", [(8.0, "dpm++2m"), (45.0, "ddim")])
def test_generate_conversation_is_its_building_blocks(dev, seconds, sampler):
    A, B = _models(dev, "fp32"), _other_models(dev)
    stats = (_stats(), _stats_b())
    wav = _recording(seconds)
    R = 1
    got = generate_conversation((_person(A, stats[0]), _person(B, stats[1])), wav, SR, num_repetitions=R, seed=SEED, sampler=sampler)
    T = got["T"]
    long = T > 600
    plan = plan_windows(T) if long else None
    assert (T == 240) if not long else (T == 1320 and len(got["window_starts"]) >= 2 and got["window_starts"] == plan.starts)
    chans = _channels(wav, SR, dev)[:, :T * 1600].cpu().numpy()
    want_audio = conversation_audio(chans, stats, R)
    for p, (ms, seed) in enumerate(zip((A, B), person_seeds(SEED))):
        want = _by_hand(ms, stats[p], want_audio[p], R, seed, sampler, dev, plan)
        for k in KEYS:
            assert np.array_equal(got["people"][p][k], want[k]), f"person {p}: {k}"
        assert np.array_equal(got["people"][p]["audio"], person_audio(chans, p, stats[p])[1])


def test_swap_symmetry_and_overlap(dev):
    A, B = _models(dev, "fp32"), _other_models(dev)
    sa, sb = _stats(), _stats_b()
    wav = _recording(8.0)
    ab = generate_conversation((_person(A, sa), _person(B, sb)), wav, SR, seed=(3, 5))
    ba = generate_conversation((_person(B, sb), _person(A, sa)), wav[:, ::-1], SR, seed=(5, 3))
    assert _same(ab["people"][0], ba["people"][1]) and _same(ab["people"][1], ba["people"][0])
    seq = generate_conversation((_person(A, sa), _person(B, sb)), wav, SR, seed=(3, 5), overlap=False)
    assert all(_same(ab["people"][p], seq["people"][p]) for p in range(2)), "the two-stream schedule changed the samples"


def _rewrapped(ms):
    """The same denoisers and diffusions under new wrapper objects: generate_conversation then takes the per-person path."""
    from audio2photoreal_amd.model.cfg_sampler import ClassifierFreeSampleModel
    return {k: (ClassifierFreeSampleModel(m.model), d) for k, (m, d) in ms.items()}


@pytest.mark.parametrize("precision", ["fp32", "fp16"])
def test_batching_rule_and_partner_only(dev, precision):
    # fp32 at T = 240, R = 1: one batch of 2 sequences vs two of 1; the fp32 mode takes the per-operation kernels and the
    # 64-row GEMM tiles at both batch sizes (and no attn3_kernel, which only the 16-bit modes take)
    A = _models(dev, precision)
    st = _stats()
    wav = _recording(8.0)
    batched = generate_conversation((_person(A, st), _person(A, st)), wav, SR, seed=SEED, overlap=True)
    split = generate_conversation((_person(A, st), _person(_rewrapped(A), st)), wav, SR, seed=SEED, overlap=True)
    alone = generate_conversation((_person(A, st), None), wav, SR, seed=SEED, overlap=False)
    assert batched["T"] == 240 and batched["sr"] == 48000 and "window_starts" not in batched and alone["people"][1] is None
    for res in (batched, split):
        for p in range(2):
            r = res["people"][p]
            assert r["face"].shape == (1, 240, 256) and r["pose"].shape == (1, 240, 104) and r["keyframes"].shape == (1, 8, 104)
            assert r["audio"].shape == (2, 384000) and all(np.isfinite(r[k]).all() for k in KEYS)
    assert _same(alone["people"][0], split["people"][0]), "a partner who is only heard changed the animated person"
    if precision == "fp32":
        for p in range(2):
            assert _same(batched["people"][p], split["people"][p]), f"batching changed person {p}"
        assert _same(alone["people"][0], batched["people"][0])
    else:
        for p in range(2):
            for k in KEYS:
                assert _rel(batched["people"][p][k], split["people"][p][k]) < 1e-3, (p, k)
    # the own voice matters: the two people of one recording move differently
    assert not np.array_equal(batched["people"][0]["face"], batched["people"][1]["face"])


def test_long_conversation_batched_fp16(dev):
    A = _models(dev, "fp16")
    st = _stats()
    res = generate_conversation((_person(A, st), _person(A, st)), _recording(45.0), SR, seed=SEED, chain_keyframes=True)
    W = len(res["window_starts"])
    assert res["T"] == 1320 and W >= 2 and 2 * W <= MAX_BATCH
    for p in range(2):
        r = res["people"][p]
        assert r["face"].shape == (1, 1320, 256) and r["pose"].shape == (1, 1320, 104) and r["keyframes"].shape == (1, W, 20, 104)
        assert r["window_starts"] == res["window_starts"] and all(np.isfinite(r[k]).all() for k in KEYS)
