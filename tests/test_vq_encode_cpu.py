"""Keyframes from known poses, host side: the float64 restatement of the VQ encode against the reference's vectors, the codec's
encoder parameters, and every refusal of the new options before any GPU work."""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import vq_encode_restatement as VE
from audio2photoreal_amd import _lib
from audio2photoreal_amd.model.guide import GuideTransformer
from audio2photoreal_amd.model.vqvae import TemporalVertexCodec
from audio2photoreal_amd.sample.recording import continue_recording, generate_from_recording, regenerate_segment
from audio2photoreal_amd.spec import TokenizerSpec, tokenizer_encoder_param_shapes, tokenizer_param_shapes
from audio2photoreal_amd.synthetic import synthetic_tokenizer_encoder_state_dict, synthetic_tokenizer_state_dict

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 10


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(HERE, "golden", "golden_vq_encode_v1.npz"))


def _sd():
    ts = TokenizerSpec()
    return ts, {**synthetic_tokenizer_state_dict(ts, SEED), **synthetic_tokenizer_encoder_state_dict(ts, SEED)}


@pytest.mark.parametrize("inputs", ["randn", "decoded"])
def test_float64_restatement_matches_the_reference(golden, inputs):
    ts, sd = _sd()
    poses = torch.from_numpy(golden[f"{inputs}/poses"])
    lat = VE.encoder(sd, poses)
    want = torch.from_numpy(golden[f"{inputs}/latents"]).double()
    assert float((lat - want).norm() / want.norm()) < 1e-6
    assert float((lat - want).abs().max() / want.abs().max()) < 1e-6
    # the reference's fp32 tokens; every margin of the fixture is far above fp32 rounding, so float64 picks the same codes
    assert golden[f"{inputs}/margin"].min() > 1e-3
    assert torch.equal(VE.quantize(sd, want, ts.residual_depth), torch.from_numpy(golden[f"{inputs}/tokens"]))
    assert torch.equal(VE.encode(sd, poses, ts.residual_depth), torch.from_numpy(golden[f"{inputs}/tokens"]))


def test_encoder_keys_are_the_references():
    """The codec built with an encoder has the reference codec's keys minus the EMA statistics and `project_mean_shape` (which
    neither encode nor decode reads); the decode-only codec and the existing spec are unchanged."""
    ts = TokenizerSpec()
    t = TemporalVertexCodec(ts.n_vertices, ts.latent_dim, ts.categories, ts.residual_depth, with_encoder=True)
    got = {k: tuple(v.shape) for k, v in t.state_dict().items()}
    assert got == {**tokenizer_param_shapes(ts), **tokenizer_encoder_param_shapes(ts)}
    ref = {f"encoder.enc.{i}.{p}" for i in (0, 2, 4, 6, 8) for p in ("weight", "bias")} | set(tokenizer_param_shapes(ts))
    assert set(got) == ref
    t.load_state_dict(_sd()[1])                     # strict
    assert t.has_encoder and t.predict == t.encode
    plain = TemporalVertexCodec(ts.n_vertices, ts.latent_dim, ts.categories, ts.residual_depth)
    assert not plain.has_encoder and set(plain.state_dict()) == set(tokenizer_param_shapes(ts))


def test_construction_leaves_the_global_rng_alone():
    ts = TokenizerSpec()
    torch.manual_seed(3)
    TemporalVertexCodec(ts.n_vertices, ts.latent_dim, ts.categories, ts.residual_depth)
    want = torch.rand(5)
    torch.manual_seed(3)
    TemporalVertexCodec(ts.n_vertices, ts.latent_dim, ts.categories, ts.residual_depth, with_encoder=True)
    assert torch.equal(torch.rand(5), want)


def test_encode_needs_an_encoder_and_the_gpu():
    t = TemporalVertexCodec(104, 64, 16, 4)
    with pytest.raises(_lib.A2PError, match="with_encoder"):
        t.encode(torch.zeros(1, 3, 104, device="meta"))
    t = TemporalVertexCodec(104, 64, 16, 4, with_encoder=True)
    with pytest.raises(_lib.A2PError, match="MI355X"):
        t.encode(torch.zeros(1, 3, 104))
    with pytest.raises(_lib.A2PError, match="MI355X"):
        t.encoder(torch.zeros(1, 3, 104))


# ------------------------------------------------------------------------------------------------------------ forced tokens
@pytest.mark.parametrize("value", [16, 17, -2, -100, 1 << 40])
def test_forced_tokens_out_of_range_are_refused_first(value):
    g = GuideTransformer(tokens=16, num_layers=1, dim=64, emb_len=64, num_audio_layers=1)
    forced = torch.full((2, 8), -1, dtype=torch.int64)
    forced[1, 5] = value
    with pytest.raises(_lib.A2PError, match="forced_tokens"):
        g.generate(torch.zeros(2, 100, 1024), 2, 4, n_sequences=2, max_key_len=2, max_seq_len=60, forced_tokens=forced)


@pytest.mark.parametrize("forced", [torch.full((2, 7), -1), torch.full((1, 8), -1), torch.full((2, 8), -1.0), np.full((2, 8), -1)])
def test_forced_tokens_shapes_and_dtypes_are_refused_first(forced):
    g = GuideTransformer(tokens=16, num_layers=1, dim=64, emb_len=64, num_audio_layers=1)
    with pytest.raises(_lib.A2PError, match="forced_tokens"):
        g.generate(torch.zeros(2, 100, 1024), 2, 4, n_sequences=2, max_key_len=2, max_seq_len=60, forced_tokens=forced)


def test_valid_forced_tokens_reach_the_gpu_check():
    g = GuideTransformer(tokens=16, num_layers=1, dim=64, emb_len=64, num_audio_layers=1)
    forced = torch.full((2, 8), -1, dtype=torch.int64)
    forced[:, :4] = torch.tensor([0, 15, 3, 7])
    with pytest.raises(_lib.A2PError, match="MI355X"):
        g.generate(torch.zeros(2, 100, 1024), 2, 4, n_sequences=2, max_key_len=2, max_seq_len=60, forced_tokens=forced)


# ------------------------------------------------------------------------------------------------------------ recording level
STATS = {"audio_mean": np.array([0.01, -0.02]), "audio_std_flat": np.array([0.3]),
         "code_mean": np.zeros(256), "code_std": np.ones(256), "pose_mean": np.zeros(104), "pose_std": np.ones(104)}
WAV4 = np.ones(48000 * 4 + 10, np.float32)      # 120 frames


def _pair(nfeats, guide=False, encoder=True):
    m = SimpleNamespace(audio_frontend=object(), seq_len=600, nfeats=nfeats)
    if guide:
        m.transformer = object()
        m.tokenizer = SimpleNamespace(has_encoder=encoder, residual_depth=4)
    return (SimpleNamespace(model=m), None)


FACE, POSE, POSE_NO_ENC = _pair(256), _pair(104, guide=True), _pair(104, guide=True, encoder=False)


def _result(R=2, T=240):
    return {"face": np.zeros((R, T, 256)), "pose": np.zeros((R, T, 104)), "keyframes": np.zeros((R, T // 30, 104)),
            "audio": np.zeros((2, T * 1600)), "T": T, "sr": 48000}


@pytest.mark.parametrize("P", [0, 45, 29, 120.5])
def test_continue_with_guide_context_refuses_context_off_the_grid(P):
    with pytest.raises(_lib.A2PError, match="multiple of 30"):
        continue_recording(FACE, POSE, STATS, WAV4, 48000, _result(), context_frames=P, guide_context=True)


def test_guide_context_needs_the_tokenizer_encoder():
    with pytest.raises(_lib.A2PError, match="with_encoder"):
        continue_recording(FACE, POSE_NO_ENC, STATS, WAV4, 48000, _result(), context_frames=120, guide_context=True)
    with pytest.raises(_lib.A2PError, match="with_encoder"):
        regenerate_segment(FACE, POSE_NO_ENC, STATS, _result(), 60, 120, guide_context=True)
    with pytest.raises(_lib.A2PError, match="with_encoder"):
        generate_from_recording(FACE, POSE_NO_ENC, STATS, WAV4, 48000, known_keyframes={0: np.zeros(104)})


def test_guide_context_passes_the_host_checks():
    """Valid calls stop where the GPU work starts: the fake models have no device."""
    with pytest.raises(AttributeError, match="null_cond_embed"):
        continue_recording(FACE, POSE, STATS, WAV4, 48000, _result(), context_frames=120, guide_context=True)
    with pytest.raises(AttributeError, match="null_cond_embed"):
        regenerate_segment(FACE, POSE, STATS, _result(), 60, 120, guide_context=True)
    with pytest.raises(AttributeError, match="null_cond_embed"):
        generate_from_recording(FACE, POSE, STATS, WAV4, 48000, known_keyframes={0: np.zeros(104), 90: torch.ones(104)})


@pytest.mark.parametrize("known,match", [
    ({}, "non-empty"), ([np.zeros(104)], "non-empty"), ({15: np.zeros(104)}, "multiple of 30"), ({120: np.zeros(104)}, "multiple of 30"),
    ({-30: np.zeros(104)}, "multiple of 30"), ({30.0: np.zeros(104)}, "multiple of 30"), ({True: np.zeros(104)}, "multiple of 30"),
    ({0: np.zeros(103)}, "104 values"), ({0: np.zeros((1, 104))}, "104 values"), ({60: np.full(104, np.nan)}, "non-finite"),
    ({0: np.zeros(104), 30: np.r_[np.zeros(103), np.inf]}, "non-finite")])
def test_bad_known_keyframes_are_refused_first(known, match):
    with pytest.raises(_lib.A2PError, match=match):
        generate_from_recording(FACE, POSE, STATS, WAV4, 48000, known_keyframes=known)


def test_replace_keyframes_refuses_bad_known_first():
    from audio2photoreal_amd.sample.generate import _replace_keyframes
    y = {"cond_embed": torch.zeros(2, 100, 1024), "keyframes": torch.zeros(2, 4, 104)}
    model = SimpleNamespace(transformer=None, tokenizer=None)
    ok_known, ok_mask = torch.zeros(2, 4, 104), torch.zeros(2, 4, dtype=torch.bool)
    for known, mask, match in ((torch.zeros(2, 3, 104), ok_mask, "known must be"), (ok_known, torch.zeros(2, 4), "known_mask"),
                               (ok_known, torch.zeros(2, 5, dtype=torch.bool), "known_mask"), (ok_known, None, "both"),
                               (torch.full((2, 4, 104), np.inf), ok_mask, "non-finite")):
        with pytest.raises(_lib.A2PError, match=match):
            _replace_keyframes({"y": y}, model, known=known, known_mask=mask)


def test_face_only_regenerate_with_guide_context_needs_no_encoder():
    """guide_context only concerns the body: a face-only re-roll goes on to the GPU work without a tokenizer encoder."""
    with pytest.raises(AttributeError, match="null_cond_embed"):
        regenerate_segment(FACE, POSE_NO_ENC, STATS, _result(), 60, 120, parts=("face",), guide_context=True)


@pytest.mark.parametrize("shape", [(1, 3, 103), (3, 104), (1, 1, 3, 104)])
def test_encode_refuses_pose_shapes_before_staging(shape, monkeypatch):
    t = TemporalVertexCodec(104, 64, 16, 4, with_encoder=True)
    monkeypatch.setattr(t, "_stage_encoder", lambda *a: pytest.fail("staged before the shape check"))
    with pytest.raises(_lib.A2PError, match="poses must be"):
        t.encode(torch.zeros(shape))
