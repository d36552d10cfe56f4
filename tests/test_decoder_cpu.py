"""Host side of the decoder layers (audio2photoreal_amd/decoder.py) and their numpy restatement (tests/decoder_restatement.py)
against the reference's ConvDecoder stored in tests/golden/golden_decoder_v1.npz.  No GPU."""
import os

import numpy as np
import pytest

import decoder_restatement as R
from audio2photoreal_amd import decoder as D
from audio2photoreal_amd import surface as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_decoder_v1.npz"))


@pytest.fixture(scope="module")
def fx():
    return R.make_fixture()


@pytest.fixture(scope="module")
def surface(fx):
    s = fx["surf"]
    return S.BodySurface.from_arrays(s["vi"], s["vt"], s["vti"], n_verts=s["n_verts"], uv_size=48)


def build(fx, surface, params=None, assets=None, **over):
    cfg = dict(fx["cfg"], **over)
    sd = {"decoder." + k: v for k, v in (fx["params"] if params is None else params).items()}
    return D.BodyDecoder.from_state_dict(sd, fx["assets"] if assets is None else assets, surface, **cfg)


def test_the_generated_fixture_is_the_one_the_reference_ran_on(gold, fx):
    prints = R.fingerprint(fx["params"])
    stored = {k.split("/", 1)[1]: float(gold[k]) for k in gold.files if k.startswith("fingerprint/")}
    assert prints == stored
    for k in ("motion", "embs", "face_embs"):
        assert np.array_equal(gold[k], fx[k]), k


def test_restatement_reproduces_the_reference_decoder(gold, fx):
    """float64 restatement against the reference's float32 ConvDecoder: on the stored elements the difference, normalised by the
    output's largest value, stays inside e_ref, which was measured over every element."""
    keep = {}
    want = R.decoder_forward(fx["params"], fx["cfg"], fx["assets"], fx["surf"], fx["motion"], fx["embs"], fx["face_embs"], keep=keep)
    rows = slice(int(gold["rows_start"]), None, int(gold["rows_step"]))
    pick = lambda a: a[..., rows, :] if a.shape[-2] >= 128 else a
    checked = 0
    for k in gold.files:
        if not k.startswith("ref/"):
            continue
        name = k[len("ref/"):]
        whole = keep[name[len("block/"):]] if name.startswith("block/") else want[name]      # every element, both frames
        sub = pick(whole[:1] if name.startswith("block/") else whole)                        # the stored part
        e_ref = float(gold[f"e_ref/{name}"])
        assert 0 < e_ref < 1e-5, name                                         # a float32 rounding error, not a formula error
        assert gold[k].shape == sub.shape and gold[k].dtype == np.float32, name
        err = float(np.abs(gold[k].astype(np.float64) - sub).max() / np.abs(whole).max())
        assert err <= e_ref, (name, err, e_ref)
        checked += 1
    assert checked == 10


def test_weight_folding_and_fused_keys(fx, surface):
    rs = np.random.RandomState(0)
    v, g = rs.randn(6, 4, 3, 3).astype(np.float32), rs.rand(6, 1, 1, 1).astype(np.float32) + 0.5
    w = D.fold_weight_norm(v, g)
    want = R.fold(v, g)
    assert w.dtype == np.float32 and np.array_equal(w, want.astype(np.float32))       # float64 throughout, rounded once
    assert R.nerr(w, v.astype(np.float64) * g / np.linalg.norm(v.astype(np.float64))) < 1e-7
    lin = D.fold_weight_norm(v.reshape(6, 36), g.reshape(6, 1))
    assert np.array_equal(lin, w.reshape(6, 36))
    split = build(fx, surface)
    fused = {}
    for k, a in fx["params"].items():
        if k.endswith(".weight_v"):
            fused[k[:-2]] = D.fold_weight_norm(a, fx["params"][k[:-2] + "_g"])
        elif not k.endswith(".weight_g"):
            fused[k] = a
    assert not any(k.endswith(("_g", "_v")) for k in fused)
    whole = build(fx, surface, params=fused)
    assert set(whole.params) == set(split.params) and len(split.params) == 2 * (3 * 11 + 2 + 2)
    for k in split.params:
        assert split.params[k].dtype == np.float32 and np.array_equal(split.params[k], whole.params[k]), k
    assert split.n_channels == [8, 4, 4] and split.sizes == [64, 128, 256]


def test_loader_refusals(fx, surface):
    p = dict(fx["params"])
    del p["conv_blocks.1.conv2.weight_g"]
    with pytest.raises(ValueError, match=r"no `conv_blocks\.1\.conv2\.weight_g` \(expected shape \[8, 1, 1, 1\]\)"):
        build(fx, surface, params=p)
    p = dict(fx["params"])
    p["embs_conv_block.2.conv1.bias"] = np.zeros((128, 32, 31), np.float32)
    with pytest.raises(ValueError, match=r"`embs_conv_block\.2\.conv1\.bias` has shape \[128, 32, 31\]; the configuration expects \[128, 32, 32\]"):
        build(fx, surface, params=p)
    with pytest.raises(ValueError, match="init_uv_size=32: only 64 is supported"):
        build(fx, surface, init_uv_size=32)
    with pytest.raises(ValueError, match="uv_size=192"):
        build(fx, surface, uv_size=192)
    a = dict(fx["assets"])
    a["face_cond_mask"] = np.zeros((64, 63), np.float32)
    with pytest.raises(ValueError, match=r"assets `face_cond_mask` has shape \[64, 63\]; the configuration expects \[64, 64\]"):
        build(fx, surface, assets=a)
    del a["face_cond_mask"]
    with pytest.raises(ValueError, match="the assets hold no `face_cond_mask`"):
        build(fx, surface, assets=a)
    with pytest.raises(ValueError, match=r"`conv_blocks\.0\.conv_resize\.weight_v` has shape \[8, 8, 1, 1\]; the configuration expects \[16, 8, 1, 1\]"):
        build(fx, surface, n_min_channels=8)


def test_seam_pair_resolution():
    ij = lambda *f: np.array([[v // 8, v % 8] for v in f])
    a, b, c, d = 3, 12, 21, 30
    # a chain a -> b, b -> c: both pairs stay, and since sources are read first c receives the original b
    dst, src = D.resolve_seam_pairs(ij(b, c), ij(a, b), 6, 8)
    assert dst.tolist() == [b, c] and src.tolist() == [a, b]
    value = np.arange(2 * 3 * 48, dtype=np.float32).reshape(2, 3, 6, 8)
    got = R.impaint(value, ij(b, c), ij(a, b)).reshape(2, 3, 48)
    flat = value.reshape(2, 3, 48)
    assert np.array_equal(got[:, :, c], flat[:, :, b]) and np.array_equal(got[:, :, b], flat[:, :, a])
    # a duplicated destination takes the last pair, in its place in the list
    dst, src = D.resolve_seam_pairs(ij(b, c, b, d), ij(a, a, d, c), 6, 8)
    assert dst.tolist() == [c, b, d] and src.tolist() == [a, d, c]
    rd, rsrc = R.resolve_pairs(ij(b, c, b, d), ij(a, a, d, c))
    assert (rd[:, 0] * 8 + rd[:, 1]).tolist() == dst.tolist() and (rsrc[:, 0] * 8 + rsrc[:, 1]).tolist() == src.tolist()
    with pytest.raises(ValueError, match=r"dst_ij\[1, 1\] = 8 is outside \[0, W=8\)"):
        D.resolve_seam_pairs(np.array([[0, 0], [5, 8]]), np.array([[0, 0], [1, 1]]), 6, 8)
    with pytest.raises(ValueError, match=r"src_ij\[0, 0\] = -1 is outside \[0, H=6\)"):
        D.resolve_seam_pairs(np.array([[0, 0]]), np.array([[-1, 0]]), 6, 8)
    seam = D.SeamSampler({"dst_ij": ij(b, c, b), "src_ij": ij(a, a, d), "uvs": np.zeros((6, 8, 2), np.float32), "weights": np.zeros((6, 8, 1))})
    assert (seam.H, seam.W, seam.P) == (6, 8, 2) and seam.weights.shape == (6, 8)
    with pytest.raises(ValueError, match=r"weights must be \[6, 8\] or \[6, 8, 1\]"):
        D.SeamSampler({"dst_ij": ij(b), "src_ij": ij(a), "uvs": np.zeros((6, 8, 2), np.float32), "weights": np.zeros((8, 6))})
