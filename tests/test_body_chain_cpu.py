"""The end-to-end float64 chain of the body renderer (tests/body_chain_restatement.py) against the reference's own wiring stored in
tests/golden/golden_body_chain_v1.npz, the conditions its scene has to meet, and the miswirings its gates have to catch.  No GPU.

Gate of the reference's arrays: max |difference| / max |value| at most 4 x max(e_ref, 2^-24), e_ref being the reference's own
float32 error over every element as the golden maker measured it; the stored rows must not exceed it.  The float64 chain runs once
per module (about 15 s); each mutant reruns only what lies downstream of it."""
import os

import numpy as np
import pytest

import body_chain_restatement as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STAGE_OF = {"geom": "verts", "cond_view": "cond_view", "tex_view_rec": "tex_view_rec", "shadow_map": "shadow_map", "tex_mean_rec": "tex_mean_rec"}


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_body_chain_v1.npz"))


@pytest.fixture(scope="module")
def scene(gold):
    return B.draw_scene(int(gold["seed"]), int(gold["draw"]))


@pytest.fixture(scope="module")
def c64(scene):
    return B.chain(scene)


@pytest.fixture(scope="module")
def ex(gold, c64):
    return B.excluded(c64, gold["e_proj"], gold["e_depth"])


def test_the_scene_is_the_one_the_golden_file_was_made_from(gold, scene):
    prints = B.fingerprints(scene)
    stored = {k[len("fingerprint/"):] for k in gold.files if k.startswith("fingerprint/")}
    assert stored == set(prints)
    for k, v in prints.items():
        assert v == float(gold[f"fingerprint/{k}"]), k
    assert scene["K"].shape == (3, 3, 3) and scene["Rt"].shape == (3, 3, 4) and scene["size"] == (96, 128)
    eyes = -np.einsum("nrc,nr->nc", scene["Rt"][:, :, :3].astype(np.float64), scene["Rt"][:, :, 3].astype(np.float64))
    fx = scene["K"][:, 0, 0]
    for a in range(3):                                                        # three clearly different eyes and fields of view
        for b in range(a + 1, 3):
            assert np.linalg.norm(eyes[a] - eyes[b]) > 5.0 and abs(fx[a] - fx[b]) > 10.0, (a, b, eyes, fx)


@pytest.mark.parametrize("name", list(STAGE_OF))
def test_reference_wiring_against_the_chain(gold, c64, name):
    want = c64[STAGE_OF[name]]
    ref = gold[f"ref/{name}"]
    sub = want[..., int(gold["rows_start"])::int(gold["rows_step"]), :] if want.ndim == 4 and want.shape[-2] >= 128 else want
    assert ref.dtype == np.float32 and ref.shape == sub.shape, (ref.shape, sub.shape)
    e_ref = float(gold[f"e_ref/{name}"])
    err = float(np.abs(ref.astype(np.float64) - sub).max() / np.abs(want).max())      # the stored rows on the scale of every element
    allowance = 4 * max(e_ref, B.FLOOR)
    print(f"{name}: err {err:.3e} e_ref {e_ref:.3e} allowance {allowance:.3e}")
    assert np.isfinite(err) and err <= allowance, (name, err, allowance)
    # e_ref recomputed: the whole array where it is stored whole, else the stored rows cannot exceed the error over every element
    if sub is want:
        assert abs(err - e_ref) <= 1e-6 * e_ref, (name, err, e_ref)
    else:
        assert err <= e_ref * (1 + 1e-6), (name, err, e_ref)
    if name == "cond_view":
        cos = float(np.abs(ref[:, :1].astype(np.float64) - sub[:, :1]).max() / np.abs(want[:, :1]).max())
        assert cos <= float(gold["e_ref/view_cos_uv"]) * (1 + 1e-6) and 0.5 < np.abs(want[:, :1]).max() <= 1.0 + 1e-12


def test_scene_conditions(gold, c64, ex):
    facts = B.conditions(c64, ex)
    print(facts)
    assert B.failed(facts) == []
    assert min(facts["covered"]) >= 0.25 and max(facts["excluded"]) <= 0.02 and min(facts["twice"]) >= 0.05 and facts["clamped"] <= 0.5
    for k, v in facts.items():
        assert np.allclose(gold[f"cond/{k}"], v, rtol=0, atol=1e-12), k
    assert np.array_equal(gold["face"], c64["face"].astype(np.int16))
    assert np.array_equal(np.unpackbits(gold["excluded"])[:ex.size].reshape(ex.shape).astype(bool), ex)
    assert np.array_equal(gold["cond/excluded_pixels"], ex.sum(axis=(1, 2)))
    assert B.nerr(gold["rgb"], c64["rgb"]) <= 2.0 ** -23                        # stored as float32: one rounding of a value up to 255
    hit = c64["face"] >= 0
    assert not c64["render"].transpose(0, 2, 3, 1)[~hit].any() and np.isfinite(c64["second"][hit & ~ex]).any()


@pytest.mark.parametrize("name", list(B.MUTANTS))
def test_mutant_is_detected(gold, scene, c64, ex, name):
    kept = (c64["face"] >= 0) & ~ex
    ratio, where = B.mutant_ratio(c64, B.chain(scene, mutant=name, base=c64), kept, B.allowances(gold))
    print(f"{name} ({B.MUTANTS[name][1]}): {ratio:.3g} allowances on {where}")
    assert ratio >= 10, (name, ratio, where)
    assert abs(ratio - float(gold[f"mutant/{name}"])) <= 1e-6 * ratio


def test_mutants_reuse_what_lies_upstream(scene, c64):
    m = B.chain(scene, mutant="texture_v_flipped", base=c64)
    assert all(m[k] is c64[k] for k in ("verts", "cond_view", "tex_rec", "face", "bary")) and m["render"] is not c64["render"]
    assert {"verts", "cond_view", "tex_view_rec", "shadow_map", "tex_rec", "face", "bary", "depth", "second", "render", "rgb"} <= set(c64)
