"""audio2photoreal_amd/avatar.py on the host: the chunk loop, the --frames window, the clip front's checks and their texts, the
asset lookup, the per-device tables of HostNet, and the stages' command-line options against tests/golden/cli_options.json
(written by tests/tools/cli_options.py before the stages' front ends were merged into avatar.py)."""
import json
import os
import re
import sys
import types

import numpy as np
import pytest
import torch

from audio2photoreal_amd import avatar as AV
from audio2photoreal_amd._lib import A2PError

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("pose_motion", "decode_motion", "render_rgb_motion", "encode_motion", "render_codes_motion", "render_conversation_motion")
PER_FRAME = 8
BUDGETS = {"below one frame": lambda N: 3, "exactly two frames": lambda N: 2 * PER_FRAME, "above N frames": lambda N: (N + 3) * PER_FRAME}


@pytest.mark.parametrize("budget", sorted(BUDGETS))
@pytest.mark.parametrize("N", [0, 1, 5])
def test_frame_chunks_tile_the_frames_in_order(N, budget):
    max_bytes = BUDGETS[budget](N)
    pairs = list(AV.frame_chunks(N, max_bytes, PER_FRAME))
    size = max(1, max_bytes // PER_FRAME)
    assert pairs == [(a, min(N, a + size)) for a in range(0, N, size)]
    assert [a for a, _ in pairs[1:]] == [b for _, b in pairs[:-1]]                # each chunk starts where the last one ended
    if N == 0:
        assert pairs == []
    else:
        assert pairs[0][0] == 0 and pairs[-1][1] == N and all(0 < b - a <= size for a, b in pairs)
        assert all(b - a == size for a, b in pairs[:-1])


@pytest.mark.parametrize("text, want", [(None, slice(None, None)), ("2:5", slice(2, 5)), (":5", slice(None, 5)), ("2:", slice(2, None)),
                                        (":", slice(None, None))])
def test_frame_window_is_the_slice_the_commands_took(text, want):
    def inline(x):                                                            # the code every main() held
        if text is not None:
            a, _, b = text.partition(":")
            x = x[slice(int(a) if a else None, int(b) if b else None)]
        return x
    x = np.arange(7)
    assert AV.frame_window(text) == want
    assert np.array_equal(x[AV.frame_window(text)], inline(x))


@pytest.mark.parametrize("entry", ENTRIES)
def test_clip_frames_refuses_a_host_without_gpu_and_a_wrong_width(entry, monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for poses in (np.zeros((2, 3, 10), np.float32), torch.zeros(6, 10), np.zeros((2, 10, 1, 3), np.float32)):
        with pytest.raises(A2PError, match=re.escape(f"{entry} runs on the MI355X; there is no CPU implementation")):
            AV.clip_frames(entry, poses, 10)
    with pytest.raises(A2PError, match=re.escape("motion must be [B, T, 10], [B, 10, 1, T] or [N, 10] (got [2, 3, 9])")):
        AV.clip_frames(entry, np.zeros((2, 3, 9), np.float32), 10)


@pytest.mark.parametrize("name, trailing", [("embs", (4,)), ("face_embs", (4,)), ("face_codes", (4,)), ("geom", (5, 3))])
def test_per_frame_holds_an_operand_against_the_leading_axes(name, trailing):
    lead = (2, 3)
    x = np.arange(6 * int(np.prod(trailing)), dtype=np.float64).reshape(*lead, *trailing)
    got = AV.per_frame(x, name, lead, trailing, "cpu")
    assert got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (6, *trailing)
    assert np.array_equal(got.numpy(), x.reshape(6, *trailing).astype(np.float32))
    assert tuple(AV.per_frame(x[:, :0], name, (2, 0), trailing, "cpu").shape) == (0, *trailing)
    want = [*lead, *trailing]
    for bad in (x[:, :2], x[..., :-1], x.reshape(6, *trailing)):               # wrong leading axes, wrong width, flat frames
        with pytest.raises(A2PError, match=re.escape(f"{name} must be {want} (got {list(bad.shape)})")):
            AV.per_frame(bad, name, lead, trailing, "cpu")


def test_cameras_checks_the_count_and_defaults_the_position():
    from audio2photoreal_amd.render import look_at
    pairs = [look_at([0.0, 0.0, 3.0 + c], [0.0, 0.0, 0.0], [0, 1, 0], 24, 32, 40.0) for c in range(2)]
    K, Rt = torch.stack([k for k, _ in pairs]), torch.stack([r for _, r in pairs])
    K2, Rt2, pos, C = AV.cameras(K.numpy(), Rt.double(), None, "cpu")
    assert C == 2 and K2.dtype == Rt2.dtype == pos.dtype == torch.float32 and torch.equal(K2, K) and torch.equal(Rt2, Rt)
    assert torch.allclose(pos, torch.tensor([[0.0, 0.0, 3.0], [0.0, 0.0, 4.0]]), atol=1e-6)
    given = [[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]]
    assert torch.equal(AV.cameras(K, Rt, given, "cpu")[2], torch.tensor(given))
    for k, rt in ((K, Rt[:1]), (K[0], Rt[0]), (K[:0], Rt[:0]), (K[:, :2], Rt)):
        with pytest.raises(A2PError, match=re.escape(f"K must be [C, 3, 3] and Rt [C, 3, 4] with C >= 1 cameras (got {list(k.shape)} and {list(rt.shape)})")):
            AV.cameras(k, rt, None, "cpu")
    with pytest.raises(A2PError, match=re.escape("camera_pos must be [2, 3] (got [1, 3])")):
        AV.cameras(K, Rt, given[:1], "cpu")


def test_the_compatibility_checks_keep_their_texts_and_take_a_prefix():
    ns = types.SimpleNamespace
    skeleton, decoder = ns(P_pos=104), ns(n_pose_dims=97, n_embs=8, n_face_embs=4)
    AV.check_pose_width(ns(P_pos=103), decoder)
    AV.check_embedding_widths(ns(n_embs=8), ns(n_embs=4), decoder)
    for prefix in ("", "avatars[1]: "):
        with pytest.raises(A2PError, match="^" + re.escape(f"{prefix}the skeleton takes 104 pose parameters; the decoder 6 + n_pose_dims = 103") + "$"):
            AV.check_pose_width(skeleton, decoder, prefix)
        with pytest.raises(A2PError, match="^" + re.escape(f"{prefix}the encoders give 8 / 5 embedding values; the decoder takes 8 / 4") + "$"):
            AV.check_embedding_widths(ns(n_embs=8), ns(n_embs=5), decoder, prefix)
    AV.check_body_embs("per_frame"), AV.check_body_embs("rest")
    with pytest.raises(A2PError, match=re.escape("body_embs='mean': need 'per_frame' or 'rest'")):
        AV.check_body_embs("mean")


@pytest.mark.parametrize("container", [dict, lambda **kw: types.SimpleNamespace(**kw)], ids=["dict", "attributes"])
def test_asset_reads_both_containers_and_names_what_is_missing(container):
    assets = container(tex_mean=1, keys_like=2)
    assert AV.asset(assets, "tex_mean") == 1 and AV.asset(assets, "keys_like", needed=("a", "b")) == 2
    with pytest.raises(ValueError, match="^" + re.escape("the assets hold no `seam_data_2048`") + "$"):
        AV.asset(assets, "seam_data_2048")
    with pytest.raises(ValueError, match="^" + re.escape("the assets hold no `face_cond_mask` (needed: pose_cond_mask, face_cond_mask)") + "$"):
        AV.asset(assets, "face_cond_mask", needed=("pose_cond_mask", "face_cond_mask"))


def test_hostnet_keeps_one_table_set_per_device():
    class Net(AV.HostNet):
        @classmethod
        def from_state_dict(cls):
            self = object.__new__(cls)
            self.params, self._dev = {"w": np.arange(6, dtype=np.float32).reshape(2, 3)[:, ::2], "i": np.arange(3, dtype=np.int32)}, {}
            return self

    with pytest.raises(TypeError, match="use Net.from_state_dict"):
        Net()
    net = Net.from_state_dict()
    cpu, meta = net._tables("cpu"), net._tables(torch.device("meta"))
    assert cpu is not meta and net._tables(torch.device("cpu")) is cpu and net._tables("meta") is meta and sorted(net._dev) == ["cpu", "meta"]
    assert cpu["w"].device.type == "cpu" and meta["w"].device.type == "meta" and meta["i"].dtype == torch.int32
    assert cpu["w"].is_contiguous() and np.array_equal(cpu["w"].numpy(), net.params["w"]) and tuple(meta["w"].shape) == (2, 2)


def test_load_block_names_the_missing_key_as_the_commands_did(tmp_path):
    path = str(tmp_path / "results.npy")
    np.save(path, {"motion": np.ones(2), "pose": np.zeros(3)})
    (motions,) = AV.load_block(path, ("motions", "motion"))
    assert np.array_equal(motions, np.ones(2)) and np.array_equal(AV.load_block(path, "pose")[0], np.zeros(3))
    with pytest.raises(A2PError, match=re.escape(f"{path} holds no `face` (keys: ['motion', 'pose'])") + "$"):
        AV.load_block(path, "pose", "face")
    with pytest.raises(A2PError, match=re.escape(f"{path} holds no `vertices` (keys: ['motion', 'pose']); run the skinning command without --joints-only")):
        AV.load_vertices(path)
    np.save(path, {"pose": np.zeros(3)})
    with pytest.raises(A2PError, match=re.escape(f"{path} holds neither `motions` nor `motion` (keys: ['pose'])") + "$"):
        AV.load_block(path, ("motions", "motion"))
    with pytest.raises(A2PError, match=re.escape("the frames are rendered on the MI355X; there is no CPU implementation")):
        with pytest.MonkeyPatch.context() as mp:
            mp.setattr(torch.cuda, "is_available", lambda: False)
            AV.require_gpu("the frames are rendered")


def test_every_command_keeps_its_options():
    sys.path.insert(0, os.path.join(ROOT, "tests", "tools"))
    try:
        import cli_options
    finally:
        sys.path.pop(0)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "cli_options.json")))
    got = cli_options.cli_options()
    assert sorted(got) == sorted(want) and len(want) == 9                      # eight commands; video has two parsers
    for command in want:
        have, held = {a["dest"]: a for a in got[command]["actions"]}, {a["dest"]: a for a in want[command]["actions"]}
        assert sorted(have) == sorted(held), command
        for dest in held:
            assert have[dest] == held[dest], (command, dest)
        assert got[command]["prog"] == want[command]["prog"]


def test_no_stage_imports_an_underscore_name_from_a_sibling():
    for module in ("avatar", "skinning", "surface", "render", "decoder", "texture", "encoder", "scene", "video"):
        text = open(os.path.join(ROOT, "audio2photoreal_amd", f"{module}.py")).read()
        assert not re.findall(r"from \.\w+ import .*\b_[A-Za-z]\w*", text), module
        assert re.findall(r"^from \. import .*$", text, re.M) in (["from . import _lib"], ["from . import _lib, avatar"]), module
    top = re.findall(r"^(?:from|import) .*$", open(os.path.join(ROOT, "audio2photoreal_amd", "avatar.py")).read(), re.M)
    assert [line for line in top if line.startswith("from .")] == ["from . import _lib", "from ._lib import A2PError"]
