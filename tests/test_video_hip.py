"""The GPU JPEG encoder and the video writer (audio2photoreal_amd/video.py, csrc/kernels_video.h) against tests/jpeg_restatement.py:
coefficients element by element against float64, entropy coding byte for byte on crafted coefficients, whole streams, the AVI
container, and render_codes_video."""
import os
import wave

import numpy as np
import pytest
import torch

import jpeg_restatement as J
from audio2photoreal_amd import _lib
from audio2photoreal_amd import encoder as E
from audio2photoreal_amd import video as V
from audio2photoreal_amd._lib import A2PError
from conftest import record
from test_render_codes_hip import body, nets, scene  # noqa: F401  (fixtures: the small ladders of the render tests)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUALITIES, SUBS = (50, 90, 100), ("420", "444")
CANARY = 0xA5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "GPU tests need the MI355X"
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def images():
    return J.source_images()


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(ROOT, "tests", "golden", "golden_video_v1.npz"))


def up(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


# ------------------------------------------------------------------------------------------------ 1. coefficients
def check_coefficients(got, frames, q, s):
    """got [N, rows, cols, bpm, 64] int16 against the float64 quotients: exact outside the ties, within 1 near them.  A coefficient
    is near a tie when F / Q lies within 2^-7 / Q of a half-integer (2^-7 bounds the fp32 error of F: a 64-term sum whose absolute
    terms add up to at most 1024, plus the colour transform's).  Returns (share of ties, mismatches near ties)."""
    ties = near = 0
    for n, img in enumerate(frames):
        a, Q = J.quotients64(img, q, s)
        want = np.rint(a)
        want[..., 1:] = np.clip(want[..., 1:], -1023, 1023)
        tie = np.abs(a - np.floor(a) - 0.5) < 2.0 ** -7 / Q
        diff = got[n].astype(np.int64) - want
        assert got[n].shape == a.shape
        assert not diff[~tie].any(), (q, s, n, int(np.count_nonzero(diff[~tie])), float(np.abs(diff).max()))
        assert np.abs(diff).max() <= 1
        ties, near = ties + int(tie.sum()), near + int(np.count_nonzero(diff))
    return ties / (len(frames) * a.size), near


@pytest.mark.parametrize("s", SUBS)
@pytest.mark.parametrize("q", QUALITIES)
def test_coefficients_equal_float64_outside_ties(dev, images, q, s):
    got = V.coefficients(up(images, dev), q, s)
    assert got.dtype == torch.int16 and tuple(got.shape) == (3, *V.mcu_grid(40, 72, s), 64)
    got = got.cpu().numpy()
    share, near = check_coefficients(got, images, q, s)
    f32 = max(float(np.abs(J.quotients64(img, q, s)[0] - J.quotients64(img, q, s, np.float32)[0]).max()) for img in images)
    record(f"video_coef_q{q}_{s}", tie_share=share, mismatches_near_ties=near, numpy_f32_vs_f64_quotient=f32,
           differs_from_rint_f64=int((got != np.stack([J.coefficients(i, q, s) for i in images])).sum()))
    assert share <= 0.02, share
    for n in range(3):                                                         # a frame alone gives the bits it gives among others
        assert np.array_equal(V.coefficients(up(images[n:n + 1], dev), q, s).cpu().numpy()[0], got[n]), n


@pytest.mark.parametrize("s", SUBS)
def test_coefficients_edge_replication_and_strides(dev, s):
    rng = np.random.default_rng(11)
    for h, w in ((16, 16), (8, 8), (17, 33), (1, 1), (33, 300)):                 # 300: more than one strip of 256 pixels
        img = rng.integers(0, 256, size=(2, h, w, 3), dtype=np.uint8)
        got = V.coefficients(up(img, dev), 90, s).cpu().numpy()
        assert got.shape[1:4] == V.mcu_grid(h, w, s)
        check_coefficients(got, img, 90, s)
    for w in (72, 33):                                                         # panels read in place: 4-byte loads (72) and single bytes (33)
        panels = rng.integers(0, 256, size=(3, 40, 2 * w, 3), dtype=np.uint8)
        t = up(panels, dev)
        for c in range(2):
            view = t[:, :, c * w:(c + 1) * w]
            assert not view.is_contiguous()
            got = V.coefficients(view, 90, s)
            assert torch.equal(got, V.coefficients(view.contiguous(), 90, s))
            check_coefficients(got.cpu().numpy(), panels[:, :, c * w:(c + 1) * w], 90, s)
        odd = t.reshape(-1)[1:1 + 2 * 40 * 2 * w * 3].reshape(2, 40, 2 * w, 3)   # a base address that is no multiple of 4
        assert torch.equal(V.coefficients(odd, 90, s), V.coefficients(odd.clone(), 90, s))


# ------------------------------------------------------------------------------------------------ 2. entropy coding
def crafted(kind, shape, rng):
    """int16 [N, rows, cols, bpm, 64] of the named content."""
    N, rows, cols, bpm, _ = shape
    c = np.zeros(shape, np.int16)
    flat = c.reshape(-1, 64)
    j = np.arange(len(flat))
    swing = np.where(j % 2 == 0, 1023, -1024)          # neighbouring blocks, and the first block of a row: differences of +-2047 and
    if kind == "zero":                                 # -1024 / 1023 after the predictor's restart
        pass
    elif kind == "only63":
        flat[:, 63] = np.where(j % 3 == 0, -1, 7 + j % 50)
    elif kind == "runs":
        for i, run in enumerate((15, 16, 17, 32, 47, 48, 62)):
            rows_ = flat[i::7]
            rows_[:, 1 + run] = (-1) ** i * (1 + 37 * i)
            if run < 47:
                rows_[1::2, 63] = 3                     # and a second run up to the last coefficient on every other block
        flat[:, 0] = rng.integers(-60, 60, size=len(flat))
    elif kind == "alternating":
        flat[:, 1:] = np.tile([1023, -1, -1023, 1], 16)[:63]
        flat[:, 0] = swing
    elif kind == "worst":                              # category 11 DC differences, 63 AC coefficients of category 10
        flat[:, 1:] = np.where(rng.random((len(flat), 63)) < 0.5, 1, -1) * rng.integers(512, 1024, size=(len(flat), 63))
        flat[:, 0] = swing
    elif kind == "dcswing":
        flat[:, 0] = swing
    elif kind == "stuffing":                           # amplitudes of all ones behind codes that start with ones
        flat[:, 1:] = 1023
        flat[:, 0] = np.where(j % 2 == 0, 1023, -1024)
        flat[::5, 1:] = 0
        flat[::5, 0] = 1023
    elif kind == "sparse":
        flat[:] = rng.integers(-1023, 1024, size=flat.shape) * (rng.random(flat.shape) < 0.1)
        flat[:, 0] = rng.integers(-1024, 1024, size=len(flat))
    else:
        raise KeyError(kind)
    return c


KINDS = ("zero", "only63", "runs", "alternating", "worst", "dcswing", "stuffing", "sparse")


@pytest.mark.parametrize("bpm", (6, 3))
@pytest.mark.parametrize("grid", ((2, 2, 3), (1, 1, 70), (1, 9, 1)), ids=("2x3x2", "1x70", "9x1"))
def test_entropy_coding_is_the_restatement_s_byte_for_byte(dev, grid, bpm):
    """Lossless, so no tolerance.  Every frame sits behind 8 untouched bytes and the stream in front of 64: one stray byte anywhere
    breaks the equality.  1 x 70: more than 64 blocks in an interval, so bits are carried between chunks; 9 x 1: RST7 is followed by
    RST0; "worst" fills all 64 lanes of a chunk with the longest blocks these tables allow (1658 bits for luminance: 9 + 11 for the DC
    difference, 63 times 16 + 10), just under the 1665 the kernel reserves per block."""
    N, rows, cols = grid
    rng = np.random.default_rng(100 * rows + cols + bpm)
    for kind in KINDS:
        coef = crafted(kind, (N, rows, cols, bpm, 64), rng)
        want = [J.entropy_segment(coef[n]) for n in range(N)]
        if kind == "stuffing":
            assert any(b"\xff\x00\xff\x00" in w for w in want), "the pattern yields no run of 0xFF bytes"
        if kind == "worst":
            assert max(len(w) for w in want) >= rows * cols * (bpm - 2) * 1658 // 8      # a luminance block: 9 + 11 + 63 (16 + 10) bits
        stream, offsets = V.entropy_segments(up(coef, dev), gap=8, slack=64, fill=CANARY)
        lengths = np.diff(offsets) - 8
        assert list(lengths) == [len(w) for w in want], kind
        expect = b"".join(bytes([CANARY]) * 8 + w for w in want) + bytes([CANARY]) * 64
        got = stream.cpu().numpy().tobytes()
        assert len(got) == len(expect)
        assert got == expect, (kind, next(i for i, (a, b) in enumerate(zip(got, expect)) if a != b))
        if kind == "sparse":                                                   # the coded bytes do not depend on N or the frame's index
            alone, off1 = V.entropy_segments(up(coef[N - 1:], dev))
            assert alone.cpu().numpy().tobytes() == want[-1] and list(off1) == [0, len(want[-1])]


def test_entropy_values_out_of_range_are_clamped(dev):
    """Any int16 array is taken: an AC coefficient beyond +-1023 and a DC difference beyond +-2047 code as the limit, which keeps a
    block inside the capacity the kernel reserves."""
    coef = np.zeros((1, 1, 2, 3, 64), np.int16)
    coef[..., 1:] = np.where(np.arange(63) % 2, 32767, -32768)
    coef[0, 0, :, :, 0] = [[32767, -32768, 32767], [-32768, 32767, -32768]]
    clamped = np.clip(coef, -1023, 1023)
    clamped[0, 0, :, :, 0] = [[2047, -2047, 2047], [0, 0, 0]]                     # differences of +-2047, then -+2047, per component
    stream, offsets = V.entropy_segments(up(coef, dev), slack=16, fill=CANARY)
    want = J.entropy_segment(clamped[0])
    assert stream.cpu().numpy().tobytes() == want + bytes([CANARY]) * 16 and list(offsets) == [0, len(want)]


# ------------------------------------------------------------------------------------------------ 3. streams
@pytest.mark.parametrize("s", SUBS)
def test_streams_are_header_entropy_eoi(dev, images, gold, s):
    for q in QUALITIES:
        t = up(images, dev)
        data, off = V.encode_jpeg_frames(t, q, s)
        coef = V.coefficients(t, q, s).cpu().numpy()
        assert data.dtype == np.uint8 and off.dtype == np.int64 and off[0] == 0 and off[-1] == len(data)
        psnr = []
        for n in range(3):
            got = data[off[n]:off[n + 1]].tobytes()
            assert got == J.header(40, 72, q, s) + J.entropy_segment(coef[n]) + b"\xff\xd9", (q, n)
            head, back = J.decode_coefficients(got)
            assert np.array_equal(back, coef[n]) and head["size"] == (40, 72)
            psnr.append(J.psnr(J.decode(got), images[n]))
        record(f"video_stream_q{q}_{s}", psnr_restatement_decoder=[round(p, 3) for p in psnr],
               psnr_pillow_own_files=[round(float(p), 3) for p in gold[f"pil/{q}_{s}/psnr"]], bytes=[int(b) for b in np.diff(off)],
               bytes_pillow=[int(b) for b in gold[f"pil/{q}_{s}/bytes"]])
        # chunks of one frame's coefficients give the same stream
        data1, off1 = V.encode_jpeg_frames(t, q, s, max_bytes=1)
        assert np.array_equal(data1, data) and np.array_equal(off1, off)
    empty, off = V.encode_jpeg_frames(t[:0], 90, s)
    assert len(empty) == 0 and list(off) == [0]


# ------------------------------------------------------------------------------------------------ 4. container
def test_write_video_round_trip(dev, images, tmp_path, monkeypatch):
    rng = np.random.default_rng(8)
    frames = up(np.concatenate([images, images[::-1], images[:1]]), dev)       # 7 frames
    data, off = V.encode_jpeg_frames(frames, 90, "420")
    want = [data[off[n]:off[n + 1]].tobytes() for n in range(7)]
    for fps, rate, channels, samples in ((30, 48000, 1, 48000 // 30 * 7), (30, 48000, 2, 5000), (3, 44101, 2, 44101 * 3 + 5), (2, None, 0, 0)):
        audio = None if rate is None else rng.uniform(-1.2, 1.2, size=(samples, channels) if channels > 1 else (samples,))
        path = tmp_path / f"clip_{fps}_{channels}.avi"
        assert V.write_video(path, frames, fps=fps, audio=audio, audio_rate=rate) == 7
        got = V.read_video(path)
        assert got["frames"] == want and got["fps"] == fps and got["size"] == (40, 72)
        if audio is None:
            assert got["audio"] is None and got["audio_rate"] is None
        else:
            pcm = J.pcm16(audio)
            assert np.array_equal(got["audio"], pcm[:, 0] if channels == 1 else pcm) and got["audio_rate"] == rate
            assert open(path, "rb").read() == J.avi_mux(want, 40, 72, fps, pcm, rate)
        two = tmp_path / "two.avi"                                             # two write calls equal one
        with V.MJPEGWriter(two, 40, 72, fps=fps, audio=audio, audio_rate=rate) as w:
            assert w.write(frames[:4]) == 4 and w.write(frames[4:]) == 7
        assert open(two, "rb").read() == open(path, "rb").read()
    # 4:4:4 and another quality reach the file
    V.write_video(tmp_path / "q.avi", frames[:2], quality=50, subsampling="444")
    d50, o50 = V.encode_jpeg_frames(frames[:2], 50, "444")
    assert V.read_video(tmp_path / "q.avi")["frames"] == [d50[o50[n]:o50[n + 1]].tobytes() for n in range(2)]
    # the size guard, with a small limit
    whole = os.path.getsize(tmp_path / "clip_2_0.avi")
    monkeypatch.setattr(V, "AVI_LIMIT", whole - 1)
    w = V.MJPEGWriter(tmp_path / "guard.avi", 40, 72, fps=2)
    assert w.write(frames[:6]) == 6
    with pytest.raises(ValueError, match="2 GiB"):
        w.write(frames[6:])
    w.close()
    assert V.read_video(tmp_path / "guard.avi")["frames"] == want[:6] and os.path.getsize(tmp_path / "guard.avi") <= V.AVI_LIMIT


def test_error_paths(dev, images, tmp_path):
    t = up(images, dev)
    with pytest.raises(A2PError, match="uint8"):
        V.encode_jpeg_frames(t.float())
    with pytest.raises(A2PError, match="MI355X"):
        V.encode_jpeg_frames(t.cpu())
    with pytest.raises(A2PError, match=r"\[N, H, W, 3\]"):
        V.encode_jpeg_frames(t[0])
    with pytest.raises(A2PError, match=r"\[N, H, W, 3\]"):
        V.encode_jpeg_frames(t[..., :2])
    with pytest.raises(ValueError, match="subsampling"):
        V.encode_jpeg_frames(t, subsampling="422")
    with pytest.raises(ValueError, match="quality"):
        V.encode_jpeg_frames(t, quality=0)
    with pytest.raises(A2PError, match="int16"):
        V.entropy_segments(torch.zeros(1, 1, 1, 3, 64, device=dev))
    with pytest.raises(A2PError, match="3 or 6"):
        V.entropy_segments(torch.zeros(1, 1, 1, 4, 64, dtype=torch.int16, device=dev))
    with V.MJPEGWriter(tmp_path / "e.avi", 40, 72) as w:
        with pytest.raises(A2PError, match="40 x 72"):
            w.write(t[:, :32])
    lib, stream = _lib.load(), _lib.current_stream(dev)
    q, out = torch.ones(128, dtype=torch.int16, device=dev), torch.zeros(6 * 64, dtype=torch.int16, device=dev)
    assert lib.a2p_jpeg_coefficients(_lib.ptr(t), 1, 40, 72, 40 * 72 * 3, 72 * 3, 422, _lib.ptr(q), _lib.ptr(out), stream) == -1
    assert b"subsampling" in lib.a2p_last_error()
    assert lib.a2p_jpeg_coefficients(_lib.ptr(t), 1, 40, 72, 40 * 72 * 3, 71 * 3, 420, _lib.ptr(q), _lib.ptr(out), stream) == -1
    assert b"row_stride" in lib.a2p_last_error()
    assert lib.a2p_jpeg_coefficients(_lib.ptr(t), 1, 8, 8, 40 * 72 * 3, 72 * 3, 444, _lib.ptr(q), _lib.ptr(t), stream) == -1
    assert b"alias" in lib.a2p_last_error()
    assert lib.a2p_jpeg_coefficients(_lib.ptr(t), 0, 8, 8, 40 * 72 * 3, 72 * 3, 444, _lib.ptr(q), _lib.ptr(out), stream) == 0     # N = 0: no launch
    i64 = torch.zeros(4, dtype=torch.int64, device=dev)
    assert lib.a2p_jpeg_entropy(_lib.ptr(out), 1, 1, 1, 4, _lib.ptr(q), None, 0, None, 0, _lib.ptr(i64), _lib.ptr(i64[2:]), None, 0, stream) == -1
    assert b"blocks_per_mcu" in lib.a2p_last_error()


# ------------------------------------------------------------------------------------------------ 5. rendering into a file, the command line
def test_render_codes_video_equals_encoding_the_rendered_frames(dev, body, tmp_path):  # noqa: F811
    b = body
    audio = np.random.default_rng(2).uniform(-1, 1, size=(1234, 2))
    with torch.cuda.device(dev):
        frames = E.render_codes_motion(*nets(b), b["frames"][:2], b["codes"][:2], b["K"], b["Rt"])
        data, off = V.encode_jpeg_frames(frames, 90, "420")
        n = V.render_codes_video(*nets(b), b["frames"][:2], b["codes"][:2], b["K"], b["Rt"], tmp_path / "clip.avi", audio=audio, audio_rate=16000,
                                 slice_frames=1)                               # 2 frames in two slices
    got = V.read_video(tmp_path / "clip.avi")
    assert n == 2 and got["frames"] == [data[off[i]:off[i + 1]].tobytes() for i in range(2)]
    assert got["size"] == tuple(frames.shape[1:3]) and got["fps"] == 30 and np.array_equal(got["audio"], J.pcm16(audio))
    back = J.decode(got["frames"][1])                                          # and it is a picture of the frame
    assert J.psnr(back, frames[1].cpu().numpy()) > 25
    with pytest.raises(A2PError, match="one sequence"):
        V.render_codes_video(*nets(b), b["frames"][None].expand(2, -1, -1), b["codes"][None].expand(2, -1, -1), b["K"], b["Rt"], tmp_path / "x.avi")


def test_command_line_file_demuxes_to_the_frames_and_samples(dev, images, tmp_path):
    pcm = np.random.default_rng(4).integers(-32768, 32768, size=(2500, 2), dtype=np.int16)
    with wave.open(str(tmp_path / "clip.wav"), "wb") as f:
        f.setnchannels(2), f.setsampwidth(2), f.setframerate(22050)
        f.writeframes(pcm.astype("<i2").tobytes())
    np.save(tmp_path / "frames.npy", images[None])                                  # [1, 3, 40, 72, 3]
    argv = ["--frames", str(tmp_path / "frames.npy"), "--audio", str(tmp_path / "clip.wav"), "--out", str(tmp_path / "clip.avi"), "--fps", "25",
            "--quality", "50", "--subsampling", "444", "--slice-frames", "2"]
    with torch.cuda.device(dev):
        assert V.main(argv) == 0
        data, off = V.encode_jpeg_frames(up(images, dev), 50, "444")
    got = V.read_video(tmp_path / "clip.avi")
    assert got["frames"] == [data[off[n]:off[n + 1]].tobytes() for n in range(3)] and got["fps"] == 25 and got["size"] == (40, 72)
    assert got["audio_rate"] == 22050 and np.array_equal(got["audio"], pcm)     # a 16-bit wav file's samples as they are stored
    with wave.open(str(tmp_path / "clip8.wav"), "wb") as f:                     # other widths: scaled to [-1, 1), then to 16 bits
        f.setnchannels(1), f.setsampwidth(1), f.setframerate(8000)
        f.writeframes(bytes([0, 64, 128, 255]))
    audio, rate = V.wav_audio(tmp_path / "clip8.wav")
    assert rate == 8000 and V.pcm16(audio)[:, 0].tolist() == [-32767, -16384, 0, 32511]
